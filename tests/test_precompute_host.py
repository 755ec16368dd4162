"""tests/precompute_reference.py on the CPU: the float64 reference of the precomputed inner products is pinned to exact integer
arithmetic and to the oracle, and the error bounds the GPU tests assert (tests/test_gpu_precompute.py) are shown to be far below
what a wrong element, a dropped row or a missing weight changes on the very datasets those tests use."""
import numpy as np
import pytest

import oracle as O
import precompute_reference as R


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_is_exact_on_integers(weighted):
    """0/1/2 genotypes and integer weights: S equals integer arithmetic, T equals S (no negative term); with signed integers T is
    the sum of the absolute products."""
    n, p = 300, 2 * 64 + 37
    X = R.integer_genotypes(n, p, 1)
    w = R.integer_weights(n, 1) if weighted else None
    Xi = X.astype(np.int64)
    Wi = Xi * (w.astype(np.int64)[:, None] if weighted else 1)
    G = Xi.T @ Wi
    assert G.max() < 2 ** 24
    S, T = R.products(X, w, slice(0, p), slice(0, p))
    assert np.array_equal(S, G) and np.array_equal(T, G)
    sx, tx = R.xpx(X, w)
    assert np.array_equal(sx, np.diag(G)) and np.array_equal(tx, np.diag(G))
    for k, (j0, b) in enumerate(R.partition(p, 64)):
        assert np.array_equal(R.gram(X, w, j0, b)[0], G[j0:j0 + b, j0:j0 + b])
        if k:
            assert np.array_equal(R.cross(X, w, j0 - 64, 64, j0, b)[0], G[j0 - 64:j0, j0:j0 + b])
    for level, gb in ((1, 128), (2, 256)):
        for i in range(1, (p + gb - 1) // gb):
            S1, _ = R.group_cross(X, w, 64, level, i)
            assert np.array_equal(S1, G[(i - 1) * gb:i * gb, i * gb:min((i + 1) * gb, p)])
    Z = (Xi - 1).astype(np.float32)                                       # -1/0/1
    S, T = R.products(Z, w, slice(0, p), slice(0, p))
    Zi = Xi - 1
    Zw = Zi * (w.astype(np.int64)[:, None] if weighted else 1)
    assert np.array_equal(S, Zi.T @ Zw) and np.array_equal(T, np.abs(Zi).T @ np.abs(Zw))


def test_partition_and_mirror_helpers():
    assert R.partition(165, 64) == [(0, 64), (64, 64), (128, 37)]
    assert [b for _, b in R.partition(R.EXPLICIT_P, starts=R.EXPLICIT_STARTS)] == [1, 63, 65, 1, 170, 170]
    M = np.arange(9.0).reshape(3, 3)
    assert np.array_equal(R.mirrored(M), [[0, 3, 6], [3, 4, 7], [6, 7, 8]])
    keep = np.zeros((3, 3), dtype=bool); keep[0, 1] = True
    assert np.array_equal(R.mirrored(M, keep), [[0, 1, 6], [3, 4, 7], [6, 7, 8]])
    assert R.padded_rows(3) == 256 and R.padded_rows(256) == 256 and R.padded_rows(257) == 512


def _f32_or_neighbour(o, S):
    s = S.astype(np.float32)
    return (o == s) | (o == np.nextafter(s, np.float32(np.inf))) | (o == np.nextafter(s, np.float32(-np.inf)))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("starts", [None, R.EXPLICIT_STARTS])
def test_reference_against_the_oracle(weighted, starts):
    """O.xpx, O.gram and O.cross_gram (ACC_F64: the same float64 products summed in row order, rounded to float32 once) on centred
    genotypes: the oracle's value is float32(S) or, where the two float64 sums straddle a rounding boundary, its float32
    neighbour.  The oracle mirrors the entries a >= c of a Gram."""
    n, p = (R.EXPLICIT_N, R.EXPLICIT_P) if starts else (257, 2 * 128 + 65)
    X = R.centred_genotypes(n, p, 4)
    w = R.positive_weights(n, 4) if weighted else None
    O.set_weights(w)
    try:
        assert _f32_or_neighbour(O.xpx(X, O.ACC_F64), R.xpx(X, w)[0]).all()
        blocks = R.partition(p, 128, starts)
        for k, (j0, b) in enumerate(blocks):
            S, _ = R.gram(X, w, j0, b)
            g = O.gram(X, j0, b, O.ACC_F64)
            assert _f32_or_neighbour(g, R.mirrored(S)).all(), k
            assert (g == R.mirrored(S).astype(np.float32)).mean() > 0.99   # (a neighbour is the rare exception)
            if k:
                jp, bp = blocks[k - 1]
                assert _f32_or_neighbour(O.cross_gram(X, jp, bp, j0, b, O.ACC_F64), R.cross(X, w, jp, bp, j0, b)[0]).all(), k
    finally:
        O.set_weights(None)


def _bounded_datasets():
    """The (X, w) pairs of the bounded GPU cases, by name."""
    out = {}
    for bs, p, n in R.UNIFORM_SHAPES:
        out[f"centred n={n} p={p}"] = (R.centred_genotypes(n, p, bs + n), None, bs)
        out[f"centred weighted n={n} p={p}"] = (R.centred_genotypes(n, p, bs + n), R.positive_weights(n, bs), bs)
    for centered in (True, False):
        out[f"packed centered={centered}"] = (R.packed_genotypes(300, 2 * 64 + 37, 9, centered)[2], R.positive_weights(300, 9), 64)
    out["explicit"] = (R.centred_genotypes(R.EXPLICIT_N, R.EXPLICIT_P, 6), R.positive_weights(R.EXPLICIT_N, 6), None)
    for bs, p, n, m in R.GROUP_SHAPES:                                    # (the pair cross-Grams are those of blocks of 2 bs markers)
        out[f"groups bs={bs} p={p} m={m}"] = (R.centred_genotypes(n, p, p + m), R.positive_weights(n, p), 2 * bs)
    out["two block sizes"] = (R.centred_genotypes(R.SECOND_SIZE_N, R.SECOND_SIZE_P, 21), R.positive_weights(R.SECOND_SIZE_N, 21), 64)
    return out


_DATA = _bounded_datasets()


@pytest.mark.parametrize("name", list(_DATA))
def test_bounds_see_a_dropped_row_a_swapped_column_and_a_missing_weight(name):
    """What the bounds are for: a kernel that leaves one individual out of a sum, reads the neighbouring marker, or forgets the
    weight on one operand.  In every Gram and cross-Gram of the GPU tests' datasets the change such a slip makes is at least 10x
    the looser ("mfma") bound on a good share of the entries -- for one dropped row a quarter of the entries that row contributes to
    (an entry whose two genotypes in that row are small moves little, one with a zero genotype there not at all; one entry past
    the bound suffices for a test to fail, a quarter of them leaves no doubt), half of all entries for a swapped column and for a
    missing weight.  The "f64" bound is tighter still, and checked to be."""
    X, w, bs = _DATA[name]
    n, p = X.shape
    blocks = R.partition(p, bs, None if bs else R.EXPLICIT_STARTS)
    ld = R.padded_rows(n)
    k = n // 2
    keep = np.arange(n) != k
    for i, (j0, b) in enumerate(blocks):
        for jp, bp in ([(j0, b)] if i == 0 else [(j0, b), blocks[i - 1]]):
            if b < 2:
                continue
            S, T = R.cross(X, w, jp, bp, j0, b)
            bound = R.bound_mfma(S, T)
            assert (R.bound_f64(S, T, ld) <= bound).all()
            Sd, _ = R.cross(X[keep], None if w is None else w[keep], jp, bp, j0, b)
            moved = np.abs(Sd - S)
            hit = moved > 0                     # (uncentred genotypes: a zero in that row leaves the entry where it was)
            assert hit.mean() >= 0.1 and (moved[hit] >= 10 * bound[hit]).mean() >= 0.25, (name, i, "row")
            swapped = S[:, np.arange(b) ^ 1 if b % 2 == 0 else np.r_[np.arange(b - 1) ^ 1, b - 1]]
            moved = np.abs(swapped - S)[:, :b - b % 2]
            assert (moved >= 10 * bound[:, :b - b % 2]).mean() >= 0.5, (name, i, "column")
            if w is not None:
                Su, _ = R.cross(X, None, jp, bp, j0, b)
                assert (np.abs(Su - S) >= 10 * bound).mean() >= 0.5, (name, i, "weight")
    sx, tx = R.xpx(X, w)
    sd, _ = R.xpx(X[keep], None if w is None else w[keep])
    assert (np.abs(sd - sx) >= 10 * R.bound_mfma(sx, tx)).mean() >= 0.25
