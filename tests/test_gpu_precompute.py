"""Every precomputed inner product, element by element (k_xpx, k_gram_f64, k_cross_f64, k_gram_mfma in both modes, k_cross_mfma128):
x'R^-1 x, the block Grams, the cross-Grams of consecutive blocks (jwas_hip_get_cross_gram level 0) and the pair / four cross-Grams
of grouped launches (levels 1, 2) against the plain float64 reference of tests/precompute_reference.py.

The bit-for-bit chain suites hand the device the oracle's products and the other chains touch an element only when its marker
changes; here nothing is replaced and nothing is sampled.

  * EXACT cases: uncentred 0/1/2 genotypes, weights 1 or small integers.  Every product and partial sum is an integer below 2^24:
    exact in float32, in the 64-row float32 chunks of the matrix-instruction kernels and in float64 -- both Gram modes and both
    storages must EQUAL the reference.
  * BOUNDED cases: centred genotypes, missing codes on packed storage, arbitrary positive weights, against the derived bounds of
    precompute_reference (bound_f64, bound_mfma); packed storage equals dense storage of the decoded columns bit for bit.

A Gram is DEFINED by its entries a >= c (the weight rides on the column operand, so S[a, c] and S[c, a] differ in the last bits
under weights); the device mirrors them, except in "mfma" mode under weights on the diagonal 64 x 64 tiles, which it computes in
full.  Symmetry is asserted exactly where the device mirrors (and on unweighted Grams everywhere), the bound on both triangles.
Every helper prints the largest error / bound it saw (pytest -s): a measurement, not a threshold."""
import numpy as np
import pytest

import precompute_reference as R
from jwas_jl_amd import streaming as S2

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUP = -1, -3, -4


@pytest.fixture(scope="module")
def engines():
    import jwas_jl_amd as J
    dense, packed = J.HipEngine(0), J.HipEngine(0)
    yield dense, packed
    dense.close(); packed.close()


@pytest.fixture(scope="module")
def hip(engines):
    return engines[0]


def _compare(G, S, T, mode, ld, exact, what):
    assert G.shape == S.shape, (what, G.shape, S.shape)
    if exact:
        assert np.array_equal(G, S.astype(np.float32)), (what, np.argwhere(G != S.astype(np.float32))[:5])
        return
    bound = R.bound_f64(S, T, ld) if mode == "f64" else R.bound_mfma(S, T)
    err = np.abs(G.astype(np.float64) - S)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"precompute[{mode}] {what}: max error / bound = {ratio:.4f}")
    assert (err <= bound).all(), (what, ratio, np.argwhere(err > bound)[:5])


def _check_blocks(e, X, w, mode, exact, starts=None):
    """x'x, every Gram and every cross-Gram of the selected block set of engine e."""
    n, p = X.shape
    ld = R.padded_rows(n)
    bs = e.block_size
    blocks = R.partition(p, bs, starts)
    assert e.nblocks == len(blocks)
    _compare(e.xpx(), *R.xpx(X, w), "f64", ld, exact, "x'x")             # (k_xpx accumulates in float64 in both modes)
    for k, (j0, b) in enumerate(blocks):
        S, T = R.gram(X, w, j0, b)
        a, c = np.indices((b, b))
        full = (a // 64 == c // 64) if (mode == "mfma" and w is not None) else np.zeros((b, b), dtype=bool)
        G = e.gram(k)
        _compare(G, R.mirrored(S, full), R.mirrored(T, full), mode, ld, exact, f"Gram {k} (bs {bs})")
        assert np.array_equal(G[~full], G.T[~full]), f"Gram {k}: not the mirror image where the device mirrors"
        if w is None or mode == "f64" or exact:
            assert np.array_equal(G, G.T), f"Gram {k} is not bit-symmetric"
        if k:
            jp, bp = blocks[k - 1]
            _compare(e.cross_gram(k), *R.cross(X, w, jp, bp, j0, b), mode, ld, exact, f"cross-Gram {k} (bs {bs})")


def _group_indices(p, bs, m, level):
    gb = (1 << level) * bs
    ngr = (p + gb - 1) // gb
    return [i for i in range(1, ngr) if not (m == 4 and level == 1 and i % 2 == 0)], ngr


def _check_groups(e, X, w, mode, exact, m):
    n, p = X.shape
    ld, bs = R.padded_rows(n), e.block_size
    out = {}
    for level in ((1, 2) if m == 4 else (1,)):
        idx, ngr = _group_indices(p, bs, m, level)
        for i in idx:                                  # (m = 4, level 1: pair 2q + 1, held at q, must come back as pair 2q + 1)
            G = e.group_cross_gram(level, i)
            _compare(G, *R.group_cross(X, w, bs, level, i), mode, ld, exact, f"group cross-Gram level {level} index {i} (bs {bs}, m {m})")
            out[level, i] = G
        for i in range(0, ngr + 1):
            if i not in idx:
                with pytest.raises(RuntimeError) as ei:
                    e.group_cross_gram(level, i)
                assert ei.value.code == EINVAL
                if m == 4 and level == 1 and 0 < i < ngr:
                    assert "odd pairs" in str(ei.value)
    if m == 2:
        with pytest.raises(RuntimeError) as ei:
            e.group_cross_gram(2, 1)
        assert ei.value.code == ESTATE
    return out


def _load_both(engines, X, w):
    """Uncentred 0/1/2 values without missing codes on both storages."""
    dense, packed = engines
    n, p = X.shape
    dense.load_dense(X)
    packed.load_packed2bit(S2.pack_2bit(X.astype(np.uint8)), n, X.mean(axis=0, dtype=np.float64).astype(np.float32), centered=False)
    assert np.array_equal(packed.get_columns(0, p), X)
    for e in engines:
        e.set_weights(w)


def _unit(engines):
    for e in engines:
        e.set_weights(None)


# ---- uniform blocks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", ["f64", "mfma"])
@pytest.mark.parametrize("bs,p,n", R.UNIFORM_SHAPES + [(64, 2 * 64 + 37, 3)])
def test_exact_integer_products_uniform_blocks(engines, bs, p, n, mode, weighted):
    X = R.integer_genotypes(n, p, bs + n)
    w = R.integer_weights(n, bs) if weighted else None
    try:
        _load_both(engines, X, w)
        for e in engines:
            e.setup_blocks(bs, mode)
            _check_blocks(e, X, w, mode, True)
    finally:
        _unit(engines)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", ["f64", "mfma"])
@pytest.mark.parametrize("bs,p,n", R.UNIFORM_SHAPES)
def test_bounded_products_uniform_blocks(hip, bs, p, n, mode, weighted):
    X = R.centred_genotypes(n, p, bs + n)
    w = R.positive_weights(n, bs) if weighted else None
    try:
        hip.load_dense(X)
        hip.set_weights(w)
        hip.setup_blocks(bs, mode)
        _check_blocks(hip, X, w, mode, False)
    finally:
        hip.set_weights(None)


@pytest.mark.parametrize("centered", [True, False])
@pytest.mark.parametrize("mode", ["f64", "mfma"])
def test_packed_with_missing_codes_equals_dense_and_meets_the_bounds(engines, mode, centered):
    """Missing fields decode to the marker mean (0 when centred): x'x, Grams, cross-Grams and the group cross-Grams of both group
    sizes from packed bytes equal those of dense storage of the decoded columns bit for bit, and meet the bounds."""
    dense, packed = engines
    n, p, bs = 300, 2 * 64 + 37, 64
    codes, means, X = R.packed_genotypes(n, p, 9, centered)
    w = R.positive_weights(n, 9)
    try:
        packed.load_packed2bit(S2.pack_2bit(codes), n, means, centered=centered)
        assert np.array_equal(packed.get_columns(0, p), X)
        dense.load_dense(X)
        got = []
        for e in engines:
            e.set_weights(w)
            e.setup_blocks(bs, mode)
            _check_blocks(e, X, w, mode, False)
            g = {"xpx": e.xpx()}
            for k in range(e.nblocks):
                g["gram", k] = e.gram(k)
                if k:
                    g["cross", k] = e.cross_gram(k)
            for m in (2, 4):
                e.setup_groups(m, mode)
                for key, v in _check_groups(e, X, w, mode, False, m).items():
                    g[(m,) + key] = v
            got.append(g)
        assert got[0].keys() == got[1].keys() and len(got[0]) >= 1 + 3 + 2 + 1 + 1
        for key in got[0]:
            assert np.array_equal(got[0][key], got[1][key]), key
    finally:
        _unit(engines)


# ---- an explicit partition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("mode", ["f64", "mfma"])
def test_explicit_partition(hip, mode, exact):
    """Blocks of 1, 63, 65, 1, 170 and 170 markers at a storage stride of 256: a predecessor shorter and longer than its successor,
    sizes on either side of a 64-marker tile, a one-marker block."""
    n, p = R.EXPLICIT_N, R.EXPLICIT_P
    X = R.integer_genotypes(n, p, 6) if exact else R.centred_genotypes(n, p, 6)
    w = R.integer_weights(n, 6) if exact else R.positive_weights(n, 6)
    try:
        hip.load_dense(X)
        hip.set_weights(w)
        hip.setup_blocks_explicit(np.array(R.EXPLICIT_STARTS), mode)
        assert hip.block_size == 256
        _check_blocks(hip, X, w, mode, exact, R.EXPLICIT_STARTS)
    finally:
        hip.set_weights(None)


# ---- grouped launches -------------------------------------------------------------------------------------------------------------
# bs = 64: 1 pair (no launch at all), 2 (a ragged last pair), 3 (a last pair shorter than one block), 5 (a last pair of one block);
# bs = 128 and a ragged last four; bs = 1024 at 65 rows: 4096-marker fours, the last one ragged


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("mode", ["f64", "mfma"])
@pytest.mark.parametrize("bs,p,n,m", R.GROUP_SHAPES)
def test_group_cross_grams(engines, bs, p, n, m, mode, exact):
    X = R.integer_genotypes(n, p, p + m) if exact else R.centred_genotypes(n, p, p + m)
    w = R.integer_weights(n, p) if exact else R.positive_weights(n, p)
    try:
        if exact:
            _load_both(engines, X, w)
        else:
            engines[0].load_dense(X)
            engines[0].set_weights(w)
        for e in (engines if exact else engines[:1]):
            e.setup_blocks(bs, mode)
            e.setup_groups(m, mode)
            got = _check_groups(e, X, w, mode, exact, m)
            npairs = (p + 2 * bs - 1) // (2 * bs)
            assert sorted(i for lv, i in got if lv == 1) == [i for i in range(1, npairs) if m == 2 or i % 2]
            _check_blocks(e, X, w, mode, exact)                            # (the block products are untouched by the groups)
    finally:
        _unit(engines)


@pytest.mark.parametrize("mode", ["f64", "mfma"])
def test_group_cross_grams_of_1024_marker_blocks(hip, mode):
    """4096-marker fours (a 32 x 32 grid of 128 x 128 tiles), the last four ragged; of the pairs only pair 1 exists."""
    n, bs, p = 65, 1024, 4096 + 1500
    X = R.integer_genotypes(n, p, 11)
    w = R.integer_weights(n, 11)
    try:
        hip.load_dense(X)
        hip.set_weights(w)
        hip.setup_blocks(bs, mode)
        hip.setup_groups(4, mode)
        got = _check_groups(hip, X, w, mode, True, 4)
        assert sorted(got) == [(1, 1), (2, 1)] and got[2, 1].shape == (4096, 1500)
    finally:
        hip.set_weights(None)


# ---- state: a second block size, weights after the set-up, the setter, the return codes ---------------------------------------------
@pytest.mark.parametrize("mode", ["f64", "mfma"])
def test_getters_follow_the_selected_block_size(hip, mode):
    n, p = R.SECOND_SIZE_N, R.SECOND_SIZE_P
    X = R.centred_genotypes(n, p, 21)
    w = R.positive_weights(n, 21)
    try:
        hip.load_dense(X)
        hip.set_weights(w)
        hip.setup_blocks(64, mode)
        hip.add_block_size(128, mode)
        hip.select_block_size(128)
        hip.setup_groups(2, mode)
        for bs in (128, 64, 128):
            hip.select_block_size(bs)
            _check_blocks(hip, X, w, mode, False)
            if bs == 128:
                _check_groups(hip, X, w, mode, False, 2)
            else:                                                         # (groups belong to the block size they were set up for)
                with pytest.raises(RuntimeError) as ei:
                    hip.group_cross_gram(1, 1)
                assert ei.value.code == ESTATE
    finally:
        hip.set_weights(None)


def test_weights_set_after_the_setup_drop_the_products(hip):
    n, p = 65, 2 * 64 + 37
    X = R.integer_genotypes(n, p, 31)
    w = R.integer_weights(n, 31)
    try:
        hip.load_dense(X)
        hip.setup_blocks(64, "mfma")
        hip.setup_groups(2, "mfma")
        _check_blocks(hip, X, None, "mfma", True)
        hip.set_weights(w)
        for call in (lambda: hip.cross_gram(1), lambda: hip.group_cross_gram(1, 1)):
            with pytest.raises(RuntimeError) as ei:
                call()
            assert ei.value.code == ESTATE
        hip.setup_blocks(64, "mfma")
        hip.setup_groups(2, "mfma")
        _check_blocks(hip, X, w, "mfma", True)
        _check_groups(hip, X, w, "mfma", True, 2)
        assert not np.array_equal(hip.cross_gram(1), R.cross(X, None, 0, 64, 64, 64)[0].astype(np.float32))
    finally:
        hip.set_weights(None)


def test_set_cross_gram_round_trips(hip):
    X = R.centred_genotypes(300, R.EXPLICIT_P, 41)
    hip.load_dense(X)
    hip.setup_blocks_explicit(np.array(R.EXPLICIT_STARTS), "f64")
    blocks = R.partition(R.EXPLICIT_P, starts=R.EXPLICIT_STARTS)
    rng = np.random.default_rng(41)
    sent = {k: rng.standard_normal((blocks[k - 1][1], blocks[k][1])).astype(np.float32) for k in range(1, len(blocks))}
    kept = hip.gram(2)
    for k, C in sent.items():
        hip.set_cross_gram(k, C)
    for k, C in sent.items():
        assert np.array_equal(hip.cross_gram(k), C), k
    assert np.array_equal(hip.gram(2), kept)


def test_cross_gram_getter_return_codes(hip):
    import jwas_jl_amd as J

    def code(f, *a):
        with pytest.raises(J.JwasHipError) as ei:
            f(*a)
        return ei.value.code

    X = R.integer_genotypes(65, 2 * 128 + 30, 51)
    hip.load_dense(X)                                                     # (loading drops every block set)
    assert code(hip.cross_gram, 1) == ESTATE
    assert code(hip.group_cross_gram, 1, 1) == ESTATE
    hip.setup_blocks(64, "f64")
    assert hip.nblocks == 5
    assert code(hip.cross_gram, 0) == EINVAL
    assert code(hip.cross_gram, 5) == EINVAL
    assert code(hip.cross_gram, -1) == EINVAL
    assert hip.cross_gram(4).shape == (64, 30)
    assert code(hip.group_cross_gram, 1, 1) == ESTATE                     # blocks, but no groups
    assert code(hip.group_cross_gram, 3, 1) == EINVAL                     # no such level
    hip.setup_groups(2, "f64")
    assert code(hip.group_cross_gram, 2, 1) == ESTATE                     # fours exist at 4 blocks per launch only
    assert code(hip.group_cross_gram, 1, 0) == EINVAL
    assert code(hip.group_cross_gram, 1, 3) == EINVAL                     # 3 pairs: indices 1 and 2
    assert hip.group_cross_gram(1, 2).shape == (128, 30)
    hip.setup_groups(4, "f64")
    assert code(hip.group_cross_gram, 1, 2) == EINVAL                     # the even pairs are part of the fours
    assert hip.group_cross_gram(1, 1).shape == (128, 128)
    assert hip.group_cross_gram(2, 1).shape == (256, 30)
    hip.setup_groups(0, "f64")
    assert code(hip.group_cross_gram, 1, 1) == ESTATE
    e64 = J.HipEngine(0, precision=64)
    try:
        e64.load_dense(X.astype(np.float64))
        e64.setup_blocks(64, "f64")
        assert code(e64.cross_gram, 1) == EUNSUP
        assert code(e64.group_cross_gram, 1, 1) == EUNSUP
    finally:
        e64.close()
