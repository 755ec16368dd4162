"""Mega-trait models on the device (csrc/mega.hpp) through the C ABI and runMCMC, against the numpy restatement of
tests/mega_reference.py on the same Philox counters.

Shapes: n = 301 individuals (two 256-row slices, the second ragged), p = 100 markers in blocks of 40 (three blocks, the last ragged;
a block of 40 runs the update kernel in four row parts, a block of 100 in two, blocks above 128 in one); T in {1, 5, 8, 9, 17, 64}
traits (8 is the trait tile of k_mega_update_partial), pi = 0, 0.5, 0.95 in turn.  The device and the restatement evaluate the same
formulas in double and differ in the ORDER of the O(n) sums and in the libm behind Box-Muller.  With u = 2^-53:

    x'x, G_jk      two summation orders of the same n products: 2 (n + 2) u sum_i |x_ij x_ik|; G symmetric, its diagonal x'x bit for bit
    indicators     discrete: EQUAL to the restatement's own chain for every marker and trait (mega_reference asserts that no decision
                   uniform of that chain lies within 1e-9 of probDelta1; tests/test_megatrait_host.py runs that check on the CPU)
    beta, alpha    every marker is compared with the restatement evaluated from the DEVICE's own history
                   (mega_reference.conditional_recheck): both sides start from the same doubles, and the bound is 2 (N + 2) u abs_s
                   carried through the scalar solve, plus the Box-Muller term of tests/test_gpu_sem.py (mega_reference.marker_bound)
    statistics     against numpy sums of the device's own state: 2 (K + 2) u sum |terms| for K terms; the counts exact
    residual       against the apply recomputed in numpy from the device's own change lists (the same IEEE operations in the same
                   order): within 4 u of the sum of the absolute terms.  Pad rows are not visible through the C ABI; the sweep's
                   sum r^2 and sum r run over them, so a pad row that moved would fail the statistics
    block sizes    under a tight prior (v / 100) the propagated bound of mega_reference.propagated_bound is meaningful, and two
                   block sizes differ by at most the sum of their bounds
Trait k of a T-trait session is compared with a one-trait session BIT FOR BIT: no sum of a trait depends on T.  Every test prints
the figures it measured before it asserts."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

import mega_reference as MR
from mega_reference import MegaStandInEngine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4
N, P, BS, SEED, LD = 301, 100, 40, 5, 512
TRAITS = (1, 5, MR.TRAIT_TILE, MR.TRAIT_TILE + 1, 17, 64)
CASES = [(T, prec) for T in TRAITS for prec in (32, 64)]
STAT_KEYS = ("sum_delta", "beta_ss", "alpha_ss", "resid_ss", "resid_sum", "n_changed")


@functools.lru_cache(maxsize=None)
def _case():
    cs = MR.make_case(N, P)
    assert not cs.missing[0].any() and 0.15 < cs.missing.mean() < 0.3 and (~cs.missing[:, :30]).sum(axis=0).min() == 1
    return cs


@functools.lru_cache(maxsize=None)
def _reference(iteration, bs=BS, vscale=1.0, T=64):
    """The restatement's own sweep of the first T traits from the common state (computed once, shared, never changed).  Trait k of it
    serves every session that holds trait k: the traits are independent chains, and the 1e-9 margin of every decision uniform
    (asserted inside) is far above the rounding by which numpy's sums move with the shape."""
    return MR.reference_sweep(_case(), T, iteration, SEED, bs, vscale)


def _engine(precision, T, bs=BS, first=0):
    import jwas_jl_amd as J
    hip = J.HipEngine(0, precision=precision)
    hip.load_dense(np.asfortranarray(_case().X.astype(hip.dtype)))
    hip.mega_begin(T, bs, first)
    return hip


def _upload(hip, c):
    hip.mega_set_residual(c.R)
    hip.mega_set_state(c.alpha, c.beta, c.delta)


def _sweep(hip, c, iteration, vscale=1.0):
    return hip.mega_sweep(iteration=iteration, seed=SEED, vare=c.vare, var_effect=c.v * vscale, pi=c.pi)


# ---- 1. x'x and the Grams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_gram_and_xpx(precision):
    cs = _case()
    Xa = np.abs(cs.X)
    hip = _engine(precision, 5)
    try:
        worst = 0.0
        for k, j0 in enumerate(range(0, P, BS)):
            b = min(BS, P - j0)
            G, xpx = hip.mega_gram(k)
            assert G.shape == (b, b) and xpx.shape == (b,)
            assert np.array_equal(G, G.T) and np.array_equal(np.diag(G), xpx)
            worst = max(worst, float((np.abs(G - MR.gram_block(cs.X, j0, b)) / (2 * (N + 2) * U * MR.gram_block(Xa, j0, b))).max()))
        print(f"Float{precision}: x'x and Gram worst error / bound {worst:.3f}")
        assert worst <= 1.0
    finally:
        hip.close()


def test_gram_beyond_one_grid_trip():
    """The Gram kernel's grid holds 32 768 blocks; with blocks of one marker p = 32 808 takes a second trip.  A small matrix tiled
    column-wise: the Gram of a one-marker block is x'x."""
    import jwas_jl_amd as J
    rng = np.random.default_rng(11)
    base = (rng.binomial(2, 0.4, size=(9, 8)) - rng.uniform(0.5, 1.1, 8)).astype(np.float32).astype(np.float64)
    p = 32768 + 40
    X = np.asfortranarray(np.tile(base, (1, p // 8 + 1))[:, :p].astype(np.float32))
    ref, refa = (base * base).sum(axis=0), (base * base).sum(axis=0)
    hip = J.HipEngine(0)
    try:
        hip.load_dense(X)
        hip.mega_begin(1, 1, 0)
        worst = 0.0
        for j in (0, 32767, 32768, 32769, p - 1):
            G, xpx = hip.mega_gram(j)
            assert G.shape == (1, 1) and G[0, 0] == xpx[0] and xpx[0] > 0
            worst = max(worst, float(abs(G[0, 0] - ref[j % 8]) / (2 * (9 + 2) * U * refa[j % 8])))
        print(f"second grid trip: worst error / bound {worst:.3f}")
        assert worst <= 1.0
    finally:
        hip.close()


# ---- 2. one sweep from a common uploaded state, iterations 1 and 2 ---------------------------------------------------------------------
@pytest.mark.parametrize("T,precision", CASES)
def test_sweep_indicators_effects_statistics_residual(T, precision):
    cs = _case()
    c = MR.case_traits(cs, T)
    hip = _engine(precision, T)
    try:
        for iteration in (1, 2):
            ref = _reference(iteration)
            _upload(hip, c)
            st = _sweep(hip, c, iteration)
            alpha, beta, delta = hip.mega_get_state()
            R = hip.mega_get_residual()
            nmis = int((delta != ref.delta[:T]).sum())
            print(f"T = {T} Float{precision} iteration {iteration}: {nmis} of {T * P} indicators differ; nearest threshold {ref.margins[:T].min():.2e}; "
                  f"{int(st['n_changed'].sum())} effects changed")
            assert nmis == 0
            assert np.array_equal(alpha, delta * beta) and set(np.unique(delta)) <= {0.0, 1.0}
            assert np.all(delta[np.flatnonzero(c.pi == 0.0)] == 1.0)                    # pi = 0 includes every marker
            # effects: every marker from the device's own history
            b_ref, bound = MR.conditional_recheck(cs.X, c.R, c.alpha, alpha, delta, iteration=iteration, seed=SEED, vare=c.vare, var_effect=c.v)
            wb = float((np.abs(beta - b_ref) / bound).max())
            print(f"    beta worst error / bound {wb:.3e} (largest bound {bound.max():.2e}, largest |beta| {np.abs(beta).max():.2e}); "
                  f"against the restatement's own chain: {np.abs(beta - ref.beta[:T]).max():.2e}")
            assert wb <= 1.0 and np.all(np.isfinite(beta))
            # statistics: the counts exact, the sums against numpy sums of the device's own state
            assert np.array_equal(st["sum_delta"], delta.sum(axis=1)) and np.array_equal(st["sum_delta"], ref.sum_delta[:T])
            assert np.array_equal(st["n_changed"], (alpha != c.alpha).sum(axis=1).astype(np.float64)) and np.array_equal(st["n_changed"], ref.n_changed[:T])
            w1 = float((np.abs(st["beta_ss"] - (beta * beta).sum(axis=1)) / (2 * (P + 2) * U * (beta * beta).sum(axis=1))).max())
            w2 = float((np.abs(st["alpha_ss"] - (alpha * alpha).sum(axis=1)) / (2 * (P + 2) * U * (alpha * alpha).sum(axis=1) + 1e-300)).max())
            w3 = float((np.abs(st["resid_ss"] - (R * R).sum(axis=1)) / (2 * (LD + 2) * U * (R * R).sum(axis=1))).max())
            w4 = float((np.abs(st["resid_sum"] - R.sum(axis=1)) / (2 * (LD + 2) * U * np.abs(R).sum(axis=1))).max())
            print(f"    statistics worst error / bound: beta'beta {w1:.3f}, alpha'alpha {w2:.3f}, sum r^2 {w3:.3f}, sum r {w4:.3f}")
            assert max(w1, w2, w3, w4) <= 1.0
            # the residual: the apply recomputed from the device's own change lists, markers ascending per trait
            Rn, d = c.R.copy(), c.alpha - alpha
            MR.apply_changes(Rn, cs.X, d)
            terms = np.abs(c.R) + np.abs(d) @ np.abs(cs.X).T
            wr = float((np.abs(R - Rn) / (4 * U * terms)).max())
            print(f"    residual worst error / bound {wr:.3f} ({'bit-equal' if np.array_equal(R, Rn) else 'not bit-equal'})")
            assert wr <= 1.0
    finally:
        hip.close()


# ---- 3. no sum of trait k depends on T ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_trait_k_is_bit_equal_to_a_one_trait_session(precision):
    cs = _case()
    c17 = MR.case_traits(cs, 17)
    hip = _engine(precision, 17)
    try:
        _upload(hip, c17)
        st17 = [_sweep(hip, c17, it) for it in (1, 2)]                   # (the second sweep applies the first one's last change list)
        full = (hip.mega_get_state(), hip.mega_get_residual())
    finally:
        hip.close()
    for k in (0, 8, 16):
        c1 = MR.case_traits(cs, 1, k)
        hip = _engine(precision, 1, first=k)
        try:
            _upload(hip, c1)
            st1 = [_sweep(hip, c1, it) for it in (1, 2)]
            one = (hip.mega_get_state(), hip.mega_get_residual())
        finally:
            hip.close()
        same = all(np.array_equal(one[0][q][0], full[0][q][k]) for q in range(3)) and np.array_equal(one[1][0], full[1][k])
        stats = all(a[key][0] == b[key][k] for a, b in zip(st1, st17) for key in STAT_KEYS)
        print(f"Float{precision} trait {k}: state and residual {'bit-equal' if same else 'DIFFER'}, statistics {'bit-equal' if stats else 'DIFFER'}; "
              f"{int(st1[1]['n_changed'][0])} effects changed in the second sweep")
        assert same and stats and st1[1]["n_changed"][0] > 0


# ---- 4. block sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_block_sizes_agree(precision):
    cs = _case()
    T, vs = 9, 0.01
    c = MR.case_traits(cs, T)
    runs = {}
    for bs in (1, 40, 100):
        hip = _engine(precision, T, bs)
        try:
            _upload(hip, c)
            _sweep(hip, c, 1, vs)
            runs[bs] = hip.mega_get_state()
        finally:
            hip.close()
    ref = _reference(1, 40, vs, T)
    err = MR.propagated_bound(cs.X, c.R, c.alpha, ref, iteration=1, seed=SEED, vare=c.vare, var_effect=c.v * vs)
    print(f"tight prior: largest propagated bound {err.max():.2e}, largest |beta| {np.abs(ref.beta).max():.2e}")
    assert err.max() < 1e-3 * np.abs(ref.beta).max()                    # (the bound means something)
    for bs in (1, 40, 100):
        a, b, d = runs[bs]
        assert np.array_equal(d, ref.delta)
        w = float((np.abs(b - ref.beta) / err).max())
        print(f"Float{precision} blocks of {bs}: beta worst error / bound against the restatement {w:.3e}")
        assert w <= 1.0
    for bs in (1, 100):
        w = float((np.abs(runs[bs][1] - runs[40][1]) / (2 * err)).max())
        wa = float((np.abs(runs[bs][0] - runs[40][0]) / (2 * err)).max())
        print(f"Float{precision} blocks of {bs} against 40: beta {w:.3e}, alpha {wa:.3e} of the bound")
        assert w <= 1.0 and wa <= 1.0


# ---- 5. the same seed gives the same bits ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal_iterations_and_traits_differ():
    cs = _case()
    c = MR.case_traits(cs, 9)
    for q in ("R", "alpha", "beta", "delta", "vare", "v", "pi"):         # traits 1 and 4 (both pi = 0.5) get equal inputs
        c[q][4] = c[q][1]
    outs = []
    for _ in range(2):
        hip = _engine(32, 9)
        try:
            _upload(hip, c)
            stats = [_sweep(hip, c, it) for it in range(1, 6)]
            outs.append((hip.mega_get_state(), hip.mega_get_residual(), stats))
        finally:
            hip.close()
    (s0, r0, t0), (s1, r1, t1) = outs
    assert all(np.array_equal(x, y) for x, y in zip(s0, s1)) and np.array_equal(r0, r1)
    for x, y in zip(t0, t1):
        assert all(np.array_equal(x[k], y[k]) for k in STAT_KEYS)
    hip = _engine(32, 9)
    try:
        got = []
        for it in (1, 2):
            _upload(hip, c)
            _sweep(hip, c, it)
            got.append(hip.mega_get_state())
        assert not np.array_equal(got[0][1], got[1][1]) and not np.array_equal(got[0][2], got[1][2])      # iterations differ
        assert not np.array_equal(got[0][1][1], got[0][1][4]) and not np.array_equal(got[0][2][1], got[0][2][4])      # traits differ
    finally:
        hip.close()


# ---- 6. missing cells ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_imputation(precision):
    cs = _case()
    T = 64
    c = MR.case_traits(cs, T)
    hip = _engine(precision, T)
    try:
        _upload(hip, c)
        hip.mega_impute(iteration=3, seed=SEED, vare=c.vare)              # before a pattern is set: nothing is redrawn
        assert np.array_equal(hip.mega_get_residual(), c.R)
        hip.mega_set_missing(c.missing)
        hip.mega_impute(iteration=3, seed=SEED, vare=c.vare)
        R = hip.mega_get_residual()
        assert np.array_equal(R[~c.missing], c.R[~c.missing]) and not np.any(R[c.missing] == c.R[c.missing])
        sd = np.sqrt(np.broadcast_to(c.vare[:, None], R.shape))
        z = (R / sd)[c.missing]
        m = z.size
        zm, zv = abs(z.mean()) * np.sqrt(m), abs(z.var(ddof=1) - 1.0) / np.sqrt(2.0 / (m - 1))
        Rr = c.R.copy()
        MR.impute(Rr, c.missing, iteration=3, seed=SEED, vare=c.vare)
        wr = float((np.abs(R - Rr)[c.missing] / ((2.0 ** -46 + 4 * U * np.abs(Rr / sd)) * sd)[c.missing]).max())
        print(f"Float{precision}: {m} missing cells, mean {zm:.2f} se, variance {zv:.2f} se; against the restatement {wr:.3e} of the Box-Muller bound")
        assert zm <= 5.0 and zv <= 5.0 and wr <= 1.0
        other = hip.mega_get_residual()
        hip.mega_impute(iteration=4, seed=SEED, vare=c.vare)
        assert not np.any(hip.mega_get_residual()[c.missing] == other[c.missing])
        # the sentinel beyond n: the sweep's sums run over the pad rows, which no imputation may have written
        R0 = hip.mega_get_residual()
        hip.mega_set_state(c.alpha * 0, c.beta, c.delta)
        st = hip.mega_sweep(iteration=1, seed=SEED, vare=c.vare, var_effect=c.v, pi=np.ones(T))      # pi = 1: no marker enters, r stays
        assert np.array_equal(hip.mega_get_residual(), R0) and np.all(st["sum_delta"] == 0)
        w = float((np.abs(st["resid_ss"] - (R0 * R0).sum(axis=1)) / (2 * (LD + 2) * U * (R0 * R0).sum(axis=1))).max())
        print(f"    sum r^2 over the padded rows against the visible rows: {w:.3f} of the bound")
        assert w <= 1.0
        hip.mega_set_missing(None)
        hip.mega_impute(iteration=5, seed=SEED, vare=c.vare)
        assert np.array_equal(hip.mega_get_residual(), R0)
    finally:
        hip.close()


# ---- 7. the draws follow the closed-form posterior -------------------------------------------------------------------------------------------
def test_one_marker_draws_follow_the_closed_form_posterior_on_the_device():
    import jwas_jl_amd as J
    case = MR.conditional_case()
    prob, _, _ = MR.conditional_posterior(case)
    hip = J.HipEngine(0, precision=64)
    try:
        rows = MR.conditional_check(MR.conditional_engine(hip, case), case)
        for k, zf, zm1, zv1, zm0, zv0 in rows:
            print(f"device, trait {k}: frequency {zf:.2f} se from P = {prob[k]:.4f}; beta | 1: mean {zm1:.2f}, variance {zv1:.2f}; "
                  f"beta | 0: mean {zm0:.2f}, variance {zv0:.2f}")
        assert len(rows) == 3 and max(max(r[1:]) for r in rows) <= 5.0
    finally:
        hip.close()


# ---- 8. the error contract ---------------------------------------------------------------------------------------------------------------------
def test_error_contract():
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    cs = _case()
    T = 5
    c = MR.case_traits(cs, T)
    X32 = np.asfortranarray(cs.X.astype(np.float32))

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    sweep_kw = dict(iteration=1, seed=1, vare=c.vare, var_effect=c.v, pi=c.pi)
    hip = J.HipEngine(0)
    try:
        def without_session():
            hip._mega = (T, BS)
            return [code(hip.mega_set_missing, c.missing), code(hip.mega_set_residual, c.R), code(hip.mega_get_residual), code(hip.mega_set_state, c.alpha),
                    code(hip.mega_get_state), code(hip.mega_impute, iteration=1, seed=1, vare=c.vare), code(hip.mega_sweep, **sweep_kw),
                    code(hip.mega_accumulate, 1), code(hip.mega_posterior, 0), code(hip.mega_mul_alpha, 0), code(hip.mega_gram, 0), code(hip.mega_end)]
        hip.n, hip.p = N, P
        assert code(hip.mega_begin, T, BS) == ESTATE                          # no genotypes
        assert without_session() == [ESTATE] * 12
        hip.alloc_packed(N, P)
        assert code(hip.mega_begin, T, BS) == EUNSUP                          # a packed context
        hip.load_dense(X32)
        hip.set_weights(np.linspace(0.5, 2.0, N).astype(np.float32))
        assert code(hip.mega_begin, T, BS) == EUNSUP                          # residual weights
        hip.set_weights(None)
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mega_begin, T, BS) == EUNSUP                          # shards
        hip.comm_destroy()
        for bad in (0, 65, -1):
            assert code(hip.mega_begin, bad, BS) == EINVAL                    # T out of range
        assert code(hip.mega_begin, T, 257) == EINVAL and code(hip.mega_begin, T, -1) == EINVAL
        assert code(hip.mega_begin, T, BS, -1) == EINVAL and code(hip.mega_begin, T, BS, (1 << 24) - 4) == EINVAL
        assert without_session() == [ESTATE] * 12                            # none of the failed calls opened a session
        hip.mega_begin(T, BS)
        _upload(hip, c)
        before = (hip.mega_get_state(), hip.mega_get_residual())
        for key, bads in (("iteration", (0,)), ("vare", (0.0, -1.0, np.nan, np.inf)), ("var_effect", (0.0, -1.0, np.nan, np.inf)), ("pi", (-0.1, 1.5, np.nan))):
            for bad in bads:
                kw = dict(sweep_kw)
                if key == "iteration":
                    kw[key] = bad
                else:
                    kw[key] = kw[key].copy()
                    kw[key][T - 1] = bad
                assert code(hip.mega_sweep, **kw) == EINVAL, (key, bad)
        vbad = c.vare.copy(); vbad[2] = 0.0
        assert code(hip.mega_impute, iteration=1, seed=1, vare=vbad) == EINVAL and code(hip.mega_impute, iteration=0, seed=1, vare=c.vare) == EINVAL
        assert code(hip.mega_accumulate, 0.5) == EINVAL and code(hip.mega_posterior, T) == EINVAL and code(hip.mega_mul_alpha, -1) == EINVAL
        assert code(hip.mega_get_residual, T) == EINVAL and code(hip.mega_get_state, -1) == EINVAL and code(hip.mega_gram, 3) == EINVAL
        assert code(hip.mega_mul_alpha, 0, True) == ESTATE                    # no output rows loaded
        Rnan = c.R.copy(); Rnan[1, 5] = np.nan
        anan = c.alpha.copy(); anan[0, 3] = np.inf
        assert code(hip.mega_set_residual, Rnan) == EINVAL and code(hip.mega_set_state, anan) == EINVAL
        assert code(hip.mega_set_state, None, None, c.delta * 0.5 + 0.25) == EINVAL
        buf = np.empty(7, dtype=np.uint8)
        assert code(lambda: hip._chk(hip._L.jwas_hip_mega_set_missing(hip._h, 7, buf.ctypes.data))) == EINVAL
        g = np.empty(7)
        assert code(lambda: hip._chk(hip._L.jwas_hip_mega_get_gram(hip._h, 0, 7, g.ctypes.data, None))) == EINVAL
        after = (hip.mega_get_state(), hip.mega_get_residual())
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])      # nothing was launched
        for post in hip.mega_posterior(0):
            assert np.all(post == 0.0)
        hip.mega_begin(T, 0)                                                  # _begin on an open session replaces it; 0: blocks of 64
        assert hip.mega_gram(1)[0].shape == (36, 36) and np.all(hip.mega_get_residual() == 0.0) and np.all(hip.mega_get_state()[2] == 1.0)
        assert J.HipEngine.mega_estimate_bytes(N, P, T, 64) == MegaStandInEngine.mega_estimate_bytes(N, P, T, 64) > 8 * P * 64
        # EBVs: the training rows, and the rows of a second resident matrix
        _upload(hip, c)
        np.testing.assert_allclose(hip.mega_mul_alpha(2), cs.X @ c.alpha[2], rtol=0, atol=1e-12)
        hip.load_output_dense(np.asfortranarray(X32[5:700:7][:20]))
        np.testing.assert_allclose(hip.mega_mul_alpha(2, True), cs.X[5:700:7][:20] @ c.alpha[2], rtol=0, atol=1e-12)
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mega_sweep, **sweep_kw) == EUNSUP
        hip.comm_destroy()
        hip.mega_sweep(**sweep_kw)
        hip.load_dense(X32)                                                   # loading genotypes frees the session
        assert without_session() == [ESTATE] * 12
        hip.mega_begin(T, BS)
        hip.mega_end()
        assert without_session() == [ESTATE] * 12
    finally:
        hip.close()
    hip = J.HipEngine(0, precision=64)                                        # a Float64 context: weights refused, then accepted again as ones
    try:
        hip.load_dense(np.asfortranarray(cs.X))
        hip.set_weights(np.linspace(0.5, 2.0, N))
        assert code(hip.mega_begin, T, BS) == EUNSUP
        hip.set_weights(None)
        hip.mega_begin(T, BS)
    finally:
        hip.close()


# ---- 9. runMCMC ------------------------------------------------------------------------------------------------------------------------------
def test_runmcmc_gpu_vs_standin(tmp_path):
    """6 traits with missing cells, 12 iterations: the device against the stand-in engine through the whole driver.  The host draws
    (location parameters, pi, variances) come from one numpy generator on both sides and read the engines' statistics, which differ
    by rounding (~1e-16 relative per sum); no indicator may flip (Model_Frequency equal), and the continuous outputs are compared
    at the FIRST saved iteration within 1e-10 relative (a few hundred roundings of that size), and over the chain within 1e-8."""
    from test_megatrait_host import check_outputs, mega_data, run_mega
    data = mega_data(n=120, p=150, seed=9)
    outs = {}
    for name, engine in (("ref", MegaStandInEngine(64)), ("hip", None)):
        outs[name] = run_mega(tmp_path, name, data=data, engine=engine, chain_length=12, burnin=2, seed=13, block_size=40)
    traits = [f"y{k + 1}" for k in range(6)]
    p = len(outs["hip"]["marker effects geno"]) // 6

    def diff(key, col):
        return float(np.abs(outs["hip"][key][col].to_numpy(dtype=np.float64) - outs["ref"][key][col].to_numpy(dtype=np.float64)).max())
    np.testing.assert_array_equal(outs["hip"]["marker effects geno"]["Model_Frequency"].to_numpy(), outs["ref"]["marker effects geno"]["Model_Frequency"].to_numpy())
    first, chain = 0.0, 0.0
    for f in ["residual_variance", "marker_effects_variances_geno", "pi_geno", "heritability"] + [f"marker_effects_geno_{tr}" for tr in traits]:
        a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{f}.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
        assert a.shape == b.shape and a.shape[0] == 10
        assert np.array_equal(a == 0.0, b == 0.0), f
        first = max(first, float((np.abs(a[0] - b[0]) / (np.abs(a[0]).max())).max()))
        chain = max(chain, float((np.abs(a - b) / np.abs(a).max()).max()))
    d_eff, d_ebv = diff("marker effects geno", "Estimate"), max(diff(f"EBV_{tr}", "EBV") for tr in traits)
    print(f"runMCMC, 6 traits: first saved iteration {first:.3e} relative, whole chain {chain:.3e}; effect means {d_eff:.3e}, EBVs {d_ebv:.3e}")
    assert first <= 1e-10 and chain <= 1e-8 and d_eff <= 1e-9 and d_ebv <= 1e-8
    assert outs["hip"]["pi_geno"]["SD"].max() > 0 and np.any(outs["hip"]["marker effects geno"]["Estimate"] != 0.0)
    check_outputs(outs["hip"], str(tmp_path / "hip"), 120, p, traits, 10)
    # Float32 storage: it runs, every file is present, every value finite
    with contextlib.redirect_stdout(io.StringIO()):
        f32 = run_mega(tmp_path, "f32", data=data, engine=None, double=False, chain_length=12, burnin=2, seed=13, block_size=40)
    check_outputs(f32, str(tmp_path / "f32"), 120, p, traits, 10)
    assert os.path.exists(tmp_path / "f32" / "EBV_y6.txt")
