"""Unconstrained multi-trait BayesC with 5 to 8 traits on the device (csrc/mtjoint.hpp) through the C ABI and runMCMC, against the numpy
restatement of tests/mtj_reference.py on the same Philox counters.

Shapes: n = 301 individuals (ld 512: two 256-row slices, the second ragged), p = 100 markers in blocks of 40 (three blocks, the last
ragged), t in {5, 8} traits (8 fills the trait tile of k_mega_update_partial and the 256-entry Pi table), Float32 and Float64
genotypes.  The device and the restatement evaluate the chain of a marker in the same IEEE operations and differ in the ORDER of the
O(n) sums behind x'r and x'x and in the libm behind log, exp and Box-Muller.  With u = 2^-53:

    indicators     discrete: EQUAL to the restatement's own chain for all t p decisions (mtj_reference asserts that no decision uniform
                   of that chain lies within 1e-9 of probDelta1; tests/test_mtj_host.py runs that check on the CPU)
    beta, alpha    every marker against the restatement evaluated from the DEVICE's own history and under its indicators
                   (mtj_reference.conditional_recheck): 2 (N + 2) u abs_s carried through the t-step conditional, plus Box-Muller
    statistics     the state counts and the changed count exact; sum beta beta', sum alpha^2, the residual cross-products and sums
                   against numpy sums of the device's own state: 2 (m + 2) u sum |terms| for m terms; sum beta beta' symmetric bit for bit
    residual       against the apply recomputed in numpy from the device's own change lists: within 4 u of the sum of the absolute terms
    block sizes    under a tight prior (G / 100) mtj_reference.propagated_bound is meaningful, and two block sizes differ by at most
                   the sum of their bounds
Every test prints the figures it measured before it asserts."""
import contextlib
import functools
import io

import numpy as np
import pytest

import mtj_reference as MJ
from mtj_reference import MtjStandInEngine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4
N, P, LD = 301, 100, 512
BS, BLOCK_SIZES, TIGHT, SEED = MJ.GPU_BLOCK, MJ.GPU_BLOCK_SIZES, MJ.GPU_TIGHT, MJ.CASE_SEED
CASES = [(t, prec) for t in (5, 8) for prec in (32, 64)]


@functools.lru_cache(maxsize=None)
def _case():
    return MJ.make_case(N, P)


@functools.lru_cache(maxsize=None)
def _traits(t, gscale=1.0):
    return MJ.case_traits(_case(), t, gscale=gscale)


@functools.lru_cache(maxsize=None)
def _reference(t, iteration, bs=BS, gscale=1.0):
    """The restatement's own sweep from the common state (computed once, shared, never changed); the 1e-9 margin is asserted inside."""
    return MJ.reference_sweep(_traits(t, gscale), iteration, SEED, bs)


def _engine(precision, t, bs=BS, X=None):
    import jwas_jl_amd as J
    hip = J.HipEngine(0, precision=precision)
    hip.load_dense(np.asfortranarray((_case().X if X is None else X).astype(hip.dtype)))
    hip.mtj_begin(t, bs)
    return hip


def _upload(hip, c):
    hip.mtj_set_residual(c.R)
    hip.mtj_set_state(c.alpha, c.beta, c.delta)


def _sweep(hip, c, iteration):
    return hip.mtj_sweep(iteration=iteration, seed=SEED, rinv=c.Rinv, ginv=c.Ginv, log_pi=c.log_pi)


def _states(delta):
    return np.array([MJ.state_of(delta[:, j]) for j in range(delta.shape[1])])


def _check_statistics(st, c, alpha, beta, delta, R, label):
    t = c.t
    assert np.array_equal(st["state_counts"], np.bincount(_states(delta), minlength=1 << t).astype(np.float64))
    assert st["n_changed"] == float((alpha != c.alpha).any(axis=0).sum())
    assert np.array_equal(st["beta_ss"], st["beta_ss"].T) and np.array_equal(st["resid_cp"], st["resid_cp"].T)      # bit-symmetric
    w1 = float((np.abs(st["beta_ss"] - beta @ beta.T) / (2 * (P + 2) * U * (np.abs(beta) @ np.abs(beta).T))).max())
    w2 = float((np.abs(st["alpha_ss"] - (alpha * alpha).sum(axis=1)) / (2 * (P + 2) * U * (alpha * alpha).sum(axis=1) + 1e-300)).max())
    w3 = float((np.abs(st["resid_cp"] - R @ R.T) / (2 * (LD + 2) * U * (np.abs(R) @ np.abs(R).T))).max())
    w4 = float((np.abs(st["resid_sum"] - R.sum(axis=1)) / (2 * (LD + 2) * U * np.abs(R).sum(axis=1))).max())
    print(f"    {label} statistics worst error / bound: beta beta' {w1:.3f}, alpha'alpha {w2:.3f}, r r' {w3:.3f}, sum r {w4:.3f}")
    assert max(w1, w2, w3, w4) <= 1.0


def _check_residual(c, alpha, R, X=None):
    X = _case().X if X is None else X
    Rn, d = c.R.copy(), c.alpha - alpha
    MJ.apply_changes(Rn, X, d)
    terms = np.abs(c.R) + np.abs(d) @ np.abs(X).T
    wr = float((np.abs(R - Rn) / (4 * U * terms)).max())
    print(f"    residual worst error / bound {wr:.3f} ({'bit-equal' if np.array_equal(R, Rn) else 'not bit-equal'})")
    assert wr <= 1.0


# ---- 1. one sweep from a common uploaded state, iterations 1 and 2 ---------------------------------------------------------------------
@pytest.mark.parametrize("t,precision", CASES)
def test_sweep_indicators_effects_statistics_residual(t, precision):
    cs, c = _case(), _traits(t)
    hip = _engine(precision, t)
    try:
        G, xpx = hip.mtj_gram(2)
        assert G.shape == (20, 20) and np.array_equal(G, G.T) and np.array_equal(np.diag(G), xpx)
        for iteration in (1, 2):
            ref = _reference(t, iteration)
            _upload(hip, c)
            st = _sweep(hip, c, iteration)
            alpha, beta, delta = hip.mtj_get_state()
            R = hip.mtj_get_residual()
            nmis = int((delta != ref.delta).sum())
            print(f"t = {t} Float{precision} iteration {iteration}: {nmis} of {t * P} indicators differ; nearest threshold {ref.margins.min():.2e}; "
                  f"{int(st['n_changed'])} markers changed; {int((st['state_counts'] > 0).sum())} joint states occupied")
            assert nmis == 0
            assert np.array_equal(alpha, delta * beta) and set(np.unique(delta)) <= {0.0, 1.0}
            assert np.array_equal(st["state_counts"], ref.state_counts) and st["n_changed"] == ref.n_changed
            b_ref, bound = MJ.conditional_recheck(cs.X, c.R, c.alpha, c.beta, c.delta, alpha, delta, iteration=iteration, seed=SEED, Rinv=c.Rinv,
                                                  Ginv=c.Ginv, log_pi=c.log_pi)
            wb = float((np.abs(beta - b_ref) / bound).max())
            wa = float((np.abs(alpha - delta * b_ref) / bound).max())
            print(f"    beta worst error / bound {wb:.3e}, alpha {wa:.3e} (largest bound {bound.max():.2e}, largest |beta| {np.abs(beta).max():.2e}); "
                  f"against the restatement's own chain: {np.abs(beta - ref.beta).max():.2e}")
            assert wb <= 1.0 and wa <= 1.0 and np.all(np.isfinite(beta))
            _check_statistics(st, c, alpha, beta, delta, R, "")
            _check_residual(c, alpha, R)
    finally:
        hip.close()


# ---- 2. block sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,precision", CASES)
def test_block_sizes_agree(t, precision):
    """1: one marker per block; 40: three blocks; 100: one block of two 64-lane sub-blocks, the second partial; 256: more than p."""
    cs, c = _case(), _traits(t, TIGHT)
    runs = {}
    for bs in BLOCK_SIZES:
        hip = _engine(precision, t, bs)
        try:
            _upload(hip, c)
            _sweep(hip, c, 1)
            runs[bs] = hip.mtj_get_state()
        finally:
            hip.close()
    ref = _reference(t, 1, BS, TIGHT)
    err = MJ.propagated_bound(cs.X, c.R, c.alpha, c.beta, c.delta, ref, iteration=1, seed=SEED, Rinv=c.Rinv, Ginv=c.Ginv, log_pi=c.log_pi)
    print(f"tight prior: largest propagated bound {err.max():.2e}, largest |beta| {np.abs(ref.beta).max():.2e}")
    assert err.max() < 1e-3 * np.abs(ref.beta).max()                    # (the bound means something)
    for bs in BLOCK_SIZES:
        a, b, d = runs[bs]
        assert np.array_equal(d, ref.delta)
        w = float((np.abs(b - ref.beta) / err).max())
        print(f"t = {t} Float{precision} blocks of {bs}: beta worst error / bound against the restatement {w:.3e}")
        assert w <= 1.0
    for bs in (1, 100, 256):
        w = float((np.abs(runs[bs][1] - runs[BS][1]) / (2 * err)).max())
        wa = float((np.abs(runs[bs][0] - runs[BS][0]) / (2 * err)).max())
        print(f"t = {t} Float{precision} blocks of {bs} against {BS}: beta {w:.3e}, alpha {wa:.3e} of the bound")
        assert w <= 1.0 and wa <= 1.0


# ---- 3. the same seed gives the same bits ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal_and_iterations_differ():
    c = _traits(8)
    outs = []
    for _ in range(2):
        hip = _engine(32, 8)
        try:
            _upload(hip, c)
            stats = [_sweep(hip, c, it) for it in range(1, 5)]
            outs.append((hip.mtj_get_state(), hip.mtj_get_residual(), stats))
        finally:
            hip.close()
    (s0, r0, t0), (s1, r1, t1) = outs
    assert all(np.array_equal(x, y) for x, y in zip(s0, s1)) and np.array_equal(r0, r1)
    for x, y in zip(t0, t1):
        assert all(np.array_equal(x[k], y[k]) for k in ("state_counts", "beta_ss", "alpha_ss", "resid_cp", "resid_sum", "n_changed"))
    hip = _engine(32, 8)
    try:
        got = []
        for it in (1, 2):
            _upload(hip, c)
            _sweep(hip, c, it)
            got.append(hip.mtj_get_state())
        assert not np.array_equal(got[0][1], got[1][1]) and not np.array_equal(got[0][2], got[1][2])      # iterations differ
        assert not np.array_equal(got[0][1][1], got[0][1][4])                                             # traits differ
    finally:
        hip.close()


# ---- 4. a commit that changes a later lane's decision; every marker commits ------------------------------------------------------------------
@pytest.mark.parametrize("t,precision", CASES)
def test_duplicated_columns_and_rrblup(t, precision):
    cs = _case()
    c, (j1, j2) = MJ.duplicate_case(cs, t)
    ref = MJ.reference_sweep(c, 1, SEED, BS)
    spec = MJ.speculative_state(c, j2, 1, SEED)
    print(f"t = {t}: marker {j1} takes state {ref.states[j1]:0{t}b}; its duplicate {j2} would take {spec:0{t}b} from the block-entry residual, takes {ref.states[j2]:0{t}b}")
    assert ref.states[j1] != 0 and spec != ref.states[j2] and j1 // 64 == j2 // 64 and j1 // BS == j2 // BS
    hip = _engine(precision, t, X=c.X)
    try:
        _upload(hip, c)
        st = _sweep(hip, c, 1)
        alpha, beta, delta = hip.mtj_get_state()
        assert np.array_equal(delta, ref.delta) and _states(delta)[j2] == ref.states[j2] != spec
        b_ref, bound = MJ.conditional_recheck(c.X, c.R, c.alpha, c.beta, c.delta, alpha, delta, iteration=1, seed=SEED, Rinv=c.Rinv, Ginv=c.Ginv, log_pi=c.log_pi)
        wb = float((np.abs(beta - b_ref) / bound).max())
        print(f"    duplicated columns, Float{precision}: beta worst error / bound {wb:.3e}; {int(st['n_changed'])} markers changed")
        assert wb <= 1.0
        _check_statistics(st, c, alpha, beta, delta, hip.mtj_get_residual(), "duplicate")
        _check_residual(c, alpha, hip.mtj_get_residual(), c.X)
    finally:
        hip.close()
    c, _ = MJ.rrblup_case(cs, t)
    ref = MJ.reference_sweep(c, 1, SEED, 100)
    hip = _engine(precision, t, 100)
    try:
        _upload(hip, c)
        st = _sweep(hip, c, 1)
        alpha, beta, delta = hip.mtj_get_state()
        R = hip.mtj_get_residual()
        assert np.all(delta == 1.0) and st["state_counts"][-1] == P and st["n_changed"] == P and np.array_equal(alpha, beta)
        b_ref, bound = MJ.conditional_recheck(cs.X, c.R, c.alpha, c.beta, c.delta, alpha, delta, iteration=1, seed=SEED, Rinv=c.Rinv, Ginv=c.Ginv, log_pi=c.log_pi)
        wb = float((np.abs(beta - b_ref) / bound).max())
        print(f"    RR-BLUP (blocks of 100), Float{precision}: beta worst error / bound {wb:.3e}; against the restatement's chain {np.abs(beta - ref.beta).max():.2e}")
        assert wb <= 1.0 and np.all(np.isfinite(beta))
        _check_statistics(st, c, alpha, beta, delta, R, "RR-BLUP")
        _check_residual(c, alpha, R)
    finally:
        hip.close()


# ---- 5. states of probability 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,precision", CASES)
def test_zero_probability_states_are_never_entered(t, precision):
    c, zero = MJ.zero_state_case(_case(), t)
    hip = _engine(precision, t)
    try:
        _upload(hip, c)
        seen = 0
        for it in (1, 2, 3):
            st = _sweep(hip, c, it)
            alpha, beta, delta = hip.mtj_get_state()
            R = hip.mtj_get_residual()
            assert np.all(np.isfinite(alpha)) and np.all(np.isfinite(beta)) and np.all(np.isfinite(R))
            assert all(np.all(np.isfinite(st[k])) for k in ("state_counts", "beta_ss", "alpha_ss", "resid_cp", "resid_sum"))
            assert not np.isin(_states(delta), zero).any() and np.all(st["state_counts"][zero] == 0.0) and st["state_counts"].sum() == P
            seen += int(st["n_changed"])
        ref = MJ.reference_sweep(c, 1, SEED, BS)
        print(f"t = {t} Float{precision}: {len(zero)} of {1 << t} states have probability 0; none entered in three sweeps ({seen} marker changes)")
        assert seen > 0 and not np.isin(ref.states, zero).any()
    finally:
        hip.close()


# ---- 6. the draws follow the enumerated posterior -----------------------------------------------------------------------------------------------
def test_one_marker_draws_follow_the_enumerated_posterior_on_the_device():
    import jwas_jl_amd as J
    case = MJ.conditional_case()
    prob, _, _ = MJ.conditional_posterior(case)
    hip = J.HipEngine(0, precision=64)
    try:
        rows_trait, rows_state = MJ.conditional_check(MJ.conditional_engine(hip, case), case)
        for k, zf, zm, zv in rows_trait:
            print(f"device, trait {k}: inclusion frequency {zf:.2f} se; beta: mean {zm:.2f}, variance {zv:.2f}")
        for s, zf, zm, zv in rows_state:
            print(f"device, state {s:05b}: frequency {zf:.2f} se from P = {prob[s]:.4f}; beta | state: mean {zm:.2f}, variance {zv:.2f}")
        assert len(rows_trait) == 5 and max(max(r[1:]) for r in rows_trait) <= 5.0
        assert len(rows_state) >= 8 and max(max(r[1:]) for r in rows_state) <= 5.0
    finally:
        hip.close()


# ---- 7. the error contract ---------------------------------------------------------------------------------------------------------------------
def test_error_contract():
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    cs = _case()
    T = 5
    c = _traits(T)
    X32 = np.asfortranarray(cs.X.astype(np.float32))

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    sweep_kw = dict(iteration=1, seed=1, rinv=c.Rinv, ginv=c.Ginv, log_pi=c.log_pi)
    hip = J.HipEngine(0)
    try:
        def without_session():
            hip._mtj = (T, BS)
            return [code(hip.mtj_set_residual, c.R), code(hip.mtj_get_residual), code(hip.mtj_set_state, c.alpha), code(hip.mtj_get_state),
                    code(hip.mtj_gram, 0), code(hip.mtj_sweep, **sweep_kw), code(hip.mtj_accumulate, 1), code(hip.mtj_posterior, 0),
                    code(hip.mtj_mul_alpha, 0), code(hip.mtj_end)]
        hip.n, hip.p = N, P
        assert code(hip.mtj_begin, T, BS) == ESTATE                           # no genotypes
        assert without_session() == [ESTATE] * 10
        hip.alloc_packed(N, P)
        assert code(hip.mtj_begin, T, BS) == EUNSUP                           # a packed context
        hip.load_dense(X32)
        hip.set_weights(np.linspace(0.5, 2.0, N).astype(np.float32))
        assert code(hip.mtj_begin, T, BS) == EUNSUP                           # residual weights
        hip.set_weights(None)
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mtj_begin, T, BS) == EUNSUP                           # shards
        hip.comm_destroy()
        for bad in (0, 4, 9, 64, -1):
            assert code(hip.mtj_begin, bad, BS) == EINVAL                     # t outside 5..8
        assert code(hip.mtj_begin, T, 257) == EINVAL and code(hip.mtj_begin, T, -1) == EINVAL
        assert without_session() == [ESTATE] * 10                            # none of the failed calls opened a session
        hip.mtj_begin(T, BS)
        _upload(hip, c)
        before = (hip.mtj_get_state(), hip.mtj_get_residual())
        assert code(hip.mtj_sweep, **dict(sweep_kw, iteration=0)) == EINVAL
        for key in ("rinv", "ginv"):
            for bad in (np.nan, np.inf):
                M = sweep_kw[key].copy(); M[1, 2] = M[2, 1] = bad
                assert code(hip.mtj_sweep, **dict(sweep_kw, **{key: M})) == EINVAL, (key, bad)
            M = sweep_kw[key].copy(); M[0, 0] = -M[0, 0]                      # not positive definite
            assert code(hip.mtj_sweep, **dict(sweep_kw, **{key: M})) == EINVAL
            M = sweep_kw[key].copy(); M[0, 3] = M[3, 0] = 10 * M.max()        # symmetric, indefinite
            assert code(hip.mtj_sweep, **dict(sweep_kw, **{key: M})) == EINVAL
            M = sweep_kw[key].copy(); M[0, 3] = 2 * M[0, 3] + 1e-3 * M[0, 0]  # not symmetric
            assert code(hip.mtj_sweep, **dict(sweep_kw, **{key: M})) == EINVAL
        for lp in (c.log_pi[:16], np.concatenate([c.log_pi, c.log_pi]), np.full(32, -np.inf)):
            assert code(hip.mtj_sweep, **dict(sweep_kw, log_pi=lp)) == EINVAL   # a Pi table of the wrong length; no possible state
        for bad in (np.nan, 0.5):
            lp = c.log_pi.copy(); lp[7] = bad
            assert code(hip.mtj_sweep, **dict(sweep_kw, log_pi=lp)) == EINVAL
        assert code(hip.mtj_accumulate, 0.5) == EINVAL and code(hip.mtj_posterior, T) == EINVAL and code(hip.mtj_mul_alpha, -1) == EINVAL
        assert code(hip.mtj_gram, 3) == EINVAL
        assert code(lambda: hip._chk(hip._L.jwas_hip_mtj_get_residual(hip._h, T, np.empty(N).ctypes.data))) == EINVAL
        assert code(lambda: hip._chk(hip._L.jwas_hip_mtj_get_state(hip._h, -1, None, None, None))) == EINVAL
        assert code(hip.mtj_mul_alpha, 0, True) == ESTATE                     # no output rows loaded
        Rnan = c.R.copy(); Rnan[1, 5] = np.nan
        anan = c.alpha.copy(); anan[0, 3] = np.inf
        assert code(hip.mtj_set_residual, Rnan) == EINVAL and code(hip.mtj_set_state, anan) == EINVAL
        assert code(hip.mtj_set_state, None, None, c.delta * 0.5 + 0.25) == EINVAL
        g = np.empty(7)
        assert code(lambda: hip._chk(hip._L.jwas_hip_mtj_gram(hip._h, 0, 7, g.ctypes.data, None))) == EINVAL
        after = (hip.mtj_get_state(), hip.mtj_get_residual())
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])      # nothing was launched
        for post in hip.mtj_posterior(0):
            assert np.all(post == 0.0)
        hip.mtj_begin(T, 0)                                                   # _begin on an open session replaces it; 0: blocks of 64
        assert hip.mtj_gram(1)[0].shape == (36, 36) and np.all(hip.mtj_get_residual() == 0.0) and np.all(hip.mtj_get_state()[2] == 1.0)
        # accumulate, posterior and the EBVs: the training rows, and the rows of a second resident matrix
        _upload(hip, c)
        hip.mtj_accumulate(1)
        m, m2, f = hip.mtj_posterior(2)
        assert np.array_equal(m, c.alpha[2]) and np.array_equal(m2, c.alpha[2] ** 2) and np.array_equal(f, c.delta[2])
        np.testing.assert_allclose(hip.mtj_mul_alpha(2), cs.X @ c.alpha[2], rtol=0, atol=1e-12)
        hip.load_output_dense(np.asfortranarray(X32[5:700:7][:20]))
        np.testing.assert_allclose(hip.mtj_mul_alpha(2, True), cs.X[5:700:7][:20] @ c.alpha[2], rtol=0, atol=1e-12)
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mtj_sweep, **sweep_kw) == EUNSUP
        hip.comm_destroy()
        hip.mtj_sweep(**sweep_kw)
        hip.load_dense(X32)                                                   # loading genotypes frees the session
        assert without_session() == [ESTATE] * 10
        hip.mtj_begin(T, BS)
        hip.mtj_end()
        assert without_session() == [ESTATE] * 10
    finally:
        hip.close()


# ---- 8. runMCMC ------------------------------------------------------------------------------------------------------------------------------
def test_runmcmc_gpu_vs_standin(tmp_path):
    """5 traits, 30 iterations with every variance and Pi estimated: the device against the stand-in engine through the whole driver.  The
    host draws (location parameters, Pi, the two inverse-Wishart draws) come from one numpy generator on both sides and read the engines'
    statistics, which differ by rounding; no indicator may flip (Model_Frequency equal), and the continuous outputs are compared with
    the tolerances of test_gpu_megatrait.py::test_runmcmc_gpu_vs_standin: the FIRST saved iteration within 1e-10 relative, the chain
    within 1e-8, the effect means within 1e-9 and the EBVs within 1e-8."""
    from test_megatrait_host import mega_data
    from test_mtj_host import check_outputs, run_joint
    data = mega_data(n=120, p=150, t=5, seed=9, missing=0.0)
    outs = {}
    for name, engine in (("ref", MtjStandInEngine(64)), ("hip", None)):
        outs[name] = run_joint(tmp_path, name, data=data, engine=engine, chain_length=30, burnin=5, seed=13, block_size=40)
    traits = [f"y{k + 1}" for k in range(5)]
    p = len(outs["hip"]["marker effects geno"]) // 5

    def diff(key, col):
        return float(np.abs(outs["hip"][key][col].to_numpy(dtype=np.float64) - outs["ref"][key][col].to_numpy(dtype=np.float64)).max())
    np.testing.assert_array_equal(outs["hip"]["marker effects geno"]["Model_Frequency"].to_numpy(), outs["ref"]["marker effects geno"]["Model_Frequency"].to_numpy())
    first, chain = 0.0, 0.0
    for f in ["residual_variance", "marker_effects_variances_geno", "pi_geno", "heritability", "genetic_variance"] + [f"marker_effects_geno_{tr}" for tr in traits]:
        a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{f}.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
        assert a.shape == b.shape and a.shape[0] == 25
        assert np.array_equal(a == 0.0, b == 0.0), f
        first = max(first, float((np.abs(a[0] - b[0]) / (np.abs(a[0]).max())).max()))
        chain = max(chain, float((np.abs(a - b) / np.abs(a).max()).max()))
    d_eff, d_ebv = diff("marker effects geno", "Estimate"), max(diff(f"EBV_{tr}", "EBV") for tr in traits)
    print(f"runMCMC, 5 traits: first saved iteration {first:.3e} relative, whole chain {chain:.3e}; effect means {d_eff:.3e}, EBVs {d_ebv:.3e}")
    assert first <= 1e-10 and chain <= 1e-8 and d_eff <= 1e-9 and d_ebv <= 1e-8
    assert outs["hip"]["pi_geno"]["SD"].max() > 0 and np.any(outs["hip"]["marker effects geno"]["Estimate"] != 0.0)
    check_outputs(outs["hip"], str(tmp_path / "hip"), 120, p, traits, 25)
    # Float32 storage: it runs, every file is present, every value finite
    with contextlib.redirect_stdout(io.StringIO()):
        f32 = run_joint(tmp_path, "f32", data=data, engine=None, double=False, chain_length=30, burnin=5, seed=13, block_size=40)
    check_outputs(f32, str(tmp_path / "f32"), 120, p, traits, 25)
