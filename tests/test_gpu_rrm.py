"""Random regression models on the device (csrc/rrm.hpp) through the C ABI and runMCMC, against the numpy restatement of
tests/rrm_reference.py on the same Philox counters.

Shapes: n = 301 individuals (two 256-row slices, the second ragged), p = 100 markers in blocks of 40 (three blocks, the last
ragged).  The device and the restatement evaluate the same formulas in double and differ in the ORDER of the O(n) sums and in the
libm behind Box-Muller.  With u = 2^-53 and |.| taken entry by entry:

    M_j, G_jk      two summation orders of the same n products: 2 (n + 2) u sum_i |x_ij x_ik| sum_t m_it |phi_ta phi_tb|
    states         discrete: EQUAL to the restatement's own chain for every marker (rrm_reference asserts that no uniform of that chain
                   lies within 1e-9 of a boundary of its state CDF)
    beta, alpha    an earlier marker's rounding reaches every later marker through the chain, and a worst-case bound on that grows
                   geometrically with the number of markers; so every marker is compared with the restatement evaluated from the
                   DEVICE's own history (rrm_reference.conditional_recheck: s_k = x_k'v(W0) + sum_{j<k} G_kj d_j with d_j the device's
                   own changes) -- then both sides start from the same doubles, and the bound is 2 (N + 2) u abs_s_k carried through
                   the c x c solve, plus the Box-Muller term of tests/test_gpu_sem.py (rrm_reference.marker_bound)
    statistics     against numpy sums of the device's own beta, alpha and residual: 2 (K + 2) u sum |terms| for K terms; the counts exact
    block sizes    under a tight prior (G / 100: a later marker is moved by an earlier one's difference by less than that difference)
                   the propagated bound of rrm_reference.sweep_blocked(bounds=True) is meaningful, and two block sizes differ by at
                   most the sum of their bounds

THE RESIDUAL is checked against the apply recomputed in numpy from the device's own change list (the same IEEE operations in the same
order): within 4 u of the sum of the absolute terms, and exactly 0 at every cell without a record.  Pad rows are not visible through
the C ABI; the sweep's sum W^2 runs over them, so a pad row that moved would fail the statistics.  Every test prints the figures
it measured before it asserts."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

import rrm_reference as RR
from rrm_reference import RrmStandInEngine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4
N, P, BS, SEED = 301, 100, 40, 5
# (T, c, fraction of missing records, individuals with a single record)
SHAPES = {1: (5, 3, 0.2, 0), 2: (2, 2, 0.0, 0), 3: (7, 4, 0.3, 40), 4: (64, 2, 0.2, 0)}
CASES = [(cid, prec) for cid in SHAPES for prec in (32, 64)]


@functools.lru_cache(maxsize=None)
def _case(cid):
    T, c, miss, single = SHAPES[cid]
    cs = RR.make_case(N, P, T, c, miss, 7 + cid, single)
    if cid == 2:
        assert cs.obs.all()
    if cid == 3:
        assert (cs.obs.sum(axis=0) == 1).sum() >= 40
    if cid == 4:
        assert cs.obs[63].any()
    return cs


def _engine(cs, precision, bs=BS):
    import jwas_jl_amd as J
    hip = J.HipEngine(0, precision=precision)
    hip.load_dense(np.asfortranarray(cs.X.astype(hip.dtype)))
    hip.rrm_begin(cs.Phi, cs.obs, bs)
    return hip


def _upload(hip, cs):
    hip.rrm_set_residual(cs.W)
    hip.rrm_set_state(cs.alpha, cs.beta, cs.delta)


def _states(delta):
    return sum(delta[q].astype(np.int64) << q for q in range(delta.shape[0]))


@functools.lru_cache(maxsize=None)
def _reference(cid, iteration, bs=BS, gscale=1.0, bounds=False):
    """The restatement's own sweep from the common state (computed once, shared, never changed)."""
    cs = _case(cid)
    O = RR.occupancy(cs.Phi, cs.obs)
    M = RR.m_array(cs.X, O)
    grams = [RR.gram_block(cs.X, O, j0, min(bs, P - j0)) for j0 in range(0, P, bs)]
    W, a, b, d = cs.W.copy(), cs.alpha.copy(), cs.beta.copy(), cs.delta.copy()
    r = RR.sweep_blocked(cs.X, cs.Phi, cs.obs, M, grams, W, a, b, d, block_size=bs, iteration=iteration, seed=SEED, vare=cs.vare, G=cs.G * gscale,
                         log_pi=cs.log_pi, min_margin=1e-9, bounds=bounds)
    r.update(W=W, alpha=a, beta=b, delta=d)
    return r


# ---- 1. M_j and the Gram tensor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,precision", CASES)
def test_m_and_gram(cid, precision):
    cs = _case(cid)
    O, Oabs, Xa = RR.occupancy(cs.Phi, cs.obs), RR.occupancy(np.abs(cs.Phi), cs.obs), np.abs(cs.X)
    hip = _engine(cs, precision)
    try:
        M = hip.rrm_m()
        worst = float((np.abs(M - RR.m_array(cs.X, O)) / (2 * (N + 2) * U * RR.m_array(Xa, Oabs))).max())
        for k, j0 in enumerate(range(0, P, BS)):
            b = min(BS, P - j0)
            G = hip.rrm_gram(k)
            assert G.shape == (b, b, cs.c, cs.c)
            assert np.array_equal(G, G.transpose(1, 0, 2, 3)) and np.array_equal(G, G.transpose(0, 1, 3, 2))
            assert np.array_equal(G[np.arange(b), np.arange(b)], M[j0:j0 + b])              # G_jj = M_j, the same sum
            worst = max(worst, float((np.abs(G - RR.gram_block(cs.X, O, j0, b)) / (2 * (N + 2) * U * RR.gram_block(Xa, Oabs, j0, b))).max()))
        print(f"case {cid} Float{precision}: M and Gram worst error / bound {worst:.3f}")
        assert worst <= 1.0
    finally:
        hip.close()


def test_gram_beyond_one_grid_trip():
    """The Gram kernel's grid holds 32 768 blocks; with blocks of one marker p = 32 808 takes a second trip.  A small matrix tiled
    column-wise: the Gram of a one-marker block is M_j."""
    import jwas_jl_amd as J
    rng = np.random.default_rng(11)
    base = (rng.binomial(2, 0.4, size=(9, 8)) - 1.0)
    p = 32768 + 40
    X = np.asfortranarray(np.tile(base, (1, p // 8 + 1))[:, :p].astype(np.float32))
    Phi = RR.legendre_phi(np.arange(2), 2)
    obs = rng.random((2, 9)) >= 0.3
    obs[0, ~obs.any(axis=0)] = True
    O, Oabs = RR.occupancy(Phi, obs), RR.occupancy(np.abs(Phi), obs)
    hip = J.HipEngine(0)
    try:
        hip.load_dense(X)
        hip.rrm_begin(Phi, obs, 1)
        M = hip.rrm_m()
        ref, refa = RR.m_array(base, O), RR.m_array(np.abs(base), Oabs)
        worst = 0.0
        for j in (0, 32767, 32768, 32769, p - 1):
            G = hip.rrm_gram(j)
            assert G.shape == (1, 1, 2, 2) and np.array_equal(G[0, 0], M[j])
            worst = max(worst, float((np.abs(G[0, 0] - ref[j % 8]) / (2 * (9 + 2) * U * refa[j % 8] + 1e-300)).max()))
        print(f"second grid trip: worst error / bound {worst:.3f}")
        assert worst <= 1.0 and np.abs(M).max() > 0
    finally:
        hip.close()


# ---- 2. and 3. one sweep from a common uploaded state ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,precision", CASES)
def test_sweep_states_effects_statistics_residual(cid, precision):
    cs = _case(cid)
    T, c = cs.T, cs.c
    hip = _engine(cs, precision)
    try:
        for iteration in (1, 2):
            ref = _reference(cid, iteration)
            _upload(hip, cs)
            st = hip.rrm_sweep(iteration=iteration, seed=SEED, vare=cs.vare, G=cs.G, log_pi=cs.log_pi)
            alpha, beta, delta = hip.rrm_get_state()
            W = hip.rrm_get_residual()
            states = _states(delta)
            nmis = int((states != ref.states).sum())
            print(f"case {cid} Float{precision} iteration {iteration}: {nmis} of {P} states differ; nearest CDF boundary {ref.margins.min():.2e}; "
                  f"{int(st['n_changed'])} markers changed")
            assert nmis == 0
            assert np.array_equal(alpha, delta * beta) and set(np.unique(delta)) <= {0.0, 1.0}
            # effects: every marker from the device's own history
            b_ref, bound = RR.conditional_recheck(cs.X, cs.Phi, cs.obs, cs.W, cs.alpha, alpha, states, iteration=iteration, seed=SEED, vare=cs.vare, G=cs.G)
            wb = float((np.abs(beta - b_ref) / bound).max())
            wa = float((np.abs(alpha - delta * b_ref) / bound).max())
            print(f"    beta worst error / bound {wb:.3e} (largest bound {bound.max():.2e}, largest |beta| {np.abs(beta).max():.2e}); alpha {wa:.3e}; "
                  f"against the restatement's own chain: {np.abs(beta - ref.beta).max():.2e}")
            assert wb <= 1.0 and wa <= 1.0
            # statistics
            assert np.array_equal(st["state_counts"], np.bincount(states, minlength=1 << c).astype(np.float64))
            assert np.array_equal(st["state_counts"], ref.state_counts) and st["n_changed"] == ref.n_changed
            assert st["n_changed"] == float((np.abs(alpha - cs.alpha).sum(axis=0) != 0).sum())
            bss, bss_abs = beta @ beta.T, np.abs(beta) @ np.abs(beta).T
            w1 = float((np.abs(st["beta_ss"] - bss) / (2 * (P + 2) * U * bss_abs)).max())
            w2 = abs(st["alpha_ss"] - (alpha * alpha).sum()) / (2 * (c * P + 2) * U * (alpha * alpha).sum())
            w3 = abs(st["resid_ss"] - (W * W).sum()) / (2 * (T * 512 + 2) * U * (W * W).sum())
            print(f"    statistics worst error / bound: beta'beta {w1:.3f}, sum alpha^2 {w2:.3f}, sum W^2 {w3:.3f}")
            assert max(w1, w2, w3) <= 1.0 and np.array_equal(st["beta_ss"], st["beta_ss"].T)
            # the residual: the apply recomputed from the device's own change list, markers ascending
            Wn, terms = cs.W.copy(), np.abs(cs.W)
            d = cs.alpha - alpha
            for j in np.flatnonzero(np.abs(d).sum(axis=0) != 0):
                g = RR.phi_times(cs.Phi, d[:, j])
                RR.apply_change(Wn, cs.obs, cs.X[:, j], g)
                terms = terms + np.where(cs.obs, np.abs(cs.X[:, j])[None, :] * np.abs(g)[:, None], 0.0)
            wr = float((np.abs(W - Wn) / (4 * U * terms + 1e-300)).max())
            print(f"    residual worst error / bound {wr:.3f} ({'bit-equal' if np.array_equal(W, Wn) else 'not bit-equal'}); "
                  f"{int((~cs.obs).sum())} cells without a record")
            assert wr <= 1.0 and np.all(W[~cs.obs] == 0.0)
    finally:
        hip.close()


# ---- 4. block sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_block_sizes_agree(precision):
    cs = _case(1)
    gs = 0.01
    runs = {}
    for bs in (1, 40, 100):
        hip = _engine(cs, precision, bs)
        try:
            _upload(hip, cs)
            hip.rrm_sweep(iteration=1, seed=SEED, vare=cs.vare, G=cs.G * gs, log_pi=cs.log_pi)
            runs[bs] = hip.rrm_get_state()
        finally:
            hip.close()
    ref = _reference(1, 1, 40, gs, True)
    err = ref.err_beta
    print(f"tight prior: largest propagated bound {err.max():.2e}, largest |beta| {np.abs(ref.beta).max():.2e}")
    assert err.max() < 1e-3 * np.abs(ref.beta).max()                    # (the bound means something)
    for bs in (1, 40, 100):
        a, b, d = runs[bs]
        assert np.array_equal(_states(d), ref.states)
        w = float((np.abs(b - ref.beta) / err).max())
        print(f"Float{precision} blocks of {bs}: beta worst error / bound against the restatement {w:.3e}")
        assert w <= 1.0
    for bs in (1, 100):
        w = float((np.abs(runs[bs][1] - runs[40][1]) / (2 * err)).max())
        wa = float((np.abs(runs[bs][0] - runs[40][0]) / (2 * err)).max())
        print(f"Float{precision} blocks of {bs} against 40: beta {w:.3e}, alpha {wa:.3e} of the bound")
        assert w <= 1.0 and wa <= 1.0


# ---- 5. the same seed gives the same bits ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal_and_iterations_differ():
    cs = _case(1)
    outs = []
    for _ in range(2):
        hip = _engine(cs, 32)
        try:
            _upload(hip, cs)
            stats = [hip.rrm_sweep(iteration=it, seed=SEED, vare=cs.vare, G=cs.G, log_pi=cs.log_pi) for it in range(1, 6)]
            outs.append((hip.rrm_get_state(), hip.rrm_get_residual(), stats))
        finally:
            hip.close()
    (s0, w0, t0), (s1, w1, t1) = outs
    assert all(np.array_equal(x, y) for x, y in zip(s0, s1)) and np.array_equal(w0, w1)
    for x, y in zip(t0, t1):
        assert all(np.array_equal(x[k], y[k]) for k in ("state_counts", "beta_ss", "alpha_ss", "resid_ss", "n_changed"))
    hip = _engine(cs, 32)
    try:
        got = []
        for it in (1, 2):
            _upload(hip, cs)
            hip.rrm_sweep(iteration=it, seed=SEED, vare=cs.vare, G=cs.G, log_pi=cs.log_pi)
            got.append(hip.rrm_get_state())
        assert not np.array_equal(got[0][1], got[1][1]) and not np.array_equal(got[0][2], got[1][2])
    finally:
        hip.close()


# ---- 6. the draws follow the closed-form posterior -------------------------------------------------------------------------------------------
def test_one_marker_draws_follow_the_closed_form_posterior_on_the_device():
    import jwas_jl_amd as J
    case = RR.conditional_case()
    prob, _ = RR.conditional_posterior(case)
    hip = J.HipEngine(0, precision=64)
    try:
        RR.conditional_engine(hip, case)
        rows_state, rows_coef = RR.conditional_check(hip, case)
        for s, zf in rows_state:
            print(f"device, state {s}: frequency {zf:.2f} se from P = {prob[s]:.4f}")
        for s, q, zm, zv in rows_coef:
            print(f"device, state {s} coefficient {q}: mean {zm:.2f} se, variance {zv:.2f} se")
        assert len(rows_state) == 4 and max(z for _, z in rows_state) <= 5.0
        assert len(rows_coef) == 8 and max(max(zm, zv) for _, _, zm, zv in rows_coef) <= 5.0
    finally:
        hip.close()


# ---- 7. the error contract ---------------------------------------------------------------------------------------------------------------------
def test_error_contract():
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    cs = _case(2)
    T, c = cs.T, cs.c
    X32 = np.asfortranarray(cs.X.astype(np.float32))

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    sweep_kw = dict(iteration=1, seed=1, vare=cs.vare, G=cs.G, log_pi=cs.log_pi)
    hip = J.HipEngine(0)
    try:
        def without_session():
            hip._rrm = (T, c, BS)
            return [code(hip.rrm_set_residual, cs.W), code(hip.rrm_get_residual), code(hip.rrm_set_state, cs.alpha), code(hip.rrm_get_state),
                    code(hip.rrm_sweep, **sweep_kw), code(hip.rrm_accumulate, 1), code(hip.rrm_posterior, 0), code(hip.rrm_mul_alpha, 0),
                    code(hip.rrm_m), code(hip.rrm_gram, 0), code(hip.rrm_end)]
        hip.n, hip.p = N, P
        assert code(hip.rrm_begin, cs.Phi, cs.obs, BS) == ESTATE             # no genotypes
        assert without_session() == [ESTATE] * 11
        hip.alloc_packed(N, P)
        assert code(hip.rrm_begin, cs.Phi, cs.obs, BS) == EUNSUP             # a packed context
        hip.load_dense(X32)
        hip.set_weights(np.linspace(0.5, 2.0, N).astype(np.float32))
        assert code(hip.rrm_begin, cs.Phi, cs.obs, BS) == EUNSUP             # residual weights
        hip.set_weights(None)
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.rrm_begin, cs.Phi, cs.obs, BS) == EUNSUP             # shards
        hip.comm_destroy()
        for phi in (np.ones((T, 1)), np.ones((T, 5))):
            assert code(hip.rrm_begin, phi, cs.obs, BS) == EINVAL            # c out of range
        assert code(hip.rrm_begin, np.ones((65, 2)), np.ones((65, N), dtype=bool), BS) == EINVAL      # T out of range
        assert code(hip.rrm_begin, cs.Phi, cs.obs[:, :N - 1], BS) == EINVAL  # a wrong n
        assert code(hip.rrm_begin, cs.Phi, cs.obs, 257) == EINVAL and code(hip.rrm_begin, cs.Phi, cs.obs, -1) == EINVAL
        for bad in (np.nan, np.inf):
            phi = cs.Phi.copy(); phi[1, 1] = bad
            assert code(hip.rrm_begin, phi, cs.obs, BS) == EINVAL
        mask = np.full(N, 0b111, dtype=np.uint64)                             # a record bit at T
        raw = lambda: hip._chk(hip._L.jwas_hip_rrm_begin(hip._h, T, c, N, cs.Phi.ctypes.data, mask.ctypes.data, BS))      # noqa: E731
        assert code(raw) == EINVAL
        assert without_session() == [ESTATE] * 11                            # none of the failed calls opened a session
        hip.rrm_begin(cs.Phi, cs.obs, BS)
        _upload(hip, cs)
        before = (hip.rrm_get_state(), hip.rrm_get_residual())
        Gnpd = np.array([[1.0, 2.0], [2.0, 1.0]])
        Gasym = np.array([[1.0, 0.1], [0.2, 1.0]])
        for bad in (dict(iteration=0), dict(vare=0.0), dict(vare=-1.0), dict(vare=np.nan), dict(vare=np.inf), dict(G=Gnpd), dict(G=Gasym),
                    dict(G=np.array([[np.nan, 0.0], [0.0, 1.0]])), dict(G=np.array([[np.inf, 0.0], [0.0, 1.0]])), dict(G=np.zeros((2, 2))),
                    dict(log_pi=np.array([0.0, np.nan, 0.0, 0.0])), dict(log_pi=np.full(4, -np.inf)), dict(log_pi=np.array([np.inf, 0, 0, 0.0]))):
            kw = dict(sweep_kw); kw.update(bad)
            assert code(hip.rrm_sweep, **kw) == EINVAL, bad
        assert code(hip.rrm_accumulate, 0.5) == EINVAL and code(hip.rrm_posterior, 2) == EINVAL and code(hip.rrm_mul_alpha, -1) == EINVAL
        assert code(hip.rrm_gram, 3) == EINVAL
        Wnan = cs.W.copy(); Wnan[1, 5] = np.nan
        anan = cs.alpha.copy(); anan[0, 3] = np.inf
        assert code(hip.rrm_set_residual, Wnan) == EINVAL and code(hip.rrm_set_state, anan) == EINVAL
        assert code(hip.rrm_set_state, None, None, cs.delta * 0.5 + 0.25) == EINVAL
        buf = np.empty(7)
        assert code(lambda: hip._chk(hip._L.jwas_hip_rrm_get_m(hip._h, 7, buf.ctypes.data))) == EINVAL
        after = (hip.rrm_get_state(), hip.rrm_get_residual())
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])      # nothing was launched
        for post in hip.rrm_posterior(0):
            assert np.all(post == 0.0)
        hip.rrm_begin(cs.Phi, cs.obs, 0)                                      # _begin on an open session replaces it; 0: blocks of 64
        assert hip.rrm_gram(1).shape == (36, 36, 2, 2) and np.all(hip.rrm_get_residual() == 0.0) and np.all(hip.rrm_get_state()[2] == 1.0)
        assert J.HipEngine.rrm_estimate_bytes(N, P, T, c, 64) == RrmStandInEngine.rrm_estimate_bytes(N, P, T, c, 64) > 8 * P * 64 * 3
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.rrm_sweep, **sweep_kw) == EUNSUP
        hip.comm_destroy()
        hip.rrm_sweep(**sweep_kw)
        hip.load_dense(X32)                                                   # loading genotypes frees the session
        assert without_session() == [ESTATE] * 11
        hip.rrm_begin(cs.Phi, cs.obs, BS)
        hip.rrm_end()
        assert without_session() == [ESTATE] * 11
    finally:
        hip.close()
    hip = J.HipEngine(0, precision=64)                                        # a Float64 context: weights refused, then accepted again as ones
    try:
        hip.load_dense(np.asfortranarray(cs.X))
        hip.set_weights(np.linspace(0.5, 2.0, N))
        hip._rrm = None
        assert code(hip.rrm_begin, cs.Phi, cs.obs, BS) == EUNSUP
        hip.set_weights(None)
        hip.rrm_begin(cs.Phi, cs.obs, BS)
    finally:
        hip.close()


# ---- 8. runMCMC ------------------------------------------------------------------------------------------------------------------------------
def test_runmcmc_gpu_vs_standin(tmp_path):
    from test_rrm_host import check_outputs, rrm_data, run_rrm
    data = rrm_data(n=120, p=150, T=5, c=3, seed=9)
    outs = {}
    for name, engine in (("ref", RrmStandInEngine(64)), ("hip", None)):
        outs[name] = run_rrm(tmp_path, name, data=data, engine=engine, chain_length=40, burnin=10, seed=13, block_size=40)
    p = len(outs["hip"]["marker effects geno"]) // 3

    def diff(key, col):
        return float(np.abs(outs["hip"][key][col].to_numpy(dtype=np.float64) - outs["ref"][key][col].to_numpy(dtype=np.float64)).max())
    d_eff = diff("marker effects geno", "Estimate")
    d_ebv = max(diff(f"EBV_{q}", "EBV") for q in (1, 2, 3))
    d_var = 0.0
    for f in ("residual_variance", "marker_effects_variances_geno", "pi_geno"):
        a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{f}.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
        assert a.shape == b.shape and a.shape[0] == 30
        d_var = max(d_var, float(np.abs(a - b).max()))
    a, b = (np.loadtxt(tmp_path / nm / "MCMC_samples_marker_effects_geno_2.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
    d_smp = float(np.abs(a - b).max())
    print(f"runMCMC RRM: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, variance and pi samples {d_var:.3e}, effect samples {d_smp:.3e}")
    assert d_eff <= 1e-8 and d_ebv <= 1e-7 and d_var <= 1e-9 and d_smp <= 1e-8
    np.testing.assert_allclose(outs["hip"]["marker effects geno"]["Model_Frequency"].to_numpy(dtype=np.float64),
                               outs["ref"]["marker effects geno"]["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)
    assert outs["hip"]["pi_geno"]["SD"].max() > 0 and np.any(outs["hip"]["marker effects geno"]["Estimate"] != 0.0)
    check_outputs(outs["hip"], str(tmp_path / "hip"), 120, p, 3, 30)
    # Float32 storage: it runs, every file is present, every value finite
    with contextlib.redirect_stdout(io.StringIO()):
        f32 = run_rrm(tmp_path, "f32", data=data, engine=None, double=False, chain_length=40, burnin=10, seed=13, block_size=40)
    check_outputs(f32, str(tmp_path / "f32"), 120, p, 3, 30)
    assert os.path.exists(tmp_path / "f32" / "EBV_3.txt")
