"""Several chains of one model on the device: the BayesR sweep of the session (k_mega_sample_r), the potential scale reduction factor
(k_mega_psrf) and runMCMC(chains=K), against the numpy restatement of tests/chains_reference.py on the same Philox counters.

Shapes: n = 301 individuals (two 256-row slices, the second ragged), p = 100 markers in blocks of 64 (a full 64-lane sub-block, then a
ragged block of 36) and of 100 (one block: a full sub-block and a ragged second one), and of 1 and 40 where named; K in {1, 9, 64}
chains (one; two trait tiles of k_mega_update_partial, the second ragged; the maximum); pi and gamma change from chain to chain, one
pi with an empty null class and one with an empty class 2.  Genotypes are count - 2 freq rounded to Float32, so the sums do round.
The device and the restatement evaluate the same formulas in double (the library is built without FMA contraction) and differ in
the ORDER of the O(n) sums and in the libm behind log, exp and Box-Muller.  With u = 2^-53:

    classes        discrete: EQUAL to the restatement's own chain (chains_reference asserts that no decision uniform of that chain lies
                   within 1e-9 of a CDF boundary; tests/test_chains_host.py runs that check on the CPU)
    effects        every marker against the restatement evaluated from the DEVICE's own history under the device's class
                   (chains_reference.conditional_recheck_r): in class c > 1 the draw is the BayesC draw with v = gamma_c sigma2, so the
                   bound is mega_reference.marker_bound with that v; in class 1 both sides hold exactly 0
    statistics     the class counts, nnz and n_changed exact; the sums against numpy sums of the device's own state:
                   2 (K + 2) u sum |terms| for K terms (the terms alpha^2 / gamma are the same IEEE operations on both sides)
    residual       BIT-EQUAL to the apply recomputed in numpy from the device's own change lists (the same operations in the same order)
    PSRF           chains_reference.psrf_bound: the cancellation in q - m^2 carried through W, V and the ratio
Chain k of a K-chain session is compared with a one-chain session BIT FOR BIT.  Every test prints the figures it measured before it
asserts."""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest

import chains_reference as CR
import mega_reference as MR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4
N, P, SEED, LD = 301, 100, 5, 512
SWEEP_CASES = [(K, prec, bs) for K in (1, 9, 64) for prec in (32, 64) for bs in (64, 100)] + [(9, 64, 1), (9, 32, 40)]


@functools.lru_cache(maxsize=None)
def _case():
    return CR.make_case_r(N, P)


@functools.lru_cache(maxsize=None)
def _reference(bs, K=64):
    """The restatement's own two consecutive sweeps of the first K chains (computed once per block size, shared, never changed).  Chain
    k of it serves every session that holds chain k: the chains are independent, and the 1e-9 margin of every decision (asserted
    inside) is far above the rounding by which numpy's sums move with the shape."""
    return CR.reference_sweeps_r(_case(), K, SEED, bs)


def _engine(precision, K, bs, first=0):
    import jwas_jl_amd as J
    hip = J.HipEngine(0, precision=precision)
    hip.load_dense(np.asfortranarray(_case().X.astype(hip.dtype)))
    hip.mega_begin(K, bs, first)
    return hip


def _upload(hip, c):
    hip.mega_set_residual(c.R)
    hip.mega_set_state(c.alpha, c.alpha, None)                            # (delta is not read by the law; set_state takes 0 / 1 only)


def _sweep(hip, c, iteration):
    return hip.mega_sweep_r(iteration=iteration, seed=SEED, vare=c.vare, var_effect=c.sig, gamma=c.gamma, pi=c.pi)


# ---- 5. two sweeps from a common uploaded state, iterations 1 and 2 -----------------------------------------------------------------------
@pytest.mark.parametrize("K,precision,bs", SWEEP_CASES)
def test_bayesr_sweep_classes_effects_statistics_residual(K, precision, bs):
    cs = _case()
    c = CR.case_chains(cs, K)
    refs = _reference(bs, 64 if bs in (64, 100) else 9)
    hip = _engine(precision, K, bs)
    try:
        _upload(hip, c)
        R0, a0 = c.R.copy(), c.alpha.copy()
        for iteration, ref in zip((1, 2), refs):
            st = _sweep(hip, c, iteration)
            alpha, beta, delta = hip.mega_get_state()
            R = hip.mega_get_residual()
            nmis = int((delta != ref.delta[:K]).sum())
            print(f"K = {K} Float{precision} blocks of {bs} iteration {iteration}: {nmis} of {K * P} classes differ; nearest boundary "
                  f"{ref.margins[:K].min():.2e}; {int(st['n_changed'].sum())} effects changed")
            assert nmis == 0
            assert np.array_equal(beta, alpha) and np.array_equal(alpha == 0.0, delta == 1.0) and set(np.unique(delta)) <= {1.0, 2.0, 3.0, 4.0}
            # effects: every marker from the device's own history, under the device's class
            a_ref, bound = CR.conditional_recheck_r(cs.X, R0, a0, alpha, delta, iteration=iteration, seed=SEED, vare=c.vare, var_effect=c.sig, gamma=c.gamma)
            inm = delta > 1.0
            assert np.all(alpha[~inm] == 0.0) and np.all(a_ref[~inm] == 0.0)
            wb = float((np.abs(alpha - a_ref)[inm] / bound[inm]).max())
            print(f"    effects worst error / bound {wb:.3e} (largest bound {bound.max():.2e}, largest |alpha| {np.abs(alpha).max():.2e}); "
                  f"against the restatement's own chain: {np.abs(alpha - ref.alpha[:K]).max():.2e}")
            assert wb <= 1.0 and np.all(np.isfinite(alpha))
            # statistics: the counts exact, the sums against numpy sums of the device's own state
            counts = np.stack([(delta == q + 1.0).sum(axis=1).astype(np.float64) for q in range(4)])
            assert np.array_equal(st["class_counts"], counts) and np.array_equal(st["class_counts"], ref.class_counts[:, :K])
            assert np.array_equal(st["nnz"], inm.sum(axis=1).astype(np.float64))
            assert np.array_equal(st["n_changed"], (alpha != a0).sum(axis=1).astype(np.float64)) and np.array_equal(st["n_changed"], ref.n_changed[:K])
            g = np.take_along_axis(c.gamma, (delta.astype(np.int64) - 1).T, axis=0).T
            with np.errstate(divide="ignore", invalid="ignore"):
                terms = np.where(inm, alpha * alpha / g, 0.0)
            w1 = float((np.abs(st["ssq"] - terms.sum(axis=1)) / (2 * (P + 2) * U * terms.sum(axis=1) + 1e-300)).max())
            w2 = float((np.abs(st["alpha_ss"] - (alpha * alpha).sum(axis=1)) / (2 * (P + 2) * U * (alpha * alpha).sum(axis=1) + 1e-300)).max())
            w3 = float((np.abs(st["resid_ss"] - (R * R).sum(axis=1)) / (2 * (LD + 2) * U * (R * R).sum(axis=1))).max())
            w4 = float((np.abs(st["resid_sum"] - R.sum(axis=1)) / (2 * (LD + 2) * U * np.abs(R).sum(axis=1))).max())
            print(f"    statistics worst error / bound: ssq {w1:.3f}, alpha'alpha {w2:.3f}, sum r^2 {w3:.3f}, sum r {w4:.3f}")
            assert max(w1, w2, w3, w4) <= 1.0
            # the residual: the apply recomputed from the device's own change lists, block by block, markers ascending per chain
            Rn, d = R0.copy(), a0 - alpha
            for j0 in range(0, P, bs):
                MR.apply_changes(Rn, cs.X[:, j0:j0 + bs], d[:, j0:j0 + bs])
            print(f"    residual {'bit-equal' if np.array_equal(R, Rn) else 'NOT bit-equal'} (largest difference {np.abs(R - Rn).max():.2e})")
            assert np.array_equal(R, Rn)
            R0, a0 = R, alpha
    finally:
        hip.close()


# ---- 6. no sum of chain k depends on K ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_chain_k_is_bit_equal_to_a_one_chain_session(precision):
    cs = _case()
    c17 = CR.case_chains(cs, 17)
    hip = _engine(precision, 17, 64)
    try:
        _upload(hip, c17)
        full = []
        for it in (1, 2):
            st = _sweep(hip, c17, it)
            full.append((st, hip.mega_get_state(), hip.mega_get_residual()))
    finally:
        hip.close()
    for k in (0, 8, 16):
        c1 = CR.case_chains(cs, 1, k)
        one = _engine(precision, 1, 64, first=k)
        try:
            _upload(one, c1)
            for it, (st17, state17, R17) in zip((1, 2), full):
                st = _sweep(one, c1, it)
                state, R = one.mega_get_state(), one.mega_get_residual()
                for a, b in zip(state, state17):
                    assert np.array_equal(a[0], b[k])
                assert np.array_equal(R[0], R17[k])
                for key in CR.R_STAT_KEYS:
                    assert np.array_equal(np.asarray(st[key])[..., 0], np.asarray(st17[key])[..., k]), (k, it, key)
        finally:
            one.close()
    assert not np.array_equal(full[1][1][0][0], full[1][1][0][4])


# ---- 7. the same seed gives the same bits; the chain id matters ------------------------------------------------------------------------------
def test_two_runs_are_bit_equal_and_chain_ids_differ():
    cs = _case()
    c = CR.case_chains(cs, 1)
    K = 4
    same = CR.SweepResult(R=np.tile(c.R, (K, 1)), alpha=np.tile(c.alpha, (K, 1)), vare=np.repeat(c.vare, K), sig=np.repeat(c.sig, K),
                          gamma=np.repeat(c.gamma, K, axis=1), pi=np.repeat(c.pi, K, axis=1))
    runs = []
    for _ in range(2):
        hip = _engine(32, K, 40)
        try:
            _upload(hip, same)
            stats = [_sweep(hip, same, it) for it in range(1, 6)]
            runs.append((stats, hip.mega_get_state(), hip.mega_get_residual()))
        finally:
            hip.close()
    for sa, sb in zip(runs[0][0], runs[1][0]):
        for key in CR.R_STAT_KEYS:
            assert np.array_equal(sa[key], sb[key]), key
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)
    assert np.array_equal(runs[0][2], runs[1][2])
    alpha = runs[0][1][0]
    for k in range(1, K):                                                  # equal inputs, different Philox ids
        assert not np.array_equal(alpha[0], alpha[k]) and not np.array_equal(runs[0][2][0], runs[0][2][k])


# ---- 8. the draws follow the closed-form posterior ----------------------------------------------------------------------------------------
def test_one_marker_bayesr_draws_follow_the_closed_form_posterior_on_the_device():
    import jwas_jl_amd as J
    case = CR.conditional_case_r()
    probs, _, _ = CR.conditional_posterior_r(case)
    assert (probs * CR.CONDITIONAL_STEPS).min() >= CR.MIN_EXPECTED
    hip = J.HipEngine(0, precision=64)
    try:
        rows = CR.conditional_check_r(CR.conditional_engine_r(hip, case), case)
        for k, c, ex, zf, zm, zv in rows:
            print(f"device, chain {k} class {c}: expected {ex:.0f}; frequency {zf:.2f} se; effect mean {zm:.2f}, variance {zv:.2f}")
        assert len(rows) == 12 and max(max(r[3:]) for r in rows) <= 5.0
    finally:
        hip.close()


# ---- 9. the potential scale reduction factor ------------------------------------------------------------------------------------------------
def test_psrf_kernel_against_numpy():
    """9 chains, 6 saved samples of BayesR sweeps from the session's starting state under a sparse prior, so that some markers never
    enter the model in any chain (W == 0: NaN) and most do."""
    cs = _case()
    K, nsamp = 9, 6
    c = CR.case_chains(cs, K)
    pi = np.repeat(np.array([[0.99], [0.005], [0.003], [0.002]]), K, axis=1)
    hip = _engine(64, K, 64)
    try:
        hip.mega_set_residual(c.R)
        for it in range(1, nsamp + 1):
            hip.mega_sweep_r(iteration=it, seed=SEED, vare=c.vare, var_effect=c.sig, gamma=c.gamma, pi=pi)
            hip.mega_accumulate_r(it)
        got = hip.mega_psrf(nsamp)
        post = [hip.mega_posterior(k) for k in range(K)]
        _, _, delta = hip.mega_get_state()
    finally:
        hip.close()
    m, q, f = (np.stack([pk[i] for pk in post]) for i in range(3))
    assert np.all((f >= 0.0) & (f <= 1.0)) and np.array_equal(f == 0.0, q == 0.0)      # the model frequency of BayesR: class > 1, a nonzero effect
    want, bound = CR.psrf_from_moments(m, q, float(nsamp)), CR.psrf_bound(m, q, float(nsamp))
    never = np.all(q == 0.0, axis=0)
    print(f"PSRF: {int(never.sum())} of {P} markers never in the model; {int(np.isinf(bound[~never]).sum())} undetermined; finite values in "
          f"[{np.nanmin(got):.3f}, {np.nanmax(got):.3f}]")
    assert 0 < never.sum() < P and np.array_equal(np.isnan(got), never) and np.array_equal(np.isnan(want), never)
    ok = ~never & np.isfinite(bound)
    assert ok.sum() >= (~never).sum() - 2
    worst = float((np.abs(got - want)[ok] / bound[ok]).max())
    print(f"      worst error / bound {worst:.3e} (largest bound {bound[ok].max():.2e})")
    assert worst <= 1.0 and np.all(got[~never] > 0.0)


def test_psrf_beyond_one_grid_trip_and_pure_function_of_the_accumulators():
    """k_mega_psrf runs at most 64 workgroups of 256 threads: p = 16 421 takes a second trip.  The accumulators are filled through
    set_state + accumulate (no sweep): two samples of three chains, every eighth marker 0 in all of them."""
    import jwas_jl_amd as J
    rng = np.random.default_rng(11)
    p, K = 64 * 256 + 37, 3
    X = np.asfortranarray(np.tile((rng.binomial(2, 0.4, size=(9, 8)) - 0.8).astype(np.float32), (1, p // 8 + 1))[:, :p])
    samples = rng.standard_normal((2, K, p)) * 0.1
    samples[:, :, ::8] = 0.0
    hip = J.HipEngine(0)
    try:
        hip.load_dense(X)
        hip.mega_begin(K, 256, 0)
        for i in range(2):
            hip.mega_set_state(samples[i], None, None)
            hip.mega_accumulate(i + 1)
        got, again = hip.mega_psrf(2), hip.mega_psrf(2)
        post = [hip.mega_posterior(k) for k in range(K)]
    finally:
        hip.close()
    m, q = (np.stack([pk[i] for pk in post]) for i in range(2))
    want, bound = CR.psrf_from_moments(m, q, 2.0), CR.psrf_bound(m, q, 2.0)
    never = np.zeros(p, dtype=bool)
    never[::8] = True
    assert np.array_equal(got, again, equal_nan=True) and np.array_equal(np.isnan(got), never)
    ok = ~never & np.isfinite(bound)
    worst = float((np.abs(got - want)[ok] / bound[ok]).max())
    print(f"PSRF at p = {p}: {int((~ok & ~never).sum())} undetermined, worst error / bound {worst:.3e}; last marker {got[-1]:.6f} against {want[-1]:.6f}")
    assert ok.sum() >= 0.99 * (~never).sum() and ok[16384:].sum() > 25 and worst <= 1.0


# ---- 10. the error contract ---------------------------------------------------------------------------------------------------------------------
def test_error_contract():
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    cs = _case()
    K = 5
    c = CR.case_chains(cs, K)
    X32 = np.asfortranarray(cs.X.astype(np.float32))

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    sweep_kw = dict(iteration=1, seed=1, vare=c.vare, var_effect=c.sig, gamma=c.gamma, pi=c.pi)
    hip = J.HipEngine(0)
    try:
        def without_session():
            hip._mega = (K, 64)
            return [code(hip.mega_sweep_r, **sweep_kw), code(hip.mega_accumulate_r, 1), code(hip.mega_psrf, 2)]
        hip.n, hip.p = N, P
        assert without_session() == [ESTATE] * 3                             # no genotypes, no session
        hip.load_dense(X32)
        assert without_session() == [ESTATE] * 3
        hip.mega_begin(K, 64)
        _upload(hip, c)
        before = (hip.mega_get_state(), hip.mega_get_residual())
        bads = [("iteration", None, 0)]
        bads += [(key, None, bad) for key in ("vare", "var_effect") for bad in (0.0, -1.0, np.nan, np.inf)]
        bads += [("gamma", 0, 0.01), ("gamma", 0, 1e-300), ("gamma", 2, 0.0), ("gamma", 1, -1.0), ("gamma", 3, np.inf), ("gamma", 3, np.nan)]
        bads += [("pi", 1, -0.1), ("pi", 0, 1.5), ("pi", 2, np.nan), ("pi", 3, c.pi[3, K - 1] + 1e-6), ("pi", 0, c.pi[0, K - 1] + 2e-8)]
        for key, row, bad in bads:
            kw = dict(sweep_kw)
            if key == "iteration":
                kw[key] = bad
            else:
                kw[key] = kw[key].copy()
                kw[key][(row, K - 1) if row is not None else K - 1] = bad
            assert code(hip.mega_sweep_r, **kw) == EINVAL, (key, row, bad)
        near = c.pi.copy()
        near[0, 0] += 5e-9                                                   # within 1e-8 of 1: accepted (checked below, after the state check)
        P_, S_ = _lib.MegaRParams(), _lib.MegaRStats()
        assert code(lambda: hip._chk(hip._L.jwas_hip_mega_sweep_r(hip._h, None, C.byref(S_)))) == EINVAL
        assert code(lambda: hip._chk(hip._L.jwas_hip_mega_sweep_r(hip._h, C.byref(P_), None))) == EINVAL
        P_.iteration = 1
        assert code(lambda: hip._chk(hip._L.jwas_hip_mega_sweep_r(hip._h, C.byref(P_), C.byref(S_)))) == EINVAL      # NULL parameter arrays
        assert code(hip.mega_accumulate_r, 0.5) == EINVAL
        assert code(hip.mega_psrf, 1) == EINVAL and code(hip.mega_psrf, np.nan) == EINVAL
        assert code(lambda: hip._chk(hip._L.jwas_hip_mega_psrf(hip._h, 2.0, None))) == EINVAL
        after = (hip.mega_get_state(), hip.mega_get_residual())
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])      # nothing was launched
        for post in hip.mega_posterior(0):
            assert np.all(post == 0.0)
        kw = dict(sweep_kw)
        kw["pi"] = near
        st = hip.mega_sweep_r(**kw)
        assert np.array_equal(st["class_counts"].sum(axis=0), np.full(K, float(P)))
        # the BayesC accumulate keeps its meaning (the mean of delta), the BayesR one counts class > 1
        delta = hip.mega_get_state()[2]
        hip.mega_accumulate_r(1)
        assert np.array_equal(hip.mega_posterior(1)[2], (delta[1] > 1.0).astype(np.float64))
        hip.mega_accumulate(1)
        assert np.array_equal(hip.mega_posterior(1)[2], delta[1])
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mega_sweep_r, **sweep_kw) == EUNSUP and code(hip.mega_psrf, 2) == EUNSUP
        hip.comm_destroy()
        hip.mega_begin(1, 64)                                                 # one chain: no statistic over chains
        assert code(hip.mega_psrf, 2) == EINVAL
        hip.mega_end()
        assert without_session() == [ESTATE] * 3
    finally:
        hip.close()


# ---- 11. runMCMC(chains=9) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["BayesC", "BayesR"])
def test_runmcmc_chains_gpu_vs_standin(tmp_path, method):
    """9 chains, 12 iterations: the device against the stand-in engine through the whole driver.  The host draws read the engines'
    statistics, which differ by rounding; no class may flip (Model_Frequency equal), and the sample files are compared as
    tests/test_gpu_megatrait.py compares its own: the FIRST saved iteration within 1e-10 relative, the chain within 1e-8."""
    from test_chains_host import chain_data, run_k
    data = chain_data(n=120, p=150, seed=9)
    K = 9
    outs = {}
    for name, engine in (("ref", CR.ChainsStandInEngine(64)), ("hip", None)):
        outs[name] = run_k(tmp_path, name, data=data, engine=engine, method=method, chains=K, chain_length=12, burnin=2, seed=13, block_size=40)
    first, chain = 0.0, 0.0
    for k in range(K):
        np.testing.assert_array_equal(outs["hip"]["chains"][k]["marker effects geno"]["Model_Frequency"].to_numpy(),
                                      outs["ref"]["chains"][k]["marker effects geno"]["Model_Frequency"].to_numpy())
        for f in ("residual_variance", "marker_effects_variances_geno", "pi_geno", "heritability", "marker_effects_geno_y"):
            a, b = (np.loadtxt(tmp_path / nm / f"chain_{k}" / f"MCMC_samples_{f}.txt", delimiter=",", skiprows=1, ndmin=2) for nm in ("ref", "hip"))
            assert a.shape == b.shape and a.shape[0] == 10
            assert np.array_equal(a == 0.0, b == 0.0), f
            first = max(first, float((np.abs(a[0] - b[0]) / (np.abs(a[0]).max())).max()))
            chain = max(chain, float((np.abs(a - b) / np.abs(a).max()).max()))
    ph, pr = outs["hip"]["PSRF"]["PSRF"].to_numpy(), outs["ref"]["PSRF"]["PSRF"].to_numpy()
    seen = np.array([np.loadtxt(tmp_path / "hip" / f"chain_{k}" / "MCMC_samples_marker_effects_geno_y.txt", delimiter=",", skiprows=1).any(axis=0) for k in range(K)]).any(axis=0)
    d_psrf = float(np.nanmax(np.abs(ph - pr) / pr))
    print(f"runMCMC(chains={K}), {method}: first saved iteration {first:.3e} relative, whole chain {chain:.3e}; PSRF {d_psrf:.3e} relative; "
          f"{int(seen.sum())} of 150 markers entered a model; largest PSRF {np.nanmax(ph[:150]):.3f}")
    assert first <= 1e-10 and chain <= 1e-8
    assert np.array_equal(np.isfinite(ph[:150]), seen) and np.array_equal(np.isnan(ph), np.isnan(pr)) and np.all(np.isfinite(ph[150:]))
    assert seen.sum() > 50
    # Float32 storage: it runs, the layout is the same, every PSRF row that should be finite is
    with contextlib.redirect_stdout(io.StringIO()):
        f32 = run_k(tmp_path, "f32", data=data, engine=None, double=False, method=method, chains=K, chain_length=12, burnin=2, seed=13, block_size=40)
    assert len(f32["chains"]) == K and np.all(np.isfinite(f32["PSRF"]["PSRF"].to_numpy()[150:]))
