"""Float64 device context (runMCMC(double_precision=true)) for multi-trait sampler II, multi-trait BayesA/B (one t x t effect
covariance per marker, sampler I and II) and marker-specific joint priors, against the Float64 restatement of
tests/f64_mt_reference.py.  The contract of test_gpu_f64.py: joint-state trajectories and state counts identical; effects and
residuals within 1e-9 relative (both sides in double; only the association of the sums differs)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import make_dataset
from f64_mt_reference import RestatementEngine64
from test_f64_multitrait_host import run_mt_case

pytestmark = pytest.mark.gpu

EUNSUP = -4


def _pair(n, p, t, method, bs=None, starts=None, seed=3):
    import jwas_jl_amd as J
    d = make_dataset(n=n, p=p, ncausal=8, seed=seed)
    X = np.asfortranarray(d["X"].astype(np.float64))
    hip, ref = J.HipEngine(0, precision=64), RestatementEngine64()
    rng = np.random.default_rng(seed)
    y = d["y"] - d["y"].mean()
    for e in (ref, hip):
        e.load_dense(X)
        if starts is not None:
            e.setup_blocks_explicit(np.asarray(starts))
        else:
            e.setup_blocks(bs)
        e.init_state(method, t)
    for k in range(t):
        yk = (1 + 0.3 * k) * y + 0.3 * rng.standard_normal(n)
        for e in (ref, hip):
            e.set_residual(yk, k)
            e.set_state(k, delta=np.ones(p))
    A = rng.standard_normal((t, t)); B = rng.standard_normal((t, t))
    R = (A @ A.T / t + np.eye(t)) * 0.5
    G = (B @ B.T / t + np.eye(t)) * 0.004
    return hip, ref, R, G, rng


def _compare(ref, hip, t):
    for k in range(t):
        ao, bo, do = ref.get_state(k)
        ah, bh, dh = hip.get_state(k)
        assert np.array_equal(do, dh), f"trait {k}: indicators differ at {np.flatnonzero(do != dh)[:5]}"
        np.testing.assert_allclose(ah, ao, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(bh, bo, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(hip.get_residual(k), ref.get_residual(k), rtol=0, atol=1e-9)


def _run(hip, ref, t, sweeps, it0=1, **kw):
    for it in range(it0, it0 + sweeps):
        so = ref.sweep(iteration=it, seed=4, **kw)
        sh = hip.sweep(iteration=it, seed=4, **kw)
        assert np.array_equal(so["state_counts"], sh["state_counts"]), f"iteration {it}: {so['state_counts']} vs {sh['state_counts']}"
        np.testing.assert_allclose(sh["beta_ss"], so["beta_ss"], rtol=1e-8)
        np.testing.assert_allclose(sh["resid_ss"], so["resid_ss"], rtol=1e-9)
    _compare(ref, hip, t)


def _prior(rng, t, restricted):
    lp = np.log(rng.dirichlet(np.ones(1 << t) * 2))
    if restricted:                                          # a Pi that leaves out joint states (MTBayesABC.jl:20-25)
        lp[1:(1 << t) - 1:2] = -np.inf
    return lp


@pytest.mark.parametrize("t,bs,p,restricted,independent,sweeps", [(2, 64, 64 * 3 + 17, True, False, 4), (3, 128, 300, False, False, 3),
                                                                   (4, 512, 600, True, False, 2), (2, 64, 64 * 2 + 30, False, True, 3)])
def test_f64_sampler2_parity(t, bs, p, restricted, independent, sweeps):
    hip, ref, R, G, rng = _pair(300, p, t, "MTBayesC_II", bs=bs, seed=20 + t)
    try:
        _run(hip, ref, t, sweeps, vare=R, var_effect=G, log_prior_states=_prior(rng, t, restricted), independent_blocks=independent)
    finally:
        hip.close()


def test_f64_sampler2_ragged_partition_with_repetitions():
    """fast_blocks as explicit ragged starts, every block repeated its own size (nreps = 0, BayesABC.jl:153)."""
    t = 2
    hip, ref, R, G, rng = _pair(260, 150, t, "MTBayesC_II", starts=[0, 5, 40, 41, 100], seed=31)
    try:
        _run(hip, ref, t, 2, vare=R, var_effect=G, log_prior_states=_prior(rng, t, True), nreps=0)
    finally:
        hip.close()


@pytest.mark.parametrize("method,t,bs,nreps", [("MTBayesB", 2, 128, 1), ("MTBayesB_II", 2, 64, 0), ("MTBayesB_II", 3, 64, 1),
                                               ("MTBayesB", 4, 512, 1)])
def test_f64_bayesb_parity(method, t, bs, nreps):
    """Multi-trait BayesA/B: per-marker covariances uploaded from the host, then drawn on the device from the double beta
    (sample_marker_covariances) between sweeps -- both sides draw on the same counters."""
    p = bs * 2 + 21 if bs < 512 else 560
    hip, ref, R, G, rng = _pair(280, p, t, method, bs=bs, seed=40 + t)
    try:
        vm = np.stack([G * rng.uniform(0.5, 2.0) + np.diag(rng.uniform(0, 0.002, t)) for _ in range(p)])
        lp = _prior(rng, t, method.endswith("II"))
        kw = dict(vare=R, var_effect=G, log_prior_states=lp, nreps=nreps)
        _run(hip, ref, t, 2, var_effect_matrix=vm, **kw)
        np.testing.assert_array_equal(hip.marker_covariances(), vm)
        assert hip.marker_covariances().dtype == np.float64
        for it in (3, 4):
            for e in (ref, hip):
                e.sample_marker_covariances(t + 3.0, G * 3.0, seed=4, iteration=it - 1)
            np.testing.assert_allclose(hip.marker_covariances(), ref.marker_covariances(), rtol=1e-10, atol=1e-15)
            _run(hip, ref, t, 1, it0=it, **kw)
    finally:
        hip.close()


@pytest.mark.parametrize("method,bs,nreps,independent", [("MTBayesC", 128, 1, False), ("MTBayesC_II", 512, 1, False),
                                                         ("MTBayesC", 64, 0, False), ("MTBayesC_II", 128, 1, True)])
def test_f64_joint_prior_matrix_parity(method, bs, nreps, independent):
    """Marker-specific joint priors (MarkerSpecificPiPrior, MTBayesABC.jl:22-47): a p x 4 table of log pi(state)."""
    t = 2
    p = 600 if bs == 512 else bs * 2 + 10
    hip, ref, R, G, rng = _pair(300, p, t, method, bs=bs, seed=51)
    try:
        lpm = np.log(rng.dirichlet(np.ones(4) * 2, size=p))
        _run(hip, ref, t, 3, vare=R, var_effect=G, log_prior_states=lpm, nreps=nreps, independent_blocks=independent)
    finally:
        hip.close()


@pytest.mark.parametrize("t", [2, 3, 4])
def test_f64_marker_covariance_draws_match_the_oracle(t):
    """The device's Float64 inverse-Wishart draws against orc_sample_marker_covariances on a beta that float32 holds exactly:
    the same counters and operation order, the oracle rounds its result to float."""
    hip, ref, R, G, rng = _pair(256, 700, t, "MTBayesB", bs=128, seed=60 + t)
    try:
        beta = (rng.standard_normal((t, 700)) * 0.05).astype(np.float32)
        for k in range(t):
            hip.set_state(k, beta=beta[k].astype(np.float64))
        scale = G * 5.0
        hip.sample_marker_covariances(t + 4.5, scale, seed=9, iteration=7, marker_offset=100)
        got = hip.marker_covariances()
        want = O.sample_marker_covariances(beta, t + 4.5, scale, 9, 7, marker0=100)
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-12)
        # df = t + 0.5: the last row's chi-square has a = 0.75 < 1 and takes the boost branch exp(log u / a)
        hip.sample_marker_covariances(t + 0.5, scale, seed=9, iteration=7, marker_offset=100)
        got = hip.marker_covariances()
        want = O.sample_marker_covariances(beta, t + 0.5, scale, 9, 7, marker0=100)
        print(f"f64 marker covariances t{t} df={t + 0.5} (boost branch): equal after rounding to float {(got.astype(np.float32) == want).mean():.4f}, "
              f"worst relative difference {np.max(np.abs(got - want) / np.abs(want)):.2e}")
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-12)
    finally:
        hip.close()


@pytest.mark.parametrize("case", ["sampler_II", "bayesb", "annotated"])
def test_runmcmc_double_precision_multitrait_gpu_vs_restatement(tmp_path, case):
    """runMCMC(double_precision=true) end to end: the Float64 device context against the same host loop on the restatement
    engine, same seed: posterior means within 1e-8."""
    out_ref, _ = run_mt_case(case, RestatementEngine64(), tmp_path / "ref")
    out_hip, _ = run_mt_case(case, None, tmp_path / "hip")
    eo, eh = out_ref["marker effects geno"], out_hip["marker effects geno"]
    np.testing.assert_allclose(eh["Estimate"].to_numpy(dtype=np.float64), eo["Estimate"].to_numpy(dtype=np.float64), atol=1e-8)
    np.testing.assert_allclose(eh["Model_Frequency"].to_numpy(dtype=np.float64), eo["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)
    for k in ("y1", "y2"):
        np.testing.assert_allclose(out_hip[f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64), out_ref[f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64), atol=1e-7)


def test_f64_refusals_stay():
    """constraint = true (MEGABAYESC / MEGABAYESB) and a float var_effect_matrix stay JWAS_HIP_EUNSUP in a Float64 context."""
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    hip, ref, R, G, rng = _pair(256, 200, 2, "MTBayesB", bs=64, seed=70)
    try:
        for mega in ("MegaBayesC", "MegaBayesB"):
            with pytest.raises(J.JwasHipError, match="constraint") as ei:
                hip.init_state(mega, 2)
            assert ei.value.code == EUNSUP
        hip.init_state("MTBayesB", 2)
        P = _lib.SweepParams()
        P.method, P.ntraits, P.nreps, P.iteration, P.seed = _lib.MTBAYESB1, 2, 1, 1, 1
        for i in range(4):
            P.vare_f64[i] = P.vare[i] = float(R.reshape(-1)[i]); P.var_effect_f64[i] = P.var_effect[i] = float(G.reshape(-1)[i])
        P.log_prior_states[3] = 0.0
        vm = np.tile(G.astype(np.float32), (200, 1, 1))
        P.var_effect_matrix = vm.ctypes.data_as(C.POINTER(C.c_float))
        S = _lib.SweepStats()
        rc = hip._L.jwas_hip_sweep(hip._h, C.byref(P), C.byref(S))
        assert rc == EUNSUP
        assert "jwas_hip_set_marker_covariances_f64" in hip._L.jwas_hip_last_error(hip._h).decode()
        with pytest.raises(J.JwasHipError) as ei:                 # (the float reader points to its _f64 namesake)
            hip._chk(hip._L.jwas_hip_get_marker_covariances(hip._h, vm.ctypes.data_as(C.c_void_p)))
        assert ei.value.code == EUNSUP
    finally:
        hip.close()
