"""runMCMC(double_precision=true) with the multi-trait samplers beyond sampler I with one shared covariance -- sampler II, multi-trait
BayesA/B (one t x t effect covariance per marker) and marker-specific joint priors -- on the CPU:

1. the Float64 restatement (tests/f64_mt_reference.py) against the Float32 oracle (oracle/jwas_oracle.c, mt2_update / mt1_update
   with orc_set_var_effect_matrix) on Float32-rounded inputs: identical joint-state trajectories, effects within 1e-4 of their
   scale -- the restatement draws on the oracle's counter-RNG slots, so the Float64 device path can be checked against it;
2. the host loop in Float64 mode through the restatement engine for a restricted Pi (sampler II), 2-trait BayesB and annotated
   2-trait BayesC."""
import numpy as np
import pandas as pd
import pytest

import oracle as O
from conftest import make_dataset
from f64_mt_reference import RestatementEngine64, SAMPLER_I, SAMPLER_II, inv_gj, mt_block_sweep, sample_marker_covariances
from jwas_jl_amd import api


def _mt_problem(t, n, p, seed):
    d = make_dataset(n=n, p=p, ncausal=10, seed=seed)
    X32 = np.asfortranarray(d["X"])
    rng = np.random.default_rng(seed)
    y = d["y"] - d["y"].mean()
    r = np.stack([((1 + 0.3 * k) * y + 0.3 * rng.standard_normal(n)).astype(np.float32) for k in range(t)])
    A = rng.standard_normal((t, t)); B = rng.standard_normal((t, t))
    vare = ((A @ A.T / t + np.eye(t)) * 0.5).astype(np.float32)
    G = ((B @ B.T / t + np.eye(t)) * 0.01).astype(np.float32)
    return X32, r, vare, G, rng


@pytest.mark.parametrize("t,case", [(t, c) for t in (2, 3, 4) for c in ("II", "I_cov", "II_cov")] + [(2, "I_lpr"), (2, "II_lpr")])
def test_restatement_tracks_the_float32_oracle(t, case):
    n, p, sweeps = 240, 300 if t < 4 else 200, 4
    X32, r32, vare, G, rng = _mt_problem(t, n, p, seed=60 + t)
    kind = SAMPLER_II if case.startswith("II") else SAMPLER_I
    ns = 1 << t
    lp = np.log(rng.dirichlet(np.ones(ns) * 2))
    if kind == SAMPLER_II and case == "II":
        lp[1] = -np.inf                                   # a restricted support (a Pi that leaves out a joint state)
    if case.endswith("lpr"):
        lp = np.log(rng.dirichlet(np.ones(ns) * 2, size=p))
    vmat = None
    if case.endswith("cov"):
        vmat = np.stack([G * rng.uniform(0.5, 2.0) + np.diag(rng.uniform(0, 0.005, t)).astype(np.float32) for _ in range(p)]).astype(np.float32)
    a32 = np.zeros((t, p), np.float32); b32 = np.zeros((t, p), np.float32); d32 = np.ones((t, p), np.float32)
    X64 = np.asfortranarray(X32.astype(np.float64))
    a64, b64, d64, r64 = a32.astype(np.float64), b32.astype(np.float64), d32.astype(np.float64), r32.astype(np.float64)
    xpx32, xpx64 = O.xpx(X32), (X64 * X64).sum(axis=0)
    ginv = None if vmat is None else np.stack([inv_gj(g) for g in vmat.astype(np.float64)])
    O.set_var_effect_matrix(vmat)
    try:
        for it in range(1, sweeps + 1):
            O.mt_sweep(kind, X32, xpx32, r32, a32, b32, d32, vare, G, lp, 5, it)
            mt_block_sweep(kind, X64, xpx64, r64, a64, b64, d64, vare.astype(np.float64), G.astype(np.float64), lp, 5, it,
                           [0], nreps=1, ginv_mat=ginv)
            assert np.array_equal(d32 != 0, d64 != 0), f"sweep {it}: joint states differ at markers {np.flatnonzero((d32 != d64).any(axis=0))[:5]}"
            scale = max(np.abs(b32).max(), 1e-3)
            assert np.abs(a64 - a32).max() <= 1e-4 * scale, f"sweep {it}"
            assert np.abs(b64 - b32).max() <= 1e-4 * scale, f"sweep {it}"
    finally:
        O.set_var_effect_matrix(None)
    assert 0 < (d64 != 0).mean() < 1


def test_restatement_block_form_is_the_literal_chain():
    """One pass per block over any partition gives the literal per-marker chain (the device's single-pass schedule)."""
    t = 3
    X32, r32, vare, G, rng = _mt_problem(t, 200, 150, seed=71)
    X = np.asfortranarray(X32.astype(np.float64)); xpx = (X * X).sum(axis=0)
    lp = np.log(rng.dirichlet(np.ones(8)))
    runs = []
    for starts in ([0], [0, 7, 64, 65, 140]):
        a = np.zeros((t, 150)); b = np.zeros((t, 150)); d = np.ones((t, 150)); r = r32.astype(np.float64)
        for it in (1, 2):
            mt_block_sweep(SAMPLER_II, X, xpx, r, a, b, d, vare, G, lp, 3, it, starts)
        runs.append((a, d, r))
    assert np.array_equal(runs[0][1], runs[1][1])
    np.testing.assert_allclose(runs[1][0], runs[0][0], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(runs[1][2], runs[0][2], rtol=0, atol=1e-10)


def test_restatement_covariance_draws_match_the_oracle():
    """The double Bartlett draw on the oracle's counters: beta exactly representable in float32 -> the oracle's draws to float
    rounding."""
    rng = np.random.default_rng(4)
    for t in (2, 3, 4):
        beta = (rng.standard_normal((t, 50)) * 0.1).astype(np.float32)
        scale = np.eye(t) * 0.02 + 0.005
        got = sample_marker_covariances(beta.astype(np.float64), 6.5, scale, 17, 3, marker0=11)
        want = O.sample_marker_covariances(beta, 6.5, scale, 17, 3, marker0=11)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-12)


# ---- runMCMC(double_precision=true) through the restatement engine ---------------------------------------------------------
def _two_trait_data(n=160, p=120, seed=21):
    d = make_dataset(n=n, p=p, ncausal=6, seed=seed, center=False)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(d["raw"], columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    rng = np.random.default_rng(seed)
    ph = pd.DataFrame({"ID": ids, "y1": d["y"], "y2": 0.6 * d["y"] + 0.8 * rng.standard_normal(n)})
    return gdf, ph


def _mt_case(case, gdf):
    """The three Float64 models: a restricted Pi (auto -> sampler II), 2-trait BayesB, annotated 2-trait BayesC."""
    if case == "sampler_II":
        return api.get_genotypes(gdf, np.eye(2) * 0.5, method="BayesC", Pi={(0.0, 0.0): 0.8, (1.0, 1.0): 0.2},
                                 estimatePi=False, multi_trait_sampler="auto", double_precision=True), "MTBayesC_II"
    if case == "bayesb":
        return api.get_genotypes(gdf, np.eye(2) * 0.5, method="BayesB", double_precision=True), "MTBayesB"
    p = gdf.shape[1] - 1
    ann = np.zeros((p, 2)); ann[: p // 4, 0] = 1.0; ann[:, 1] = np.random.default_rng(3).standard_normal(p)
    Pi = {(0.0, 0.0): 0.85, (1.0, 0.0): 0.05, (0.0, 1.0): 0.05, (1.0, 1.0): 0.05}
    return api.get_genotypes(gdf, np.eye(2) * 0.5, method="BayesC", annotations=ann, Pi=Pi, double_precision=True), "MTBayesC"


def run_mt_case(case, engine, tmp_path, chain_length=40):
    gdf, ph = _two_trait_data()
    geno, expect = _mt_case(case, gdf)
    assert geno.genotypes.dtype == np.float64
    model = api.build_model("y1 = intercept + geno\ny2 = intercept + geno", np.eye(2))
    out = api.runMCMC(model, ph, chain_length=chain_length, burnin=10, seed=13, double_precision=True, output_folder=str(tmp_path / case),
                      _engine=engine)
    return out, expect


@pytest.mark.parametrize("case", ["sampler_II", "bayesb", "annotated"])
def test_runmcmc_double_precision_multitrait_host_loop(tmp_path, case):
    used = {}

    class Spy(RestatementEngine64):
        def init_state(self, method, ntraits=1):
            used["method"] = method
            return super().init_state(method, ntraits)

    out, expect = run_mt_case(case, Spy(), tmp_path)
    assert used["method"] == expect
    me = out["marker effects geno"]
    assert me["Estimate"].dtype == np.float64 and np.isfinite(me["Estimate"]).all()
    f1 = me[me.Trait == "y1"]["Model_Frequency"].to_numpy()
    assert 0 < f1.mean() <= 1
    if case == "sampler_II":                             # the support {00, 11}: both traits in or out together
        assert np.array_equal(f1, me[me.Trait == "y2"]["Model_Frequency"].to_numpy())
    assert np.isfinite(np.asarray(out["residual variance"]["Estimate"], dtype=np.float64)).all()
    assert np.corrcoef(out["EBV_y1"]["EBV"].to_numpy(dtype=np.float64), out["EBV_y2"]["EBV"].to_numpy(dtype=np.float64))[0, 1] > 0
