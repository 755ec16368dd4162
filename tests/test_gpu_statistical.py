"""Tier-2 (statistical) agreement, SURVEY section 8c: chains that do NOT share arithmetic -- the device path with its
production fp32-MFMA Grams and block schedule vs the oracle's literal non-block restatement (per-marker dot / axpy) --
over several seeds.  Trajectories differ (an MCMC chain is chaotic), posterior summaries must agree within the envelope the
reference itself accepted between its Julia and R implementations (benchmarks/reports/2026-03-18-bayesr-parity-final-note.md:
75-105): residual variance <= ~1.5 %, marker variance <= ~5 %, mean model frequency abs <= ~0.01, pi abs <= ~0.02 -- or within
3 standard errors of the 5-seed comparison where the Monte-Carlo error of 5 x 500 saved iterations is wider than that."""
import numpy as np
import pandas as pd
import pytest

import draw_laws as DL
from conftest import make_dataset
from oracle_engine import OracleEngine
import jwas_jl_amd.api as api

pytestmark = pytest.mark.gpu


def _summaries(out):
    me = out["marker effects geno"]
    return {
        "vare": float(out["residual variance"]["Estimate"][0]),
        "varg": float(out["marker effects variance geno"]["Estimate"][0]),
        "pi": float(out["pi_geno"]["Estimate"][0]),
        "freq": float(me["Model_Frequency"].mean()),
        "ebv": out["EBV_y1"]["EBV"].to_numpy(),
    }


@pytest.mark.parametrize("method,Pi", [("BayesC", 0.95), ("BayesR", 0.0)])
def test_multi_seed_posterior_summaries_agree(tmp_path, method, Pi):
    d = make_dataset(n=400, p=1200, ncausal=12, seed=5, center=False)
    ids = [f"i{i}" for i in range(400)]
    gdf = pd.DataFrame(d["raw"], columns=[f"m{j}" for j in range(1200)])
    gdf.insert(0, "ID", ids)
    ph = pd.DataFrame({"ID": ids, "y1": d["y"]})
    acc = {"hip": [], "orc": []}
    for seed in (11, 22, 33, 44, 55):
        for tag, eng, kw in (("hip", None, dict(block_size=256, gram_mode="mfma")), ("orc", OracleEngine("dense"), dict(block_size=256))):
            geno = api.get_genotypes(gdf, method=method, Pi=Pi, estimatePi=True)
            model = api.build_model("y1 = intercept + geno")
            out = api.runMCMC(model, ph, chain_length=700, burnin=200, seed=seed + (1000 if tag == "orc" else 0),
                              output_folder=str(tmp_path / f"{tag}{seed}"), _engine=eng, **kw)
            if method == "BayesR":                      # pi_geno has 4 rows: use the null-class share
                out["pi_geno"] = out["pi_geno"].iloc[[0]].reset_index(drop=True)
            acc[tag].append(_summaries(out))
    keys = ("vare", "varg", "pi", "freq")
    m = {tag: {k: np.mean([s[k] for s in acc[tag]]) for k in keys} for tag in acc}
    # standard error of the difference of the two 5-seed means (the seeds of the two paths are independent)
    se = {k: np.sqrt(np.var([s[k] for s in acc["hip"]], ddof=1) / 5 + np.var([s[k] for s in acc["orc"]], ddof=1) / 5) for k in keys}
    print(method, {k: (round(m["hip"][k], 5), round(m["orc"][k], 5), round(float(se[k]), 5)) for k in keys})

    def close(k, envelope, relative):
        diff = abs(m["hip"][k] - m["orc"][k])
        scale = abs(m["orc"][k]) if relative else 1.0
        # the reference's envelope, or 3 standard errors of this short multi-seed comparison if that is wider
        return diff <= max(envelope * scale, 3.0 * se[k])
    assert close("vare", 0.015, True)
    assert close("varg", 0.055, True)
    assert close("pi", 0.02, False)
    assert close("freq", 0.01, False)
    ebv_h = np.mean([s["ebv"] for s in acc["hip"]], axis=0)
    ebv_o = np.mean([s["ebv"] for s in acc["orc"]], axis=0)
    assert np.corrcoef(ebv_h, ebv_o)[0, 1] > 0.995


@pytest.mark.parametrize("method,precision", [("BayesC", 32), ("BayesR", 32), ("BayesC", 64)], ids=["BayesC", "BayesR", "BayesC-f64"])
def test_device_chain_samples_the_exact_posterior(method, precision):
    """Oracle-independent check of WHAT the device samples: with fixed hyper-parameters and three correlated markers
    the posterior over inclusion / class states is computable exactly by enumeration (marginal likelihood of every
    state); a long device chain must visit the states with those frequencies (Monte-Carlo error ~0.01 at 30 000 sweeps).
    THE EFFECTS of every sweep after burn-in against the same enumeration (tests/draw_laws.exact_mixture_moments): every first
    and second moment within 5 standard errors (50 batch means), every standard error of a mean <= 0.02 posterior sd.  The oracle
    chain on the same data and seed (tests/test_draw_laws_host.py): deviations <= 1.7 SE, SE <= 0.0072 sd; the device: the same
    figures (its trajectories are the oracle's).  A copy of the chain whose effect sd is scaled by 1.05 misses a second moment
    by 5.003 SE (1.40 SE unscaled).  BayesC-f64: the separately written Float64 sampler."""
    import jwas_jl_amd as J
    e = J.HipEngine(0, precision=precision)
    try:
        DL.assert_st_chain(e, DL.st_chain_case(method), f"device f{precision} {method}", np.float64 if precision == 64 else np.float32)
    finally:
        e.close()


@pytest.mark.parametrize("sampler,precision", [("MTBayesC", 32), ("MTBayesC_II", 32), ("MTBayesC", 64), ("MegaBayesC", 32), ("MTBayesB", 32)],
                         ids=["MTBayesC", "MTBayesC_II", "MTBayesC-f64", "MegaBayesC", "MTBayesB"])
def test_device_multitrait_chain_samples_the_exact_posterior(sampler, precision):
    """Same for the two-trait samplers I and II: two correlated markers, 4 joint states each (16 configurations);
    vec(Y) ~ N(0, R (x) I + sum_j (D_j G_j D_j) (x) x_j x_j'), D_j = diag(delta_j) -- states and effects
    (tests/draw_laws.exact_mixture_moments_mt).  Also sampler I in a Float64 context, constraint = true (diagonal R and G, one pi
    per trait) and multi-trait BayesB with a fixed covariance per marker handed in.  Measured, device and oracle alike: deviations
    <= 2.25 SE, SE <= 0.0074 sd."""
    import jwas_jl_amd as J
    e = J.HipEngine(0, precision=precision)
    try:
        DL.assert_mt_chain(e, DL.mt_chain_case(sampler), f"device f{precision} {sampler}", np.float64 if precision == 64 else np.float32)
    finally:
        e.close()
