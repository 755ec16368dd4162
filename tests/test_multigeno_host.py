"""Several genotype categories in one model (jwas.jl_amd/multigeno.py) on the CPU stand-ins (tests/multigeno_reference.py): the
two-context chain against the one chain on [X1 X2], the driver against run_chain, the law against an enumerated posterior, the
defaults and the order of the reference, outputs and the contract's refusals."""
import os

import numpy as np
import pandas as pd
import pytest

import draw_laws as DL
import multigeno_reference as MR
from conftest import make_dataset
from multigeno_reference import MultiOracleEngine, MultiOracleEngine64
from oracle_engine import OracleEngine
from jwas_jl_amd import api, multigeno
from jwas_jl_amd.mcmc import genetic2marker

N, P1, P2, BS, SWEEPS = 301, 70, 50, 32, 5


def _shapes(seed=5, n=N, p1=P1, p2=P2):
    d = make_dataset(n=n, p=p1 + p2, ncausal=8, seed=seed)
    return d["X"][:, :p1], d["X"][:, p1:], d["y"] - d["y"].mean()


ST_KW = {"BayesC": dict(vare=np.float32(0.5), var_effect=np.float32(0.02), pi=0.7),
         "BayesR": dict(vare=np.float32(0.5), var_effect=np.float32(0.2), pi_classes=np.array([0.6, 0.2, 0.15, 0.05]))}
MT_R = np.array([[0.6, 0.2], [0.2, 0.5]], dtype=np.float32)
MT_G = np.array([[0.03, 0.01], [0.01, 0.02]], dtype=np.float32)
MT_KW = {"I": ("MTBayesC", np.array([0.4, 0.2, 0.15, 0.25])), "II": ("MTBayesC_II", np.array([0.4, 0.2, 0.15, 0.25])),
         "RR-BLUP": ("MTBayesC", np.array([0.0, 0.0, 0.0, 1.0]))}


def _chain_pair(method, t, kw, Y, offset2=P1):
    """SWEEPS sweeps of two engines chained through the residual and of one engine on [X1 X2] with a block start at p1."""
    X1, X2, _ = _shapes()
    one, e1, e2 = OracleEngine("block"), MultiOracleEngine("block"), MultiOracleEngine("block")
    one.load_dense(np.hstack([X1, X2]))
    one.setup_blocks_explicit(np.array([0, 32, 64, 70, 102]))
    for e, X in ((e1, X1), (e2, X2)):
        e.load_dense(X)
        e.setup_blocks(BS)
    for e in (one, e1, e2):
        e.init_state(method, t)
        for k in range(t):                       # (every marker starts in the model, as in the driver)
            e.set_state(k, delta=np.ones(e.p, dtype=np.int32 if method == "BayesR" else np.float32))
    for k in range(t):
        one.set_residual(Y[k], k)
        e1.set_residual(Y[k], k)
    owner = e1
    for it in range(1, SWEEPS + 1):
        one.sweep(iteration=it, seed=3, **kw)
        for e, off_ in ((e1, 0), (e2, offset2)):
            if e is not owner:
                e.residual_handover(owner)
                owner = e
            e.sweep(iteration=it, seed=3, marker_offset=off_, **kw)
    return one, e1, e2


# ---- 1. concatenation, engine level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["BayesC", "BayesR"])
def test_two_chained_engines_are_one_engine_on_the_concatenation(method):
    _, _, y = _shapes()
    one, e1, e2 = _chain_pair(method, 1, ST_KW[method], y[None])
    a, _, d = one.get_state()
    a1, _, d1 = e1.get_state()
    a2, _, d2 = e2.get_state()
    assert np.any(a1 != 0) and np.any(a2 != 0)
    assert np.array_equal(a, np.concatenate([a1, a2])) and np.array_equal(d, np.concatenate([d1, d2]))
    assert np.array_equal(one.get_residual(), e2.get_residual())
    # a driver that forgets the offset reuses category 1's counters: another chain, not a rounding difference
    _, _, w2 = _chain_pair(method, 1, ST_KW[method], y[None], offset2=0)
    assert not np.array_equal(w2.get_state()[0], a2)


# ---- 5a. the same for two traits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["I", "II", "RR-BLUP"])
def test_two_chained_engines_are_one_engine_multi_trait(sampler):
    X1, X2, y = _shapes()
    rng = np.random.default_rng(8)
    Y = np.stack([y, (0.5 * y + 0.7 * rng.standard_normal(N)).astype(np.float32)])
    Y -= Y.mean(axis=1, keepdims=True)
    method, prior = MT_KW[sampler]
    with np.errstate(divide="ignore"):
        kw = dict(vare=MT_R, var_effect=MT_G, log_prior_states=np.log(prior))
    one, e1, e2 = _chain_pair(method, 2, kw, Y)
    for k in range(2):
        a, b, d = one.get_state(k)
        assert np.any(a != 0)
        assert np.array_equal(a, np.concatenate([e1.get_state(k)[0], e2.get_state(k)[0]]))
        assert np.array_equal(d, np.concatenate([e1.get_state(k)[2], e2.get_state(k)[2]]))
        assert np.array_equal(one.get_residual(k), e2.get_residual(k))


# ---- data for the runMCMC tests ----------------------------------------------------------------------------------------------------
def _frames(n=120, p1=64, p2=50, seed=17, traits=1):
    d = make_dataset(n=n, p=p1 + p2, ncausal=6, seed=seed, center=False)
    ids = [f"i{i}" for i in range(n)]
    cols = [f"m{j}" for j in range(p1 + p2)]
    gdf = pd.DataFrame(d["raw"], columns=cols)
    gdf.insert(0, "ID", ids)
    g1, g2 = gdf[["ID"] + cols[:p1]], gdf[["ID"] + cols[p1:]]
    rng = np.random.default_rng(seed + 1)
    ph = pd.DataFrame({"ID": ids, "y1": d["y"], "x1": rng.standard_normal(n)})
    for k in range(1, traits):
        ph[f"y{k + 1}"] = (0.6 * d["y"] + rng.standard_normal(n)).astype(np.float32)
    return gdf, g1, g2, ph


def _two(g1, g2, kw1, kw2=None, G1=False, G2=False):
    kw2 = kw1 if kw2 is None else kw2
    geno1 = api.get_genotypes(g1, G1, quality_control=False, **kw1)
    geno2 = api.get_genotypes(g2, G2, quality_control=False, **kw2)
    return geno1, geno2


# ---- 2. concatenation through runMCMC ----------------------------------------------------------------------------------------------
def test_runmcmc_two_categories_equal_the_single_category_chain(tmp_path):
    """No place was found where run_chain consumes the host generator differently from the two-category chain when pi and the
    marker-effect variances are fixed: location parameters, then the residual variance, in both."""
    gdf, g1, g2, ph = _frames()
    kw = dict(method="BayesC", Pi=0.7, estimatePi=False, G_is_marker_variance=True, estimate_variance=False)
    geno = api.get_genotypes(gdf, 0.02, quality_control=False, **kw)
    model = api.build_model("y1 = intercept + x1 + geno")
    api.set_covariate(model, "x1")
    one = api.runMCMC(model, ph, chain_length=30, burnin=5, seed=9, output_folder=str(tmp_path / "one"), _engine=OracleEngine("block"),
                      block_size=32)
    geno1, geno2 = _two(g1, g2, kw, G1=0.02, G2=0.02)
    model = api.build_model("y1 = intercept + x1 + geno1 + geno2")
    api.set_covariate(model, "x1")
    two = api.runMCMC(model, ph, chain_length=30, burnin=5, seed=9, output_folder=str(tmp_path / "two"),
                      _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")], block_size=32)
    me = pd.concat([two["marker effects geno1"], two["marker effects geno2"]], ignore_index=True)
    assert np.any(one["marker effects geno"]["Estimate"].to_numpy() != 0)
    for col in ("Estimate", "Model_Frequency"):
        assert np.array_equal(me[col].to_numpy(), one["marker effects geno"][col].to_numpy()), col
    assert list(me["Marker_ID"]) == list(one["marker effects geno"]["Marker_ID"])
    assert two["residual variance"].equals(one["residual variance"])
    assert two["location parameters"].equals(one["location parameters"])
    e1, e2 = one["EBV_y1"]["EBV"].to_numpy(), two["EBV_y1"]["EBV"].to_numpy()
    bound = 4 * 2.0 ** -24 * np.abs(e1).max()
    print(f"EBV: two products summed vs one: max difference {np.abs(e1 - e2).max():.3e} (bound {bound:.3e})")
    assert np.abs(e1 - e2).max() <= bound


# ---- 3. the law, independent of the oracle -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def law_case():
    case = MR.two_category_case()
    X = np.hstack([case["X1"], case["X2"]])
    return case, MR.exact_marker_mixture_moments(X, case["y"], case["vare"], case["class_vars"], case["class_probs"])


def assert_two_category_law(make_engine, law_case, sweeps, tag, dtype=np.float32):
    """The acceptance of draw_laws.assert_st_chain for the two-category chain, and its rejection of the chain that gives category 2
    category 1's prior."""
    case, (exact, Ea, Eaa) = law_case
    assert len(exact) == 64
    figs = {}
    for wrong in (False, True):
        counts, alphas = MR.run_two_category_chain(make_engine(), make_engine(), case, sweeps, DL.CHAIN_BURN, dtype, wrong_prior=wrong)
        m = figs[wrong] = MR.chain_figures(counts, alphas, exact, Ea, Eaa)
        print(f"two-category law {tag} ({'category 2 with the prior of category 1' if wrong else 'own priors'}): worst state frequency "
              f"difference {m['freq']:.4f} (bound 0.02), means within {m['dev1']:.2f} SE, second moments within {m['dev2']:.2f} SE (bound 5), "
              f"worst SE {m['se_sd']:.4f} of the posterior sd (bound 0.02); N {len(alphas)}")
    assert MR.figures_pass(figs[False]), figs[False]
    assert not MR.figures_pass(figs[True]), figs[True]


def test_two_category_chain_has_the_enumerated_law(law_case):
    assert_two_category_law(lambda: MultiOracleEngine("block"), law_case, DL.CHAIN_SWEEPS, "oracle")


def test_two_category_law_short_chain_keeps_the_standard_errors(law_case):
    """The device test may run 10 000 sweeps: the SE bound holds at that length too."""
    case, (exact, Ea, Eaa) = law_case
    counts, alphas = MR.run_two_category_chain(MultiOracleEngine("block"), MultiOracleEngine("block"), case, 10_000, DL.CHAIN_BURN)
    m = MR.chain_figures(counts, alphas, exact, Ea, Eaa)
    print(f"two-category law, 10 000 sweeps: {m}")
    assert MR.figures_pass(m), m


# ---- 4. defaults and order -----------------------------------------------------------------------------------------------------------
def test_defaults_per_category_and_the_order_of_the_reference(tmp_path, monkeypatch):
    _, g1, g2, ph = _frames()
    geno1, geno2 = _two(g1, g2, dict(method="BayesC", Pi=0.8), dict(method="BayesR"))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    assert [Mi.name for Mi in model.M] == ["geno1", "geno2"]
    log = []
    engines = [MultiOracleEngine("block", log, "geno1"), MultiOracleEngine("block", log, "geno2")]
    default_rng = np.random.default_rng

    class Rng:                                   # the one host generator, with the order of its draws recorded
        def __init__(self, seed):
            self._g = default_rng(seed)

        def __getattr__(self, name):
            f = getattr(self._g, name)

            def wrapped(*a, **k):
                log.append(("draw", name))
                return f(*a, **k)
            return wrapped
    monkeypatch.setattr(np.random, "default_rng", Rng)
    out = api.runMCMC(model, ph, chain_length=3, seed=4, output_folder=str(tmp_path / "o"), _engine=engines)
    monkeypatch.undo()
    vary = float(np.var(ph["y1"].to_numpy(dtype=np.float32).astype(np.float64), ddof=1))
    for Mi in model.M:                           # varg = var(y) / 2 / C (input_data_validation.jl:301-327)
        assert Mi.genetic_variance.val == pytest.approx(vary * 0.5 / 2, rel=1e-12)
    assert float(model.R.val) == pytest.approx(vary * 0.5, rel=1e-6)
    # genetic2marker per category: its own sum2pq and pi (tools4genotypes.jl:426-478), its own scale (:414-418)
    G1 = vary * 0.25 / ((1 - 0.8) * geno1.sum2pq)
    G2 = vary * 0.25 / (geno2.sum2pq * float((MR.GAMMA * api.BAYESR_DEFAULT_PI).sum()))
    assert geno1.G.val == pytest.approx(G1, rel=1e-12) and geno2.G.val == pytest.approx(G2, rel=1e-12)
    assert geno1.G.val == genetic2marker(geno1, 0.8, "BayesC") and geno2.G.val == genetic2marker(geno2, api.BAYESR_DEFAULT_PI, "BayesR")
    assert geno1.G.scale == pytest.approx(G1 * 2 / 4) and geno2.G.scale == pytest.approx(G2 * 2 / 4)
    # per iteration: the intercept's normal, [hand-over to 1,] sweep 1 at offset 0, beta (pi 1), chisquare (variance 1), hand-over to 2,
    # sweep 2 at offset p1, dirichlet (pi 2), chisquare (variance 2), chisquare (residual variance)
    it1 = [("get_residual", "geno1"), ("draw", "standard_normal"), ("sweep", "geno1", 0), ("draw", "beta"), ("draw", "chisquare"),
           ("handover", "geno2", "geno1"), ("sweep", "geno2", 64), ("draw", "dirichlet"), ("draw", "chisquare"), ("draw", "chisquare")]
    it2 = [("get_residual", "geno2"), ("draw", "standard_normal"), ("handover", "geno1", "geno2")] + it1[2:]
    assert log[:len(it1)] == it1
    assert log[len(it1):len(it1) + len(it2)] == it2
    assert out["_timing"]["marker_offset"] == [0, 64]
    # nothing reads a residual from an engine that does not own it
    owner = "geno1"
    for e in log:
        if e[0] == "handover":
            assert e[2] == owner
            owner = e[1]
        elif e[0] in ("sweep", "get_residual"):
            assert e[1] == owner, e


# ---- 5b. three traits, two categories ------------------------------------------------------------------------------------------------
def test_runmcmc_three_traits_two_categories(tmp_path):
    _, g1, g2, ph = _frames(traits=3)
    geno1, geno2 = _two(g1, g2, dict(method="BayesC"), dict(method="RR-BLUP"))
    geno1.multi_trait_sampler = "II"
    model = api.build_model("y1 = intercept + x1 + geno1 + geno2\ny2 = intercept + geno1 + geno2\ny3 = intercept + geno1 + geno2")
    api.set_covariate(model, "x1")
    folder = str(tmp_path / "o")
    out = api.runMCMC(model, ph, chain_length=12, burnin=2, seed=5, output_folder=folder,
                      _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")], block_size=32)
    assert len(out["marker effects geno1"]) == 3 * 64 and len(out["marker effects geno2"]) == 3 * 50
    assert list(out["marker effects geno1"]["Trait"].unique()) == ["y1", "y2", "y3"]
    assert len(out["pi_geno1"]) == 8 and "pi_geno2" not in out          # RR-BLUP: estimatePi = false
    assert np.all(out["marker effects geno2"]["Model_Frequency"] == 1.0)
    for key in ("residual variance", "marker effects variance geno1", "marker effects variance geno2", "genetic_variance"):
        assert len(out[key]) == 9 and np.all(np.isfinite(out[key]["Estimate"]))
    assert len(out["heritability"]) == 3 and len(out["location parameters"]) == 4
    for tr in ("y1", "y2", "y3"):
        assert len(out[f"EBV_{tr}"]) == 120 and np.all(np.isfinite(out[f"EBV_{tr}"]["EBV"]))
        assert os.path.exists(os.path.join(folder, f"MCMC_samples_marker_effects_geno2_{tr}.txt"))


# ---- 6. outputs and contract ---------------------------------------------------------------------------------------------------------
def mixed_model(g1, g2):
    """BayesB + RR-BLUP: the mixed model of the output test and of the device's end-to-end test."""
    geno1, geno2 = _two(g1, g2, dict(method="BayesB", Pi=0.9), dict(method="RR-BLUP"))
    model = api.build_model("y1 = intercept + x1 + geno1 + geno2")
    api.set_covariate(model, "x1")
    return model


def test_outputs_tables_and_files_mixed_methods(tmp_path):
    _, g1, g2, ph = _frames()
    folder = str(tmp_path / "o")
    out = api.runMCMC(mixed_model(g1, g2), ph, chain_length=20, burnin=4, seed=6, output_folder=folder,
                      _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")])
    for key in ("marker effects geno1", "marker effects geno2", "pi_geno1", "marker effects variance geno2", "EBV_y1", "genetic_variance",
                "heritability", "residual variance", "location parameters"):
        assert key in out, key
    assert "pi_geno2" not in out and "marker effects variance geno1" not in out      # RR-BLUP has no pi, BayesB no common variance
    assert len([k for k in out if k.startswith("EBV_")]) == 1
    for f in ("MCMC_samples_marker_effects_geno1_y1.txt", "MCMC_samples_marker_effects_geno2_y1.txt", "MCMC_samples_pi_geno1.txt",
              "MCMC_samples_marker_effects_variances_geno2.txt", "MCMC_samples_residual_variance.txt", "MCMC_samples_genetic_variance.txt",
              "MCMC_samples_heritability.txt", "marker_effects_geno1.txt", "marker_effects_geno2.txt", "pi_geno1.txt", "EBV_y1.txt",
              "IDs_for_individuals_with_genotypes.txt"):
        assert os.path.exists(os.path.join(folder, f)), f
    rows = open(os.path.join(folder, "MCMC_samples_marker_effects_geno2_y1.txt")).read().splitlines()
    assert len(rows) == 1 + 16 and len(rows[0].split(",")) == 50
    # the EBV is the sum over the categories of X_i times the posterior mean effects (a linear map of the running means)
    want = model_matrix(g1) @ out["marker effects geno1"]["Estimate"].to_numpy(dtype=np.float64) + model_matrix(g2) @ out["marker effects geno2"]["Estimate"].to_numpy(dtype=np.float64)
    np.testing.assert_allclose(out["EBV_y1"]["EBV"], want, atol=2e-5)
    assert np.all(out["marker effects geno2"]["Model_Frequency"] == 1.0) and out["marker effects geno1"]["Model_Frequency"].min() < 1.0


def model_matrix(g):
    X = g.iloc[:, 1:].to_numpy(dtype=np.float32)
    return (X - X.mean(axis=0, dtype=np.float32)).astype(np.float64)


def test_packed_and_dense_pair_equals_the_dense_pair(tmp_path):
    from jwas_jl_amd import streaming as S
    _, g1, g2, ph = _frames()
    prefix = S.prepare_streaming_genotypes(g1.iloc[:, 1:].to_numpy(dtype=np.float64), tmp_path / "st", obs_ids=list(g1["ID"]),
                                           marker_ids=list(g1.columns[1:]), quality_control=False)
    outs = {}
    for tag in ("dense", "stream"):
        geno1 = (api.get_genotypes(g1, method="BayesC", Pi=0.8, quality_control=False) if tag == "dense" else
                 api.get_genotypes(prefix, method="BayesC", Pi=0.8, storage="stream"))
        geno2 = api.get_genotypes(g2, method="BayesR", quality_control=False)
        assert geno1.nMarkers == 64
        model = api.build_model("y1 = intercept + geno1 + geno2")
        outs[tag] = api.runMCMC(model, ph, chain_length=15, burnin=3, seed=8, output_folder=str(tmp_path / tag),
                                _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")], block_size=32)
    for key in ("marker effects geno1", "marker effects geno2"):
        np.testing.assert_allclose(outs["stream"][key]["Estimate"], outs["dense"][key]["Estimate"], atol=1e-4)
    # stream needs the exact ID order for the whole model
    geno1 = api.get_genotypes(prefix, method="BayesC", Pi=0.8, storage="stream")
    geno2 = api.get_genotypes(g2, method="BayesR", quality_control=False)
    model = api.build_model("y1 = intercept + geno1 + geno2")
    with pytest.raises(ValueError, match="exact genotype/phenotype ID match"):
        api.runMCMC(model, ph.iloc[::-1], chain_length=3, output_folder=str(tmp_path / "rev"),
                    _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")])


def test_double_precision_two_categories(tmp_path):
    _, g1, g2, ph = _frames()
    geno1, geno2 = _two(g1, g2, dict(method="BayesC", Pi=0.8, double_precision=True), dict(method="BayesR", double_precision=True))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    out = api.runMCMC(model, ph, chain_length=15, burnin=3, seed=8, double_precision=True, output_folder=str(tmp_path / "o"),
                      _engine=[MultiOracleEngine64(), MultiOracleEngine64()])
    assert out["marker effects geno1"]["Estimate"].dtype == np.float64 and np.any(out["marker effects geno2"]["Estimate"] != 0)
    geno1, geno2 = _two(g1, g2, dict(method="BayesC", double_precision=True), dict(method="BayesC"))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    for dp in (True, False):
        with pytest.raises(NotImplementedError, match="Float64"):
            api.runMCMC(model, ph, chain_length=3, double_precision=dp, output_folder=str(tmp_path / "bad"),
                        _engine=[MultiOracleEngine64(), MultiOracleEngine64()])


def test_heterogeneous_residuals_reach_every_context(tmp_path):
    _, g1, g2, ph = _frames()
    ph = ph.assign(weights=np.random.default_rng(2).uniform(0.5, 2.0, len(ph)))
    geno1, geno2 = _two(g1, g2, dict(method="BayesC", Pi=0.8))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    engines = [MultiOracleEngine("block"), MultiOracleEngine("block")]
    out = api.runMCMC(model, ph, chain_length=10, burnin=2, seed=8, heterogeneous_residuals=True, output_folder=str(tmp_path / "o"),
                      _engine=engines)
    want = (1.0 / ph["weights"].to_numpy(dtype=np.float64)).astype(np.float32)
    for e in engines:
        assert np.array_equal(e._rinv, want)
    assert np.all(np.isfinite(out["EBV_y1"]["EBV"]))


def test_output_ebv_id_list_and_ungenotyped_phenotypes(tmp_path, capsys):
    _, g1, g2, ph = _frames()
    geno1, geno2 = _two(g1, g2, dict(method="BayesC", Pi=0.8))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    ids = ["i7", "i3", "i100"]
    api.outputEBV(model, ids)
    ph2 = pd.concat([ph.iloc[:100], pd.DataFrame({"ID": ["nobody"], "y1": [0.3], "x1": [0.0]})], ignore_index=True)
    out = api.runMCMC(model, ph2, chain_length=10, burnin=2, seed=8, output_folder=str(tmp_path / "o"),
                      _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")])
    assert "1 phenotyped individuals are not genotyped" in capsys.readouterr().out
    assert list(out["EBV_y1"]["ID"]) == ids
    rows = [7, 3, 100]
    want = (model_matrix(g1)[rows] @ out["marker effects geno1"]["Estimate"].to_numpy(dtype=np.float64)
            + model_matrix(g2)[rows] @ out["marker effects geno2"]["Estimate"].to_numpy(dtype=np.float64))
    np.testing.assert_allclose(out["EBV_y1"]["EBV"], want, atol=2e-5)


def test_categories_must_hold_the_same_individuals(tmp_path):
    _, g1, g2, ph = _frames()
    geno1, geno2 = _two(g1, g2.iloc[::-1], dict(method="BayesC"))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    with pytest.raises(ValueError, match="genotypic information is not provided for same individuals"):
        api.runMCMC(model, ph, chain_length=3, output_folder=str(tmp_path / "o"), _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")])
    assert not os.path.exists(tmp_path / "o")


def _refusal_cases():
    def plain(g1, g2, ph):
        geno1, geno2 = _two(g1, g2, dict(method="BayesC"))
        return api.build_model("y1 = intercept + geno1 + geno2"), ph, {}

    def with_(**kw):
        return lambda g1, g2, ph: plain(g1, g2, ph)[:2] + (kw,)

    def set_random(g1, g2, ph):
        geno1, geno2 = _two(g1, g2, dict(method="BayesC"))
        model = api.build_model("y1 = intercept + herd + geno1 + geno2")
        api.set_random(model, "herd")
        return model, ph.assign(herd=[f"h{i % 5}" for i in range(len(ph))]), {}

    def categorical(g1, g2, ph):
        geno1, geno2 = _two(g1, g2, dict(method="BayesC"))
        model = api.build_model("y1 = intercept + geno1 + geno2", categorical_trait=["y1"])
        return model, ph.assign(y1=(ph["y1"] > ph["y1"].median()).astype(float) + 1.0), {}

    def censored(g1, g2, ph):
        geno1, geno2 = _two(g1, g2, dict(method="BayesC"))
        model = api.build_model("y1 = intercept + geno1 + geno2", censored_trait=["y1"])
        return model, ph.assign(y1_l=ph["y1"] - 1.0, y1_u=ph["y1"] + 1.0), {}

    def two_traits(kw1, kw2=None, **run):
        def make(g1, g2, ph):
            geno1, geno2 = _two(g1, g2, kw1, kw2)
            model = api.build_model("y1 = intercept + geno1 + geno2\ny2 = intercept + geno1 + geno2")
            return model, ph.assign(y2=ph["y1"] * 0.5 + ph["x1"]), run
        return make

    def missing_traits(g1, g2, ph):
        model, ph, _ = two_traits(dict(method="BayesC"))(g1, g2, ph)
        ph = ph.copy()
        ph.loc[3, "y2"] = np.nan
        return model, ph, {}

    def annotations(g1, g2, ph):
        ann = np.random.default_rng(1).integers(0, 2, size=(64, 2)).astype(float)
        geno1 = api.get_genotypes(g1, method="BayesC", Pi=0.5, quality_control=False, annotations=ann)
        geno2 = api.get_genotypes(g2, method="BayesC", quality_control=False)
        return api.build_model("y1 = intercept + geno1 + geno2"), ph, {}

    def marker_start(g1, g2, ph):
        geno1 = api.get_genotypes(g1, method="BayesC", quality_control=False, starting_value=np.zeros(64))
        geno2 = api.get_genotypes(g2, method="BayesC", quality_control=False)
        return api.build_model("y1 = intercept + geno1 + geno2"), ph, {}

    def device_genotypes(g1, g2, ph):
        eng = MultiOracleEngine("block")
        eng.load_dense(model_matrix(g1).astype(np.float32))
        eng.setup_blocks(32)
        geno1 = api.device_genotypes(eng, method="BayesC", obsID=list(g1["ID"]))
        geno2 = api.get_genotypes(g2, method="BayesC", quality_control=False)
        return api.build_model("y1 = intercept + geno1 + geno2"), ph, {}

    class Sharded(MultiOracleEngine):
        def comm_info(self):
            return 0, 2

    return {
        "fast_blocks": (with_(fast_blocks=True), "fast_blocks"),
        "independent_blocks": (with_(fast_blocks=True, independent_blocks=True), "independent_blocks"),
        "location_parameters": (with_(location_parameters="device"), 'location_parameters="device"'),
        "set_random": (set_random, "set_random"),
        "categorical": (categorical, "categorical or censored"),
        "censored": (censored, "categorical or censored"),
        "causal_structure": (two_traits(dict(method="BayesC"), causal_structure=np.array([[0, 0], [1, 0]])), "causal_structure"),
        "RRM": (with_(RRM=api.generatefullPhi([1, 2, 3], 2)), "RRM"),
        "annotations": (annotations, "annotations"),
        "marker_start": (marker_start, "starting values"),
        "start": (with_(starting_value=True), "starting values"),
        "constraint": (two_traits(dict(method="BayesC", constraint=True)), "constraint=true"),
        "mt_bayesb": (two_traits(dict(method="BayesC"), dict(method="BayesB")), "multi-trait BayesB"),
        "mt_bayesa": (two_traits(dict(method="BayesA")), "multi-trait BayesA"),
        "mt_bayesl": (two_traits(dict(method="BayesL")), "multi-trait BayesL"),
        "missing_traits": (missing_traits, "missing traits"),
        "device_genotypes": (device_genotypes, "device_genotypes"),
        "shards": (with_(_engine=[Sharded("block"), Sharded("block")]), "marker shards"),
    }


REFUSALS = _refusal_cases()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_out_of_scope_features_raise_before_any_device_work(tmp_path, case):
    _, g1, g2, ph = _frames()
    make, words = REFUSALS[case]
    model, ph, kw = make(g1, g2, ph)
    log = []
    engines = kw.pop("_engine", None) or [MultiOracleEngine("block", log, "a"), MultiOracleEngine("block", log, "b")]
    with pytest.raises(NotImplementedError, match=words.replace("(", r"\(").replace(")", r"\)")):
        api.runMCMC(model, ph, chain_length=3, output_folder=str(tmp_path / "o"), _engine=engines, **kw)
    assert log == [] and all(e.n == 0 for e in engines) and not os.path.exists(tmp_path / "o")


def test_engine_list_and_memory_guard(tmp_path):
    _, g1, g2, ph = _frames()
    geno1, geno2 = _two(g1, g2, dict(method="BayesC", Pi=0.8))
    model = api.build_model("y1 = intercept + geno1 + geno2")
    for bad in (MultiOracleEngine("block"), [MultiOracleEngine("block")]):
        with pytest.raises(ValueError, match="one engine per genotype category"):
            api.runMCMC(model, ph, chain_length=3, output_folder=str(tmp_path / "o"), _engine=bad)
    one = MultiOracleEngine("block")
    with pytest.raises(ValueError, match="engine of its own"):
        api.runMCMC(model, ph, chain_length=3, output_folder=str(tmp_path / "o"), _engine=[one, one])
    with pytest.raises(NotImplementedError, match="residual_handover"):
        api.runMCMC(model, ph, chain_length=3, output_folder=str(tmp_path / "o"), _engine=[OracleEngine("block"), OracleEngine("block")])
    engines = [MultiOracleEngine("block"), MultiOracleEngine("block")]
    engines[0].hbm_free = 50_000                 # less than the two contexts need together
    with pytest.raises(MemoryError, match=r"marker path needs .* GB of HBM, more than 0.80 x free"):
        api.runMCMC(model, ph, chain_length=3, output_folder=str(tmp_path / "m"), _engine=engines)
    assert engines[0].n == 0 and engines[1].n == 0
    cats = [type("C", (), dict(p=64, block_size=64, stream=False)), type("C", (), dict(p=50, block_size=64, stream=True))]
    from jwas_jl_amd import HipEngine
    assert multigeno.memory_need(cats, 120, 1, False, 0) == HipEngine.estimate_bytes(120, 64, 1, 64) + HipEngine.estimate_bytes(120, 50, 1, 64, "stream")
    assert multigeno.memory_need(cats, 120, 1, False, 3) - multigeno.memory_need(cats, 120, 1, False, 0) == 4 * 256 * (64 + 50)


def test_build_model_orders_categories_by_first_appearance():
    _, g1, g2, ph = _frames()
    b, a = _two(g1, g2, dict(method="BayesC"))
    model = api.build_model("y1 = intercept + b + a\ny2 = intercept + a + b")
    assert [Mi.name for Mi in model.M] == ["b", "a"] and all(Mi.ntraits == 2 for Mi in model.M)
    assert model.M[0].G.df == 6.0 and model.M[1].G.df == 6.0


def test_default_block_size_is_run_chains():
    f = multigeno.default_block_size
    assert f("BayesC", 1, 0.95, 5000, True, False) == 512 and f("BayesC", 1, 0.2, 5000, True, False) == 128
    assert f("BayesC", 1, 0.0, 5000, False, False) == 512 and f("BayesC", 1, 0.0, 5000, True, False) == 128
    assert f("BayesR", 1, np.array([0.95, 0.03, 0.015, 0.005]), 300, True, False) == 256
    assert f("BayesC", 2, np.array([0, 0, 0, 1.0]), 5000, True, False) == 256 and f("BayesC", 1, 0.9, 50, True, False) == 64
    assert f("BayesC", 1, 0.2, 5000, True, True) == 512
