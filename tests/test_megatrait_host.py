"""runMCMC on models of more than 4 traits (constraint=true, megatrait.py) on the CPU stand-in (tests/mega_reference.py): the routing
rule, every refusal of the contract, the priors, one pi per trait, the driver's outputs, missing cells, outputEBV and the seed."""
import contextlib
import io
import os

import numpy as np
import pytest

import mega_reference as MR
from mega_reference import MegaStandInEngine

TRAITS6 = [f"y{k + 1}" for k in range(6)]


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------
def test_block_form_is_the_marker_by_marker_chain():
    """n = 301, p = 100, 9 traits (pi 0, 0.5, 0.95 in turn), three sweeps with shared draws: blocks of 1, 40 and p choose the indicators
    of the plain chain; effects and residuals agree within 1e-11 relative."""
    cs = MR.case_traits(MR.make_case(), 9)

    def run(bs):
        R, a, b, d = cs.R.copy(), cs.alpha.copy(), cs.beta.copy(), cs.delta.copy()
        out = []
        for it in (1, 2, 3):
            kw = dict(iteration=it, seed=5, vare=cs.vare, var_effect=cs.v, pi=cs.pi, min_margin=MR.MIN_MARGIN)
            r = MR.sweep_plain(cs.X, R, a, b, d, **kw) if bs is None else MR.sweep_blocked(cs.X, R, a, b, d, block_size=bs, **kw)
            out.append((d.copy(), a.copy(), b.copy(), R.copy(), r))
        return out
    ref = run(None)
    assert all(o[4].n_changed.min() > 0 for o in ref) and not np.array_equal(ref[0][0], ref[1][0])
    assert np.all(ref[0][0][0] == 1.0) and 0 < ref[0][0][1].mean() < 1      # pi = 0 includes every marker, pi = 0.5 does not
    for bs in (1, 40, cs.p):
        for (d0, a0, b0, r0, s0), (d1, a1, b1, r1, s1) in zip(ref, run(bs)):
            assert np.array_equal(d0, d1)
            da, db, dr = (np.abs(x - y).max() / np.abs(x).max() for x, y in ((a0, a1), (b0, b1), (r0, r1)))
            print(f"blocks of {bs}: alpha {da:.2e}, beta {db:.2e}, residual {dr:.2e} relative")
            assert max(da, db, dr) <= 1e-11
            assert np.array_equal(s0.sum_delta, s1.sum_delta) and np.array_equal(s0.n_changed, s1.n_changed)


def test_no_decision_uniform_of_the_gpu_cases_is_near_its_threshold():
    """The chains tests/test_gpu_megatrait.py compares indicators with: all 64 traits, iterations 1 and 2 in blocks of 40, and the
    tight-prior sweeps of the three block sizes.  reference_sweep asserts the 1e-9 margin; the seed is the GPU tests'."""
    cs = MR.make_case()
    for it in (1, 2):
        r = MR.reference_sweep(cs, 64, it, 5, 40)
        print(f"iteration {it}: nearest threshold {r.margins.min():.2e}")
        assert r.margins.min() >= MR.MIN_MARGIN
    for bs in (1, 40, 100):
        assert MR.reference_sweep(cs, 9, 1, 5, bs, vscale=0.01).margins.min() >= MR.MIN_MARGIN


def test_trait_k_does_not_depend_on_the_number_of_traits():
    """Trait k of a T-trait sweep draws what trait 0 of a one-trait sweep with first_trait = k draws."""
    cs = MR.make_case()
    j = np.arange(cs.p)
    assert np.array_equal(MR.draws(cs.p, 17, 1, 5)[0][8], MR.mega_uniform(j, 1, 5, 8)) and np.array_equal(MR.draws(cs.p, 1, 1, 5, 8)[1][0], MR.mega_normal(j, 1, 5, 8))
    full = MR.reference_sweep(cs, 17, 1, 5, 40)
    for k in (0, 8, 16):
        c = MR.case_traits(cs, 1, k)
        MR.sweep_blocked(c.X, c.R, c.alpha, c.beta, c.delta, block_size=40, iteration=1, seed=5, vare=c.vare, var_effect=c.v, pi=c.pi, first_trait=k)
        # (numpy's matrix products change their summation order with the shape, so the values agree to rounding here; on the device
        # they are equal bit for bit, tests/test_gpu_megatrait.py)
        assert np.array_equal(c.delta[0], full.delta[k])
        np.testing.assert_allclose(c.beta[0], full.beta[k], rtol=0, atol=1e-12 * np.abs(full.beta[k]).max())
        np.testing.assert_allclose(c.R[0], full.R[k], rtol=0, atol=1e-12 * np.abs(full.R[k]).max())
    assert not np.array_equal(full.beta[1], full.beta[4])                   # (both pi = 0.5)


def test_one_marker_draws_follow_the_closed_form_posterior():
    case = MR.conditional_case()
    prob, _, _ = MR.conditional_posterior(case)
    assert prob.min() > 0.1 and prob.max() < 0.9                           # both indicators are visited a few hundred times
    rows = MR.conditional_check(MR.conditional_engine(MegaStandInEngine(64), case), case)
    for k, zf, zm1, zv1, zm0, zv0 in rows:
        print(f"trait {k}: frequency {zf:.2f} se from P = {prob[k]:.4f}; beta | 1: mean {zm1:.2f}, variance {zv1:.2f}; beta | 0: mean {zm0:.2f}, variance {zv0:.2f}")
    assert len(rows) == 3 and max(max(r[1:]) for r in rows) <= 5.0


def test_imputation_law_and_observed_cells():
    cs = MR.make_case()
    R = cs.R.copy()
    MR.impute(R, cs.missing, iteration=3, seed=5, vare=cs.vare)
    assert np.array_equal(R[~cs.missing], cs.R[~cs.missing]) and not np.any(R[cs.missing] == cs.R[cs.missing])
    z = R[cs.missing] / np.sqrt(np.broadcast_to(cs.vare[:, None], R.shape)[cs.missing])
    m = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(m) and abs(z.var(ddof=1) - 1.0) <= 5 * np.sqrt(2.0 / (m - 1))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def mega_data(n=60, p=48, t=6, seed=3, nph=None, missing=0.15):
    """(genotype frame, phenotype frame in shuffled order): t traits with ~15 % of the cells missing (y1 complete)."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    ids = [f"i{i}" for i in range(n)]
    raw = rng.binomial(2, rng.uniform(0.15, 0.85, p), size=(n, p)).astype(np.float64)
    gdf = pd.DataFrame(raw, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    Xc = raw - raw.mean(axis=0)
    a = np.zeros((p, t))
    a[rng.choice(p, 8, replace=False)] = 0.4 * rng.standard_normal((8, t))
    age = rng.uniform(1, 3, n)
    Y = 1.0 + 0.3 * age[:, None] + Xc @ a + 0.6 * rng.standard_normal((n, t))
    miss = rng.random((n, t)) < missing
    miss[:, 0] = False
    Y[miss] = np.nan
    ph = pd.DataFrame(Y, columns=[f"y{k + 1}" for k in range(t)])
    ph.insert(0, "ID", ids)
    ph["age"] = age
    ph = ph.iloc[:nph if nph is not None else n].sample(frac=1.0, random_state=5).reset_index(drop=True)
    return gdf, ph


def run_mega(tmp_path, name, *, data=None, engine="standin", double=True, geno_kw=None, model_kw=None, t=6, rhs="intercept + age + geno",
             equation=None, ph_edit=None, model_edit=None, **kw):
    from jwas_jl_amd import api
    gdf, ph = data if data is not None else mega_data(t=t)
    ph = ph.copy()
    if ph_edit is not None:
        ph = ph_edit(ph)
    if engine == "standin":
        engine = MegaStandInEngine(64 if double else 32)
    with contextlib.redirect_stdout(io.StringIO()):
        gk = dict(method="BayesC", double_precision=double, constraint=True)
        gk.update(geno_kw or {})
        geno = api.get_genotypes(gdf, **gk)                              # noqa: F841 (build_model finds it)
        mk = dict(constraint=True)
        mk.update(model_kw or {})
        model = api.build_model(equation or "\n".join(f"y{k + 1} = {rhs}" for k in range(t)), **mk)
        api.set_covariate(model, "age")
        if model_edit is not None:
            model_edit(model, api)
        args = dict(chain_length=20, burnin=5, seed=17, double_precision=double, output_folder=str(tmp_path / name), _engine=engine, block_size=20)
        args.update(kw)
        return api.runMCMC(model, ph, **args)


def check_outputs(out, folder, n_out, p, traits, nsaved, pi=True):
    t = len(traits)
    rnames = [f"{a}_{b}" for a in traits for b in traits]
    me = out["marker effects geno"]
    assert list(me.columns) == ["Trait", "Marker_ID", "Estimate", "SD", "Model_Frequency"] and len(me) == t * p
    assert list(me["Trait"].unique()) == traits
    assert list(out["residual variance"]["Covariance"]) == rnames and list(out["marker effects variance geno"]["Covariance"]) == rnames
    for key in ("residual variance", "marker effects variance geno", "genetic_variance"):
        M = out[key]["Estimate"].to_numpy().reshape(t, t)
        assert np.all(np.diag(M) > 0) and np.all(M[~np.eye(t, dtype=bool)] == 0.0), key      # constraint: the diagonal only
    assert list(out["heritability"]["Covariance"]) == traits and np.all((out["heritability"]["Estimate"] > 0) & (out["heritability"]["Estimate"] < 1))
    if pi:
        assert list(out["pi_geno"]["π"]) == traits and np.all((out["pi_geno"]["Estimate"] > 0) & (out["pi_geno"]["Estimate"] < 1))
    else:
        assert "pi_geno" not in out
    assert list(out["location parameters"]["Effect"]) == ["intercept", "age"] * t
    for tr in traits:
        assert len(out[f"EBV_{tr}"]) == n_out and list(out[f"EBV_{tr}"].columns) == ["ID", "EBV", "PEV"]
    names = ["residual_variance", "marker_effects_variances_geno", "genetic_variance", "heritability"] + (["pi_geno"] if pi else [])
    names += [f"marker_effects_geno_{tr}" for tr in traits]
    width = {"residual_variance": t * t, "marker_effects_variances_geno": t * t, "genetic_variance": t * t, "heritability": t, "pi_geno": t}
    for nm in names:
        rows = open(os.path.join(folder, f"MCMC_samples_{nm}.txt")).read().strip().split("\n")
        assert len(rows) == nsaved + 1, nm
        assert len(rows[0].split(",")) == len(rows[1].split(",")) == width.get(nm, p), nm
    assert open(os.path.join(folder, "MCMC_samples_pi_geno.txt")).readline().strip() == ",".join(f"pi{k + 1}" for k in range(t)) if pi else True
    from jwas_jl_amd import samples
    for tr in traits:
        recs = list(samples.iter_records(os.path.join(folder, f"MCMC_samples_marker_effects_geno_{tr}.bin")))
        assert len(recs) == nsaved
    for tab in out.values():
        if hasattr(tab, "select_dtypes"):
            assert np.all(np.isfinite(tab.select_dtypes("number").to_numpy()))
    for key in out:
        if key != "_timing":
            assert os.path.exists(os.path.join(folder, key.replace(" ", "_") + ".txt"))
    assert os.path.exists(os.path.join(folder, "IDs_for_individuals_with_phenotypes.txt"))


def test_six_trait_run_writes_every_output(tmp_path):
    data = mega_data()
    eng = MegaStandInEngine(64)
    out = run_mega(tmp_path, "a", data=data, engine=eng)
    p = len(out["marker effects geno"]) // 6
    check_outputs(out, str(tmp_path / "a"), 60, p, TRAITS6, 15)
    assert out["_timing"]["ntraits"] == 6 and out["_timing"]["n"] == 60
    assert eng.calls[:2] == ["load_dense", "mega_begin"] and eng.calls.count("mega_sweep") == 20 and eng.calls.count("mega_impute") == 20
    assert eng.calls[-1] == "mega_end"
    assert out["pi_geno"]["SD"].max() > 0 and len(set(out["pi_geno"]["Estimate"])) == 6          # one pi per trait
    # the sparse .bin samples hold the text rows
    from jwas_jl_amd import samples
    dense = samples.read_dense(str(tmp_path / "a" / "MCMC_samples_marker_effects_geno_y3.bin"))
    dense = dense[0] if isinstance(dense, tuple) else dense
    text = np.loadtxt(tmp_path / "a" / "MCMC_samples_marker_effects_geno_y3.txt", delimiter=",", skiprows=1)
    np.testing.assert_allclose(np.asarray(dense, dtype=np.float64), text, rtol=1e-6, atol=0)
    # RR-BLUP: every marker in the model, no pi
    rr = run_mega(tmp_path, "rr", data=data, geno_kw=dict(method="RR-BLUP"))
    check_outputs(rr, str(tmp_path / "rr"), 60, p, TRAITS6, 15, pi=False)
    assert np.all(rr["marker effects geno"]["Model_Frequency"] == 1.0)
    # Float32 storage, estimatePi = false with one Pi per trait
    used = {}

    class Spy(MegaStandInEngine):
        def mega_sweep(self, **kw):
            used.setdefault("pi", []).append(np.asarray(kw["pi"]).copy())
            return super().mega_sweep(**kw)
    pis = [0.3, 0.5, 0.7, 0.9, 0.6, 0.8]
    f32 = run_mega(tmp_path, "f32", data=data, double=False, engine=Spy(32), geno_kw=dict(estimatePi=False, Pi=pis))
    check_outputs(f32, str(tmp_path / "f32"), 60, p, TRAITS6, 15, pi=False)
    assert len(used["pi"]) == 20 and all(np.array_equal(v, pis) for v in used["pi"])


def test_routing_rule(tmp_path):
    """5 traits and more with constraint=true on both sides go to the mega-trait driver; 4 traits keep mcmc.py's MegaBayesC sweep."""
    from oracle_engine import OracleEngine
    eng = MegaStandInEngine(64)
    out = run_mega(tmp_path, "five", data=mega_data(t=5), t=5, engine=eng, chain_length=4, burnin=0)
    assert "mega_sweep" in eng.calls and len(out["pi_geno"]) == 5
    used = {}

    class Spy(OracleEngine):
        def init_state(self, m, t=1):
            used["method"], used["t"] = m, t
            return super().init_state(m, t)

        def sweep(self, **kw):
            used["sweeps"] = used.get("sweeps", 0) + 1
            return super().sweep(**kw)

        def __getattr__(self, name):
            assert not name.startswith("mega_"), "a model of 4 traits reached the mega-trait driver"
            raise AttributeError(name)
    gdf, ph = mega_data(t=4, missing=0.0)
    out4 = run_mega(tmp_path, "four", data=(gdf, ph), t=4, engine=Spy("block"), double=False, chain_length=4, burnin=0, block_size=64)
    assert used == {"method": "MegaBayesC", "t": 4, "sweeps": 4} and list(out4["pi_geno"]["π"]) == ["y1", "y2", "y3", "y4"]


def test_priors_are_the_references_constraint_priors():
    """constraint_priors against a literal restatement of the defaults followed by R_constraint! and G_constraint!
    (input_data_validation.jl:296-350,530-559; tools4genotypes.jl:414-438)."""
    from jwas_jl_amd import api, megatrait
    gdf, ph = mega_data()
    t, df = 6, 4.0
    for pi in (0.0, 0.5, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", Pi=pi, constraint=True, double_precision=True)      # noqa: F841
            model = api.build_model("\n".join(f"y{k + 1} = intercept + geno" for k in range(t)), constraint=True)
        phenovar = np.linspace(0.5, 2.0, t)
        got = megatrait.constraint_priors(model, phenovar, np.float64)
        Mi = model.M[0]
        # the reference, literally
        R_df, G_df = df + t, df + t                                      # build_MME.jl:128-134, :98-116
        R_val = np.diag(phenovar * 0.5)
        R_scale = R_val * (R_df - t - 1)                                 # input_data_validation.jl:296-350
        pi_t = np.full(t, pi) if np.isscalar(pi) else np.array(pi)
        G_val = np.diag((phenovar * 0.5) / (Mi.sum2pq * (1 - pi_t)))     # genetic2marker's diagonal
        G_scale = G_val * (G_df - t - 1)                                 # tools4genotypes.jl:414-418
        R_df = R_df - t                                                  # R_constraint!
        R_scale = np.diag(np.diag(R_scale / (R_df - 1))) * (R_df - 2) / R_df
        G_df = G_df - t                                                  # G_constraint!
        G_scale = np.diag(np.diag(G_scale / (G_df - 1))) * (G_df - 2) / G_df
        assert got["R_df"] == R_df == 4.0 and got["G_df"] == G_df == 4.0
        np.testing.assert_allclose(got["R_scale"], np.diag(R_scale), rtol=1e-15)
        np.testing.assert_allclose(got["G_scale"], np.diag(G_scale), rtol=1e-15)
        np.testing.assert_allclose(got["vare"], np.diag(R_val), rtol=1e-15)
        np.testing.assert_allclose(got["G"], np.diag(G_val), rtol=1e-15)
        np.testing.assert_array_equal(got["pi"], pi_t)
        # the prior mean of a scaled inverse chi-square with these df and scale is the starting value
        np.testing.assert_allclose(got["R_scale"] * got["R_df"] / (got["R_df"] - 2), got["vare"], rtol=1e-14)
        assert np.array_equal(model.R.val, np.diag(np.diag(model.R.val))) and np.array_equal(Mi.G.scale, np.diag(np.diag(Mi.G.scale)))


def test_missing_cells_observed_cells_are_never_rewritten(tmp_path):
    seen = []

    class Spy(MegaStandInEngine):
        def mega_set_missing(self, missing):
            seen.append(("pattern", np.asarray(missing).copy()))
            return super().mega_set_missing(missing)

        def mega_impute(self, **kw):
            before = self._mega.R.copy()
            super().mega_impute(**kw)
            seen.append(("impute", before, self._mega.R.copy(), np.asarray(kw["vare"]).copy()))
    data = mega_data()
    run_mega(tmp_path, "m", data=data, engine=Spy(64), chain_length=6, burnin=0)
    pattern = seen[0][1]
    assert seen[0][0] == "pattern" and pattern.shape == (6, 60) and not pattern[0].any() and 0.05 < pattern.mean() < 0.3
    steps = [s for s in seen if s[0] == "impute"]
    assert len(steps) == 6
    for _, before, after, vare in steps:
        assert np.array_equal(before[~pattern], after[~pattern]) and not np.any(before[pattern] == after[pattern])
        assert vare.shape == (6,) and np.all(vare > 0)
    # complete records: no pattern is uploaded, no cell is redrawn
    eng = MegaStandInEngine(64)
    run_mega(tmp_path, "c", data=mega_data(missing=0.0), engine=eng, chain_length=3, burnin=0)
    assert "mega_impute" not in eng.calls and eng.calls.count("mega_sweep") == 3
    with pytest.raises(ValueError, match="missing_phenotypes=false"):
        run_mega(tmp_path, "mp", data=data, missing_phenotypes=False)


def test_output_ebv_ids_without_records(tmp_path):
    """outputEBV(model, IDs) with genotyped individuals that have no record: EBV = X_out alpha from the second resident matrix."""
    gdf, ph = mega_data(nph=50)
    want = [f"i{i}" for i in range(45, 60)]                              # i50 .. i59 have no phenotype
    out = run_mega(tmp_path, "o", data=(gdf, ph), model_edit=lambda m, api_: api_.outputEBV(m, want))
    assert out["_timing"]["n"] == 50
    Xc = gdf.iloc[:, 1:].to_numpy(dtype=np.float64)
    Xc = Xc - Xc.mean(axis=0)
    for tr in TRAITS6:
        tab = out[f"EBV_{tr}"]
        assert list(tab["ID"]) == want
        a = out["marker effects geno"].query("Trait == @tr")["Estimate"].to_numpy()
        np.testing.assert_allclose(tab["EBV"].to_numpy(), Xc[45:60] @ a, rtol=0, atol=1e-12)
    assert np.abs(out["EBV_y2"]["EBV"]).max() > 0


def test_same_seed_same_files(tmp_path):
    data = mega_data()
    a = run_mega(tmp_path, "a", data=data)
    run_mega(tmp_path, "b", data=data)
    for f in sorted(os.listdir(tmp_path / "a")):
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    c = run_mega(tmp_path, "c", data=data, seed=18)
    assert not np.array_equal(c["marker effects geno"]["Estimate"], a["marker effects geno"]["Estimate"])


def test_contract_errors(tmp_path):
    """Everything else with more than 4 traits raises NotImplementedError naming the argument, with no engine call and no folder."""
    data = mega_data()
    count = [0]

    def fails(match, exc=NotImplementedError, **kw):
        count[0] += 1
        eng = kw.pop("engine", None) or MegaStandInEngine(64 if kw.get("double", True) else 32)
        with pytest.raises(exc, match=match):
            run_mega(tmp_path, f"e{count[0]}", data=data, engine=eng, **kw)
        assert not os.path.exists(tmp_path / f"e{count[0]}")            # nothing was written
        assert getattr(eng, "calls", []) == []                           # no device work

    fails("constraint=True in BOTH get_genotypes and build_model", geno_kw=dict(constraint=False))
    fails("constraint=True in BOTH get_genotypes and build_model", model_kw=dict(constraint=False))
    fails("constraint=True in BOTH", geno_kw=dict(constraint=False), model_kw=dict(constraint=False))
    for method in ("BayesA", "BayesB", "BayesL", "BayesR"):
        fails(f"method={method}", geno_kw=dict(method=method))
    fails("annotations", geno_kw=dict(annotations=np.random.default_rng(1).random((48, 2))))
    fails("independent_blocks", fast_blocks=True, independent_blocks=True)
    fails("fast_blocks", fast_blocks=True)
    fails("fast_blocks", fast_blocks=[1, 21, 41])
    fails("heterogeneous_residuals", heterogeneous_residuals=True, ph_edit=lambda ph: ph.assign(weights=1.0))
    fails('location_parameters="device"', location_parameters="device")
    fails("set_random", rhs="intercept + age + herd + geno", ph_edit=lambda ph: ph.assign(herd=[f"h{i % 3}" for i in range(len(ph))]),
          model_edit=lambda m, api_: api_.set_random(m, "herd"))
    fails("categorical_trait / censored_trait", model_kw=dict(categorical_trait=["y2"]))
    fails("categorical_trait / censored_trait", model_kw=dict(censored_trait=["y3"]))
    fails("causal_structure", causal_structure=np.tril(np.ones((6, 6)), -1))
    fails("RRM", RRM=np.ones((3, 2)))
    fails("RRM", RRM=True)
    fails("single_step_analysis", single_step_analysis=True)
    fails("starting_value", geno_kw=dict(starting_value=np.zeros(6 * 48)))
    fails("starting_value", starting_value=np.zeros(12))
    fails("Dict Pi", geno_kw=dict(Pi={tuple([1.0] * 6): 1.0}))
    fails("one value per trait", exc=ValueError, geno_kw=dict(Pi=[0.5, 0.5]))
    fails("block_size", exc=ValueError, block_size=257)

    class Sharded(MegaStandInEngine):
        def comm_info(self):
            return (0, 2)
    fails("shards", engine=Sharded(64))
    # several genotype categories
    from jwas_jl_amd import api
    gdf, ph = data
    with contextlib.redirect_stdout(io.StringIO()):
        g1 = api.get_genotypes(gdf.iloc[:, :25], method="BayesC", constraint=True)
        g2 = api.get_genotypes(gdf.iloc[:, [0] + list(range(25, 49))], method="BayesC", constraint=True)
        model = api.build_model("\n".join(f"y{k + 1} = intercept + g1 + g2" for k in range(6)), constraint=True, genotypes={"g1": g1, "g2": g2})
    with pytest.raises(NotImplementedError, match="several genotype categories"):
        api.runMCMC(model, ph, output_folder=str(tmp_path / "mg"), _engine=[MegaStandInEngine(32), MegaStandInEngine(32)])
    assert not os.path.exists(tmp_path / "mg")
    # storage=:stream
    from jwas_jl_amd import streaming as S
    prefix = S.prepare_streaming_genotypes(gdf.iloc[:, 1:].to_numpy(dtype=np.float64), tmp_path / "st", obs_ids=list(gdf["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", storage="stream", constraint=True)      # noqa: F841
        model = api.build_model("\n".join(f"y{k + 1} = intercept + geno" for k in range(6)), constraint=True)
    with pytest.raises(NotImplementedError, match="storage=:stream"):
        api.runMCMC(model, ph, output_folder=str(tmp_path / "stream"), _engine=MegaStandInEngine(32))
    assert not os.path.exists(tmp_path / "stream")
    # more than 64 traits
    import pandas as pd
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC", constraint=True)                          # noqa: F841
        model = api.build_model("\n".join(f"t{k} = intercept + geno" for k in range(65)), constraint=True)
    wide = pd.concat([ph[["ID"]], pd.DataFrame(np.random.default_rng(2).standard_normal((len(ph), 65)), columns=[f"t{k}" for k in range(65)])], axis=1)
    with pytest.raises(NotImplementedError, match="at most 64 traits"):
        api.runMCMC(model, wide, output_folder=str(tmp_path / "wide"), _engine=MegaStandInEngine(32))
    assert not os.path.exists(tmp_path / "wide")
    # no CPU fallback: an engine without the mega_* methods
    class NoMega:
        precision, dtype = 64, np.float64
    with pytest.raises(NotImplementedError, match="no CPU fallback") as ei:
        run_mega(tmp_path, "nofallback", data=data, engine=NoMega())
    assert "mega_sweep" in str(ei.value) and "mega_begin" in str(ei.value) and not os.path.exists(tmp_path / "nofallback")
