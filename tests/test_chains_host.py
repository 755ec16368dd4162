"""runMCMC(chains=K) (chains.py) and PSRF (diagnostics.py) on the CPU stand-in (tests/chains_reference.py): the BayesR restatement
against its own marker-by-marker chain and the closed-form posterior, the routing rule, chain k against the chain run alone, the
seed, the layout, the pooled tables, the PSRF rows, every refusal of the contract, and the reference's PSRF on hand-computed files."""
import contextlib
import io
import os

import numpy as np
import pytest

import chains_reference as CR
from chains_reference import ChainsStandInEngine


# ---- 1. the restatement itself ---------------------------------------------------------------------------------------------------------
def test_bayesr_block_form_is_the_marker_by_marker_chain():
    """n = 301, p = 100, 9 chains (pi and gamma in turn), three sweeps with shared draws: blocks of 1, 40 and p choose the classes of the
    plain chain; effects and residuals agree within 1e-11 relative (the bound of tests/test_megatrait_host.py for BayesC)."""
    cs = CR.case_chains(CR.make_case_r(), 9)

    def run(bs):
        R, a, b, d = cs.R.copy(), cs.alpha.copy(), cs.beta.copy(), cs.delta.copy()
        out = []
        for it in (1, 2, 3):
            kw = dict(iteration=it, seed=5, vare=cs.vare, var_effect=cs.sig, gamma=cs.gamma, pi=cs.pi, min_margin=CR.MIN_MARGIN)
            r = CR.sweep_r_plain(cs.X, R, a, b, d, **kw) if bs is None else CR.sweep_r_blocked(cs.X, R, a, b, d, block_size=bs, **kw)
            out.append((d.copy(), a.copy(), R.copy(), r))
        return out
    ref = run(None)
    assert all(o[3].n_changed.min() > 0 for o in ref) and not np.array_equal(ref[0][0], ref[1][0])
    d_all = np.concatenate([o[0] for o in ref], axis=1)
    assert set(np.unique(d_all)) == {1.0, 2.0, 3.0, 4.0}
    assert np.all(d_all[2] > 1.0) and np.all(d_all[3] != 2.0)              # pi_1 = 0: no marker in the null class; pi_2 = 0: none in class 2
    for o in ref:
        assert np.array_equal(o[1] == 0.0, o[0] == 1.0)                     # class 1 and only class 1 holds a zero effect
        assert np.array_equal(o[3].class_counts.sum(axis=0), np.full(9, float(cs.p))) and np.array_equal(o[3].nnz, cs.p - o[3].class_counts[0])
    for bs in (1, 40, cs.p):
        for (d0, a0, r0, s0), (d1, a1, r1, s1) in zip(ref, run(bs)):
            assert np.array_equal(d0, d1)
            da, dr = (np.abs(x - y).max() / np.abs(x).max() for x, y in ((a0, a1), (r0, r1)))
            print(f"blocks of {bs}: alpha {da:.2e}, residual {dr:.2e} relative")
            assert max(da, dr) <= 1e-11
            assert np.array_equal(s0.class_counts, s1.class_counts) and np.array_equal(s0.n_changed, s1.n_changed)


def test_no_decision_uniform_of_the_gpu_cases_is_near_a_boundary():
    """The chains tests/test_gpu_chains.py compares classes with: all 64 chains, iterations 1 and 2, blocks of 64 and 100 (and 1 and 40
    for 9 chains).  reference_sweeps_r asserts the 1e-9 margin; the seed is the GPU tests'."""
    cs = CR.make_case_r()
    for bs in (64, 100):
        for it, r in enumerate(CR.reference_sweeps_r(cs, 64, 5, bs), 1):
            print(f"blocks of {bs}, iteration {it}: nearest CDF boundary {r.margins.min():.2e}")
            assert r.margins.min() >= CR.MIN_MARGIN
    for bs in (1, 40):
        assert min(r.margins.min() for r in CR.reference_sweeps_r(cs, 9, 5, bs)) >= CR.MIN_MARGIN


# ---- 2. the closed-form posterior --------------------------------------------------------------------------------------------------------
def test_one_marker_bayesr_draws_follow_the_closed_form_posterior():
    case = CR.conditional_case_r()
    probs, _, _ = CR.conditional_posterior_r(case)
    assert (probs * CR.CONDITIONAL_STEPS).min() >= CR.MIN_EXPECTED         # every class of every chain is visited often enough
    rows = CR.conditional_check_r(CR.conditional_engine_r(ChainsStandInEngine(64), case), case)
    for k, c, ex, zf, zm, zv in rows:
        print(f"chain {k} class {c}: expected {ex:.0f}; frequency {zf:.2f} se; effect mean {zm:.2f}, variance {zv:.2f}")
    assert len(rows) == 12 and max(max(r[3:]) for r in rows) <= 5.0


# ---- 3. the driver ---------------------------------------------------------------------------------------------------------------------------
def chain_data(n=60, p=48, seed=3, nph=None):
    import pandas as pd
    rng = np.random.default_rng(seed)
    ids = [f"i{i}" for i in range(n)]
    raw = rng.binomial(2, rng.uniform(0.15, 0.85, p), size=(n, p)).astype(np.float64)
    gdf = pd.DataFrame(raw, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    Xc = raw - raw.mean(axis=0)
    a = np.zeros(p)
    a[rng.choice(p, 8, replace=False)] = 0.4 * rng.standard_normal(8)
    age = rng.uniform(1, 3, n)
    ph = pd.DataFrame({"ID": ids, "y": 1.0 + 0.3 * age + Xc @ a + 0.6 * rng.standard_normal(n), "age": age})
    ph = ph.iloc[:nph if nph is not None else n].sample(frac=1.0, random_state=5).reset_index(drop=True)
    return gdf, ph


def run_k(tmp_path, name, *, data=None, engine="standin", double=True, method="BayesC", geno_kw=None, model_kw=None, rhs="intercept + age + geno",
          ph_edit=None, model_edit=None, equation=None, **kw):
    from jwas_jl_amd import api
    gdf, ph = data if data is not None else chain_data()
    ph = ph.copy()
    if ph_edit is not None:
        ph = ph_edit(ph)
    if engine == "standin":
        engine = ChainsStandInEngine(64 if double else 32)
    with contextlib.redirect_stdout(io.StringIO()):
        gk = dict(method=method, double_precision=double)
        gk.update(geno_kw or {})
        geno = api.get_genotypes(gdf, **gk)                              # noqa: F841 (build_model finds it)
        model = api.build_model(equation or f"y = {rhs}", **(model_kw or {}))
        api.set_covariate(model, "age")
        if model_edit is not None:
            model_edit(model, api)
        args = dict(chain_length=20, burnin=5, seed=17, double_precision=double, output_folder=str(tmp_path / name), _engine=engine, block_size=20,
                    chains=3)
        args.update(kw)
        return api.runMCMC(model, ph, **args)


def _files(folder):
    return sorted(f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)))


def test_routing(tmp_path, monkeypatch):
    """chains=1 (and the default) never touches chains.py; chains=3 does; anything else is a ValueError."""
    from jwas_jl_amd import chains as CH
    called = []
    real = CH.run_chains
    monkeypatch.setattr(CH, "validate", lambda *a, **k: called.append("validate"))
    monkeypatch.setattr(CH, "run_chains", lambda *a, **k: called.append("run") or real(*a, **k))

    from jwas_jl_amd import api
    monkeypatch.setattr(api, "run_chain", lambda *a, **k: "single-chain driver")
    for i, kw in enumerate((dict(chains=1), dict(chains=np.int64(1)))):
        assert run_k(tmp_path, f"d{i}", **kw) == "single-chain driver" and called == []
    gdf, ph = chain_data()
    with contextlib.redirect_stdout(io.StringIO()):                       # the default: no chains keyword at all
        geno = api.get_genotypes(gdf, method="BayesC", double_precision=True)      # noqa: F841 (build_model finds it)
        model = api.build_model("y = intercept + geno")
        assert api.runMCMC(model, ph, chain_length=3, double_precision=True, output_folder=str(tmp_path / "dd"), _engine=ChainsStandInEngine(64)) == "single-chain driver"
    assert called == []
    out = run_k(tmp_path, "three", chains=3)
    assert called == ["validate", "run"] and len(out["chains"]) == 3
    for bad in (0, -1, 65, 2.5, "2", True, None):
        with pytest.raises(ValueError, match="chains must be"):
            run_k(tmp_path, "bad", chains=bad)
        assert not os.path.exists(tmp_path / "bad")
    with pytest.raises(ValueError, match="first_chain"):
        run_k(tmp_path, "bad", chains=1, first_chain=2)
    assert not os.path.exists(tmp_path / "bad")


@pytest.mark.parametrize("method,kw", [("BayesC", {}), ("BayesC", dict(geno_kw=dict(Pi=0.7, estimatePi=False))), ("RR-BLUP", {}), ("BayesR", {}),
                                       ("BayesR", dict(bayesr_gamma=[0.0, 0.001, 0.05, 2.0], geno_kw=dict(Pi=[0.6, 0.2, 0.1, 0.1])))])
def test_chain_k_equals_the_chain_run_alone(tmp_path, method, kw):
    """Chain k of a K-chain run equals that chain run alone (chains=2, first_chain=k takes its first chain) in every output file."""
    data = chain_data()
    full = run_k(tmp_path, "full", data=data, method=method, chains=5, **kw)
    names = _files(tmp_path / "full" / "chain_0")
    assert len(names) >= 8 and any(f.endswith(".bin") for f in names)
    for k in (0, 2, 4):
        run_k(tmp_path, f"solo{k}", data=data, method=method, chains=2, first_chain=k, **kw)
        assert _files(tmp_path / f"solo{k}" / f"chain_{k}") == names
        for f in names:
            assert open(tmp_path / "full" / f"chain_{k}" / f, "rb").read() == open(tmp_path / f"solo{k}" / f"chain_{k}" / f, "rb").read(), (k, f)
    a = [c["marker effects geno"]["Estimate"].to_numpy() for c in full["chains"]]
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])       # the chains differ


def test_same_seed_same_files_other_seed_differs(tmp_path):
    data = chain_data()
    a = run_k(tmp_path, "a", data=data, method="BayesR")
    run_k(tmp_path, "b", data=data, method="BayesR")
    seen = 0
    for root, _, fs in os.walk(tmp_path / "a"):
        for f in fs:
            rel = os.path.relpath(os.path.join(root, f), tmp_path / "a")
            assert open(tmp_path / "a" / rel, "rb").read() == open(tmp_path / "b" / rel, "rb").read(), rel
            seen += 1
    assert seen > 30
    c = run_k(tmp_path, "c", data=data, method="BayesR", seed=18)
    assert not np.array_equal(c["marker effects geno"]["Estimate"], a["marker effects geno"]["Estimate"])
    assert not np.array_equal(c["PSRF"]["PSRF"].to_numpy(), a["PSRF"]["PSRF"].to_numpy())


@pytest.mark.parametrize("method", ["BayesC", "BayesR"])
def test_layout_keys_pooled_tables_and_psrf(tmp_path, method):
    import pandas as pd
    K, p, nsaved = 4, 48, 15
    eng = ChainsStandInEngine(64)
    out = run_k(tmp_path, "r", method=method, chains=K, engine=eng)
    folder = tmp_path / "r"
    assert sorted(d for d in os.listdir(folder) if os.path.isdir(folder / d)) == [f"chain_{k}" for k in range(K)]
    assert eng.calls.count("mega_begin") == 1 and eng.calls.count("load_dense") == 1          # one session, one upload
    assert eng.calls.count("mega_sweep_r" if method == "BayesR" else "mega_sweep") == 20 and eng.calls[-1] == "mega_end"
    assert {"chains", "PSRF", "PSRF_summary", "marker effects geno", "residual variance", "marker effects variance geno", "pi_geno",
            "location parameters", "EBV_y", "genetic_variance", "heritability"} <= set(out)
    npi = 4 if method == "BayesR" else 1
    for k in range(K):
        names = _files(folder / f"chain_{k}")
        for nm in ("MCMC_samples_residual_variance.txt", "MCMC_samples_marker_effects_variances_geno.txt", "MCMC_samples_pi_geno.txt",
                   "MCMC_samples_marker_effects_geno_y.txt", "MCMC_samples_marker_effects_geno_y.bin", "MCMC_samples_genetic_variance.txt",
                   "MCMC_samples_heritability.txt", "marker_effects_geno.txt", "residual_variance.txt", "pi_geno.txt", "EBV_y.txt",
                   "location_parameters.txt", "IDs_for_individuals_with_phenotypes.txt"):
            assert nm in names, nm
        assert pd.read_csv(folder / f"chain_{k}" / "MCMC_samples_pi_geno.txt").shape == (nsaved, npi)
        assert pd.read_csv(folder / f"chain_{k}" / "MCMC_samples_marker_effects_geno_y.txt").shape == (nsaved, p)
    for nm in ("PSRF.txt", "PSRF_summary.txt", "marker_effects_geno.txt", "residual_variance.txt", "EBV_y.txt"):
        assert os.path.isfile(folder / nm), nm
    # the pooled tables: the mean of the chain means, the SD from the pooled second moment
    per = out["chains"]
    for key, col in (("marker effects geno", "Estimate"), ("marker effects geno", "Model_Frequency"), ("residual variance", "Estimate"),
                     ("marker effects variance geno", "Estimate"), ("pi_geno", "Estimate"), ("EBV_y", "EBV"), ("location parameters", "Estimate")):
        np.testing.assert_allclose(out[key][col].to_numpy(), np.mean([c[key][col].to_numpy() for c in per], axis=0), rtol=1e-13, atol=1e-15)
    rv = np.array([pd.read_csv(folder / f"chain_{k}" / "MCMC_samples_residual_variance.txt")["y"].to_numpy() for k in range(K)])
    np.testing.assert_allclose(out["residual variance"]["SD"].to_numpy()[0], np.sqrt((rv * rv).mean() - rv.mean() ** 2), rtol=1e-10)
    al = np.array([pd.read_csv(folder / f"chain_{k}" / "MCMC_samples_marker_effects_geno_y.txt").to_numpy() for k in range(K)])      # K x N x p
    np.testing.assert_allclose(out["marker effects geno"]["SD"].to_numpy(), np.sqrt(np.abs((al * al).mean(axis=(0, 1)) - al.mean(axis=(0, 1)) ** 2)),
                               rtol=1e-9, atol=1e-14)
    if method == "BayesR":                                                # the model frequency of a BayesR chain: class > 1, that is a nonzero effect
        np.testing.assert_allclose(per[1]["marker effects geno"]["Model_Frequency"].to_numpy(), (al[1] != 0.0).mean(axis=0), rtol=1e-12)
    # PSRF.txt: the marker rows and the scalar rows against a direct numpy computation from the saved samples
    ps = out["PSRF"]
    assert list(ps.columns) == ["Parameter", "PSRF"] and len(ps) == p + npi + 2
    assert list(ps["Parameter"][:2]) == ["marker_effect_geno:m0", "marker_effect_geno:m1"] and list(ps["Parameter"][-2:]) == ["marker_effects_variance_geno", "residual_variance"]
    direct = CR.psrf_from_samples(al)
    got = ps["PSRF"].to_numpy()[:p]
    assert np.array_equal(np.isnan(got), np.isnan(direct))
    np.testing.assert_allclose(got[np.isfinite(got)], direct[np.isfinite(direct)], rtol=1e-9)
    pis = np.array([pd.read_csv(folder / f"chain_{k}" / "MCMC_samples_pi_geno.txt").to_numpy() for k in range(K)])
    gv = np.array([pd.read_csv(folder / f"chain_{k}" / "MCMC_samples_marker_effects_variances_geno.txt").to_numpy() for k in range(K)])
    scal = np.concatenate([CR.psrf_from_samples(pis), CR.psrf_from_samples(gv), CR.psrf_from_samples(rv[:, :, None])])
    np.testing.assert_allclose(ps["PSRF"].to_numpy()[p:], scal, rtol=1e-12)
    assert np.all(np.isfinite(scal)) and np.all(scal > 0.5)
    pd.testing.assert_frame_equal(pd.read_csv(folder / "PSRF.txt"), ps, rtol=1e-14)
    sm = dict(zip(out["PSRF_summary"]["Statistic"], out["PSRF_summary"]["Value"]))
    fin = got[np.isfinite(got)]
    assert sm["chains"] == K and sm["saved_samples"] == nsaved and sm["markers_with_finite_PSRF"] == fin.size
    assert sm["max"] == fin.max() and sm["percentile_99"] == np.percentile(fin, 99) and sm["count_above_1.1"] == (fin > 1.1).sum()


def test_psrf_is_nan_where_no_chain_ever_had_the_marker(tmp_path):
    """W == 0 gives NaN: under BayesC with pi = 0.999 fixed most markers never enter the model in a short run of any chain."""
    import pandas as pd
    out = run_k(tmp_path, "nan", chains=2, geno_kw=dict(Pi=0.999, estimatePi=False), chain_length=8, burnin=2)
    al = np.array([pd.read_csv(tmp_path / "nan" / f"chain_{k}" / "MCMC_samples_marker_effects_geno_y.txt").to_numpy() for k in range(2)])
    never = np.all(al == 0.0, axis=(0, 1))
    got = out["PSRF"]["PSRF"].to_numpy()[:48]
    assert 0 < never.sum() < 48 and np.array_equal(np.isnan(got), never)
    assert "pi_geno" not in out and list(out["PSRF"]["Parameter"][48:]) == ["marker_effects_variance_geno", "residual_variance"]
    # fewer than two saved samples: every row NaN, nothing raised
    one = run_k(tmp_path, "one", chains=2, chain_length=3, burnin=2)
    assert np.all(np.isnan(one["PSRF"]["PSRF"])) and np.isnan(dict(zip(one["PSRF_summary"]["Statistic"], one["PSRF_summary"]["Value"]))["max"])


def test_output_ebv_ids_without_records(tmp_path):
    gdf, ph = chain_data(nph=50)
    want = [f"i{i}" for i in range(45, 60)]
    out = run_k(tmp_path, "o", data=(gdf, ph), method="BayesR", model_edit=lambda m, api_: api_.outputEBV(m, want))
    Xc = gdf.iloc[:, 1:].to_numpy(dtype=np.float64)
    Xc = Xc - Xc.mean(axis=0)
    for tab_set in out["chains"] + [out]:
        assert list(tab_set["EBV_y"]["ID"]) == want
        np.testing.assert_allclose(tab_set["EBV_y"]["EBV"].to_numpy(), Xc[45:60] @ tab_set["marker effects geno"]["Estimate"].to_numpy(), rtol=0, atol=1e-12)


def test_contract_errors(tmp_path):
    """Everything outside the scope raises NotImplementedError naming the argument, with no engine call and no folder."""
    data = chain_data()
    count = [0]

    def fails(match, exc=NotImplementedError, **kw):
        count[0] += 1
        eng = kw.pop("engine", None) or ChainsStandInEngine(64 if kw.get("double", True) else 32)
        with pytest.raises(exc, match=match):
            run_k(tmp_path, f"e{count[0]}", data=data, engine=eng, **kw)
        assert not os.path.exists(tmp_path / f"e{count[0]}")            # nothing was written
        assert getattr(eng, "calls", []) == []                           # no device work

    for method in ("BayesA", "BayesB", "BayesL"):
        fails(f"method={method}", method=method)
    fails("annotations", geno_kw=dict(annotations=np.random.default_rng(1).random((48, 2))))
    fails("independent_blocks", fast_blocks=True, independent_blocks=True)
    fails("fast_blocks", fast_blocks=True)
    fails("fast_blocks", fast_blocks=[1, 21, 41])
    fails("heterogeneous_residuals", heterogeneous_residuals=True, ph_edit=lambda ph: ph.assign(weights=1.0))
    fails('location_parameters="device"', location_parameters="device")
    fails("set_random", rhs="intercept + age + herd + geno", ph_edit=lambda ph: ph.assign(herd=[f"h{i % 3}" for i in range(len(ph))]),
          model_edit=lambda m, api_: api_.set_random(m, "herd"))
    fails("categorical_trait / censored_trait", model_kw=dict(categorical_trait=["y"]))
    fails("categorical_trait / censored_trait", model_kw=dict(censored_trait=["y"]))
    fails("causal_structure", causal_structure=np.zeros((1, 1)))
    fails("RRM", RRM=np.ones((3, 2)))
    fails("RRM", RRM=True)
    fails("single_step_analysis", single_step_analysis=True)
    fails("starting_value", geno_kw=dict(starting_value=np.zeros(48)))
    fails("starting_value", starting_value=np.zeros(2))
    fails("block_size", exc=ValueError, block_size=257)
    fails("first_chain", exc=ValueError, first_chain=-1)
    fails("first_chain", exc=ValueError, first_chain=(1 << 24) - 2)
    fails("bayesr_gamma", exc=ValueError, bayesr_gamma=[0.0, 0.01, 0.1, 1.0])                     # BayesC has no gamma
    fails("bayesr_gamma", exc=ValueError, method="BayesR", bayesr_gamma=[0.1, 0.01, 0.1, 1.0])
    fails("length 4", exc=ValueError, method="BayesR", geno_kw=dict(Pi=[0.5, 0.5]))

    class Sharded(ChainsStandInEngine):
        def comm_info(self):
            return (0, 2)
    fails("shards", engine=Sharded(64))
    # several traits, several genotype categories
    from jwas_jl_amd import api
    gdf, ph = data
    ph2 = ph.assign(y2=ph["y"] * 0.5 + 1.0)
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC")                           # noqa: F841
        model = api.build_model("y = intercept + geno\ny2 = intercept + geno")
    with pytest.raises(NotImplementedError, match="single-trait"):
        api.runMCMC(model, ph2, chains=2, output_folder=str(tmp_path / "mt"), _engine=ChainsStandInEngine(32))
    with contextlib.redirect_stdout(io.StringIO()):
        g1 = api.get_genotypes(gdf.iloc[:, :25], method="BayesC")
        g2 = api.get_genotypes(gdf.iloc[:, [0] + list(range(25, 49))], method="BayesC")
        model = api.build_model("y = intercept + g1 + g2", genotypes={"g1": g1, "g2": g2})
    with pytest.raises(NotImplementedError, match="several genotype categories"):
        api.runMCMC(model, ph, chains=2, output_folder=str(tmp_path / "mg"), _engine=[ChainsStandInEngine(32), ChainsStandInEngine(32)])
    # storage=:stream
    from jwas_jl_amd import streaming as S
    prefix = S.prepare_streaming_genotypes(gdf.iloc[:, 1:].to_numpy(dtype=np.float64), tmp_path / "st", obs_ids=list(gdf["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", storage="stream")      # noqa: F841
        model = api.build_model("y = intercept + geno")
    with pytest.raises(NotImplementedError, match="storage=:stream"):
        api.runMCMC(model, ph, chains=2, output_folder=str(tmp_path / "stream"), _engine=ChainsStandInEngine(32))
    for nm in ("mt", "mg", "stream"):
        assert not os.path.exists(tmp_path / nm)

    # no CPU fallback: an engine without the session's methods; the mega-trait stand-in lacks the new ones
    class NoMega:
        precision, dtype = 64, np.float64
    with pytest.raises(NotImplementedError, match="no CPU fallback") as ei:
        run_k(tmp_path, "nofallback", data=data, engine=NoMega())
    assert "mega_sweep_r" in str(ei.value) and "mega_psrf" in str(ei.value) and "mega_begin" in str(ei.value)
    with pytest.raises(NotImplementedError, match="no CPU fallback") as ei:
        run_k(tmp_path, "nofallback", data=data, engine=CR.MegaStandInEngine(64))
    assert "mega_sweep_r" in str(ei.value) and "mega_begin" not in str(ei.value) and not os.path.exists(tmp_path / "nofallback")


# ---- 4. PSRF(*files): the reference's function on sample files ---------------------------------------------------------------------------
def test_psrf_function_against_hand_computed_values(tmp_path):
    import jwas_jl_amd as J
    from jwas_jl_amd.diagnostics import PSRF
    assert J.PSRF is PSRF

    def write(name, rows, header=None):
        with open(tmp_path / name, "w") as fh:
            if header:
                fh.write(header + "\n")
            fh.write("\n".join(rows) + "\n")
        return str(tmp_path / name)
    # two chains of three values: means 2 and 4, variances 1 and 4; M = 2, N = 3
    #   B = 3 / 1 * ((2 - 3)^2 + (4 - 3)^2) = 6,  W = 2.5,  V = 2/3 * 2.5 + (3 / 3) * 2 * 6 = 5/3 + 12,  V / W = (5/3 + 12) / 2.5
    a, b = write("a.txt", ["1.0", "2.0", "3.0"], "x"), write("b.txt", ["2.0", "4.0", "6.0"], "x")
    assert PSRF(a, b) == pytest.approx((5.0 / 3.0 + 12.0) / 2.5, rel=1e-14)
    # without a header line: the first row counts; header=True on the same files drops it (N = 2: means 2.5, 5; variances 0.5, 2)
    a0, b0 = write("a0.txt", ["1.0", "2.0", "3.0"]), write("b0.txt", ["2.0", "4.0", "6.0"])
    assert PSRF(a0, b0, header=False) == pytest.approx((5.0 / 3.0 + 12.0) / 2.5, rel=1e-14)
    B2, W2 = 2 / 1 * (2 * 1.25 ** 2), 1.25
    assert PSRF(a0, b0) == pytest.approx((0.5 * W2 + 3 / 2 * 2 * B2) / W2, rel=1e-14)
    # three chains; a file of two columns is ONE pooled sample of its four values (white space or commas separate)
    #   values {0, 2, 0, 2}, {1, 3, 1, 3}, {2, 4, 5, 1}: means 1, 2, 3; variances 4/3, 4/3, 10/3; M = 3, N = 4
    #   B = 4 / 2 * (1 + 0 + 1) = 4,  W = 2,  V = 3/4 * 2 + (4 / 4) * 3 * 4 = 13.5,  V / W = 6.75
    c1 = write("c1.txt", ["0.0 2.0", "0.0 2.0"], "p q")
    c2 = write("c2.txt", ["1.0,3.0", "1.0,3.0"], "p,q")
    c3 = write("c3.txt", ["2.0\t4.0", "5.0\t1.0"], "p\tq")
    assert PSRF(c1, c2, c3) == pytest.approx(6.75, rel=1e-14)
    assert PSRF(a, a) == pytest.approx(2.0 / 3.0, rel=1e-14)               # equal chains: B = 0, V / W = (N - 1) / N
    with pytest.raises(ValueError, match="at least two"):
        PSRF(a)
