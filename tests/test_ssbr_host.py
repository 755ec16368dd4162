"""runMCMC(single_step_analysis=True, pedigree=ped) on the CPU stand-in (ssbr_reference.py): the route of ssbr.py -- validation, the
model terms J and ϵ, output IDs, the EBV identity, file names -- and its contract errors.  No GPU.  Every call of the new route
fails on a tree without it, where single_step_analysis=True raises NotImplementedError."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest

import ssbr_reference as SR
from ssbr_reference import SsOracleEngine, SsOracleEngine64
from jwas_jl_amd import api, ssbr
from jwas_jl_amd import single_step as SS


@pytest.fixture(scope="module")
def case1():
    return SR.small_case(traits=("y",))


@pytest.fixture(scope="module")
def case2():
    return SR.small_case(traits=("y1", "y2"))


def _run(case, folder, *, traits, engine, dp=False, G=1.0, model_kw=None, sampler="I", geno=None, **kw):
    with contextlib.redirect_stdout(io.StringIO()) as log:
        if geno is None:
            geno = api.get_genotypes(case["gdf"], G, method="BayesC", Pi=0.9 if len(traits) == 1 else 0.0, double_precision=dp, multi_trait_sampler=sampler)
        model = api.build_model("\n".join(f"{tr} = intercept + age + geno" for tr in traits), **(model_kw or {}))
        api.set_covariate(model, "age")
        out = api.runMCMC(model, case["ph"], single_step_analysis=True, pedigree=case["ped"], chain_length=12, burnin=4, seed=3,
                          double_precision=dp, output_folder=str(folder), _engine=engine, **kw)
    return out, model, log.getvalue()


def _table(path):
    return np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)


def _check_outputs(out, model, case, folder, traits, fitting_J=True):
    ped, non, gen = case["ped"], case["non"], case["gen"]
    nsamples = 8
    # the model gained ϵ (then J) per trait; ϵ's levels are the non-genotyped IDs in pedigree order
    for k, tr in enumerate(traits):
        names = [mt.name for mt in model.modelTerms[k]]
        assert names == ["intercept", "age", "ϵ"] + (["J"] if fitting_J else [])
    eps = [re_ for re_ in model.rndTrmVec if re_.name == "ϵ"]
    assert len(eps) == 1 and eps[0].names == non and eps[0].term_array == [f"{tr}:ϵ" for tr in traits]
    assert non == [v for v in ped.ids if v not in set(gen)]
    lp = out["location parameters"]
    for tr in traits:
        sub = lp[lp["Trait"] == tr]
        assert list(sub["Effect"]) == ["intercept", "age"] + ["ϵ"] * len(non) + (["J"] if fitting_J else [])
        assert list(sub[sub["Effect"] == "ϵ"]["Level"]) == non
    assert "heritability" not in out and "genetic_variance" not in out
    assert not os.path.exists(folder / "MCMC_samples_heritability.txt")
    # output IDs default to the whole pedigree
    for k, tr in enumerate(traits):
        ebv = out[f"EBV_{tr}"]
        assert list(ebv["ID"]) == ped.ids
    # sample files: the reference's names and shapes
    for tr in traits:
        e = _table(folder / f"MCMC_samples_{tr}.ϵ.txt")
        assert e.shape == (nsamples, len(non))
        assert open(folder / f"MCMC_samples_{tr}.ϵ.txt").readline().strip().split(",") == [f"{tr}:ϵ:{v}" for v in non]
        if fitting_J:
            assert _table(folder / f"MCMC_samples_{tr}.J.txt").reshape(-1).shape == (nsamples,)
            assert open(folder / f"MCMC_samples_{tr}.J.txt").readline().strip() == f"{tr}:J:J"
        else:
            assert not os.path.exists(folder / f"MCMC_samples_{tr}.J.txt")
    key = "_".join(f"{tr}:ϵ" for tr in traits) + "_variances"
    v = _table(folder / f"MCMC_samples_{key}.txt")
    assert v.shape == (nsamples, len(traits) ** 2) and key in out and np.all(np.isfinite(v))


class _Spy:
    """An engine whose every attribute access after construction is a test failure: the contract errors come before any engine call."""

    def __init__(self, names=ssbr.SS_METHODS):
        for nm in names:
            object.__setattr__(self, nm, self._boom)

    def _boom(self, *a, **k):
        raise AssertionError("the engine was called")

    def __getattr__(self, name):
        if name == "comm_info":
            raise AttributeError(name)
        raise AssertionError(f"the engine was touched ({name})")


def test_full_route_one_trait_float32(case1, tmp_path):
    """One trait, BayesC, Float32: terms, levels, output IDs, the EBV identity (to the Float32 rounding of a saved EBV sample; to 1e-12 in
    the Float64 test below), no heritability, files, same seed same bytes."""
    class Recording(SsOracleEngine):
        factors = []

        def locpar_add_factor(self, trait, level, nlevels, random_group=-1):
            self.factors.append((np.array(level), nlevels, random_group))
            super().locpar_add_factor(trait, level, nlevels, random_group)
    eng = Recording()
    out, model, log = _run(case1, tmp_path / "a", traits=["y"], engine=eng)
    assert "3 phenotyped individuals are not included in the pedigree" in log
    _check_outputs(out, model, case1, tmp_path / "a", ["y"])
    # records of genotyped individuals sit in no level of ϵ; the others in the level of their ID
    ids = [v for v in case1["ph"]["ID"] if v in case1["ped"].index]
    assert open(tmp_path / "a" / "IDs_for_individuals_with_phenotypes.txt").read().split() == ids
    lev = {v: i for i, v in enumerate(case1["non"])}
    (level, nlevels, group), = eng.factors
    assert nlevels == len(case1["non"]) and group == 0 and list(level) == [lev.get(v, -1) for v in ids]
    assert any(v in set(case1["gen"]) for v in ids) and any(v in lev for v in ids) and len(set(ids)) < len(ids)
    # EBV identity: from the mean marker effects, J and eps of the tables (the means of linear functions of the samples)
    non, ped = case1["non"], case1["ped"]
    lp = out["location parameters"]
    Jhat = float(lp[lp["Effect"] == "J"]["Estimate"].iloc[0])
    ehat = dict(zip(non, lp[lp["Effect"] == "ϵ"]["Estimate"].to_numpy(dtype=np.float64)))
    alpha = out["marker effects geno"]["Estimate"].to_numpy(dtype=np.float64)
    Mout = eng.X_out.astype(np.float64)
    Ai_nn, Ai_ng, _ = SR.blocks(ped, case1["gen"])
    Jn = np.linalg.solve(Ai_nn.toarray(), Ai_ng @ np.ones(len(case1["gen"])))
    Jfull = dict(zip(non + case1["gen"], np.concatenate([Jn, -np.ones(len(case1["gen"]))])))
    expect = Mout @ alpha + np.array([Jfull[v] for v in ped.ids]) * Jhat + np.array([ehat.get(v, 0.0) for v in ped.ids])
    got = out["EBV_y"]["EBV"].to_numpy(dtype=np.float64)
    # The issue asks for this identity to 1e-12.  In a Float32 run every saved EBV sample is rounded to Float32 before it enters the
    # mean (ebvs are Float32 as in the reference, whose EBVs have the genotypes' element type), so here the identity holds to that
    # rounding only: 8 ulps of Float32 at the largest EBV.  The 1e-12 bar is asserted where it can hold, in the Float64 test below.
    assert np.abs(got - expect).max() <= 8 * 2.0 ** -24 * max(1.0, np.abs(expect).max())
    # same seed, same files, byte for byte
    out2, _, _ = _run(case1, tmp_path / "b", traits=["y"], engine=SsOracleEngine())
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for nm in names:
        assert open(tmp_path / "a" / nm, "rb").read() == open(tmp_path / "b" / nm, "rb").read(), nm


def test_ebv_identity_float64_two_traits_sampler_one(case2, tmp_path):
    """Two traits, BayesC sampler I, Float64: the EBV table equals Mout alpha + J_out J + Zo eps recomputed from the tables to 1e-12."""
    eng = SsOracleEngine64()
    Gm = np.array([[1.0, 0.3], [0.3, 0.8]])
    out, model, _ = _run(case2, tmp_path / "a", traits=["y1", "y2"], engine=eng, dp=True, G=Gm)
    _check_outputs(out, model, case2, tmp_path / "a", ["y1", "y2"])
    ped, non, gen = case2["ped"], case2["non"], case2["gen"]
    Ai_nn, Ai_ng, _ = SR.blocks(ped, gen)
    Jn = np.linalg.solve(Ai_nn.toarray(), Ai_ng @ np.ones(len(gen)))
    Jfull = dict(zip(non + gen, np.concatenate([Jn, -np.ones(len(gen))])))
    lp, me = out["location parameters"], out["marker effects geno"]
    for tr in ("y1", "y2"):
        sub = lp[lp["Trait"] == tr]
        Jhat = float(sub[sub["Effect"] == "J"]["Estimate"].iloc[0])
        ehat = dict(zip(non, sub[sub["Effect"] == "ϵ"]["Estimate"].to_numpy(dtype=np.float64)))
        alpha = me[me["Trait"] == tr]["Estimate"].to_numpy(dtype=np.float64)
        expect = eng.X_out @ alpha + np.array([Jfull[v] for v in ped.ids]) * Jhat + np.array([ehat.get(v, 0.0) for v in ped.ids])
        got = out[f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64)
        assert np.abs(got - expect).max() <= 1e-12 * max(1.0, np.abs(expect).max())
    eps = next(re_ for re_ in model.rndTrmVec if re_.name == "ϵ")
    assert eps.randomType == "V" and eps.Vinv.shape == (len(non), len(non))
    # ϵ's prior covariance is the total genetic variance: the scale of its inverse-Wishart prior is G (df - t - 1), df = 4 + t
    assert float(eps.Gi.df) == 6.0 and np.allclose(eps.Gi.scale, Gm * 3.0, rtol=0, atol=0)


def test_fitting_j_vector_false_drops_j_and_nothing_else(case1, tmp_path):
    eng = SsOracleEngine()
    out, model, _ = _run(case1, tmp_path / "a", traits=["y"], engine=eng, fitting_J_vector=False)
    _check_outputs(out, model, case1, tmp_path / "a", ["y"], fitting_J=False)
    assert "J" not in set(out["location parameters"]["Effect"])


def test_output_ids_list_is_intersected_with_the_pedigree(case1, tmp_path):
    want = [case1["non"][3], case1["gen"][2], "nobody", case1["non"][0]]
    with contextlib.redirect_stdout(io.StringIO()) as log:
        geno = api.get_genotypes(case1["gdf"], 1.0, method="BayesC", Pi=0.9)
        model = api.build_model("y = intercept + geno")
        api.outputEBV(model, want)
        out = api.runMCMC(model, case1["ph"], single_step_analysis=True, pedigree=case1["ped"], chain_length=6, burnin=2, seed=3,
                          output_folder=str(tmp_path / "a"), _engine=SsOracleEngine())
    assert list(out["EBV_y"]["ID"]) == [want[0], want[1], want[3]]
    assert "Only output EBV for tesing individuals in the pedigree" in log.getvalue()


def test_j_from_the_driver_matches_the_dense_solve(case1):
    """J = [Ai_nn \\ (Ai_ng 1); -1] (make_JVecs, SSBR.jl:146-159) to 1e-12, through the driver's own preparation."""
    ped, gen, non = case1["ped"], case1["gen"], case1["non"]
    eng = SsOracleEngine64()
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(case1["gdf"], 1.7, method="BayesC", double_precision=True)
        model = api.build_model("y = intercept + geno")
        plan = ssbr.validate(model, case1["ph"], ped, fitting_J_vector=True, location_parameters="auto", double_precision=True, outputEBV=True, engine=eng)
        ph, g2, ss = ssbr.prepare(model, plan, ped, eng, double_precision=True)
    Ai_nn, Ai_ng, _ = SR.blocks(ped, gen)
    Jfull = np.concatenate([np.linalg.solve(Ai_nn.toarray(), Ai_ng @ np.ones(len(gen))), -np.ones(len(gen))])
    at = {v: i for i, v in enumerate(non + gen)}
    assert np.abs(ss.J_out - Jfull[[at[v] for v in ped.ids]]).max() <= 1e-12
    assert np.abs(ph["J"].to_numpy() - Jfull[[at[v] for v in ph["ID"]]]).max() <= 1e-12
    assert list(ph["ϵ"]) == [v if v in set(non) else "missing" for v in ph["ID"]]
    # ϵ as set_random(mme, "ϵ", G, Vinv=Ai_nn, names=...) would leave it (SSBR.jl:37): Gi = inv(Float32(G)), df = 4 + 1, scale = G (df - 2),
    # Vinv = Ai_nn rounded through Float32, exactly symmetric
    eps, = [re_ for re_ in model.rndTrmVec if re_.name == "ϵ"]
    assert eps.names == non and eps.traits == [0] and float(eps.Gi.df) == 5.0 and eps.Gi.estimate_variance is True
    assert np.array_equal(eps.Gi.val, np.linalg.inv(np.array([[np.float32(1.7)]]))) and np.array_equal(eps.Gi.scale, np.array([[1.7 * 3.0]]))
    V32 = Ai_nn.toarray().astype(np.float32).astype(np.float64)
    assert np.array_equal(eps.Vinv.toarray(), (V32 + V32.T) * 0.5) and np.array_equal(eps.Vinv.toarray(), eps.Vinv.toarray().T)
    assert g2.storage_mode == "device" and g2.obsID == list(ph["ID"]) and eng.X.shape == (len(ph), 70) and eng.X_out.shape == (len(ped.ids), 70)
    # the imputed matrix is [Mn; Mg] of the dense solve
    Mg = geno.genotypes[[geno.obsID.index(v) for v in gen], :]
    full = np.vstack([np.linalg.solve(Ai_nn.toarray(), -(Ai_ng @ Mg)), Mg])
    assert np.abs(eng.X - full[[at[v] for v in ph["ID"]]]).max() <= 1e-12


def test_contract_errors_come_before_any_engine_call_or_folder(case1, tmp_path):
    ped, gdf, ph = case1["ped"], case1["gdf"], case1["ph"]
    count = [0]

    def fails(exc, match, *, geno_kw=None, model_eq="y = intercept + geno", model_kw=None, prep=None, ph_=None, engine="spy", G=1.0, **kw):
        count[0] += 1
        folder = tmp_path / f"e{count[0]}"
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, G, method="BayesC", **(geno_kw or {}))
            model = api.build_model(model_eq, **(model_kw or {}))
            if prep:
                prep(model)
            kw.setdefault("pedigree", ped)
            with pytest.raises(exc, match=match):
                api.runMCMC(model, ph if ph_ is None else ph_, single_step_analysis=True, chain_length=5, output_folder=str(folder),
                            _engine=_Spy() if engine == "spy" else engine, **kw)
        assert not folder.exists()

    sub = SS.Pedigree(ped.ids[:60], ped.sire[:60], ped.dam[:60])
    fails(ValueError, "Not all genotyped individuals are found in pedigree!", pedigree=sub)
    fails(ValueError, "All phenotyped individuals arer genotyped. Do not run single step analysis.", ph_=ph[ph["ID"].isin(case1["gen"])].reset_index(drop=True))
    fails(ValueError, "Please input the genetic variance", G=False)
    fails(NotImplementedError, "location_parameters", location_parameters="host")
    fails(NotImplementedError, "set_random", model_eq="y = intercept + ID + geno", prep=lambda m: api.set_random(m, "ID", ped, 0.3))
    fails(NotImplementedError, "categorical_trait", model_kw=dict(categorical_trait=["y"]))
    fails(NotImplementedError, "censored_trait", model_kw=dict(censored_trait=["y"]))
    fails(NotImplementedError, "starting_value", geno_kw=dict(starting_value=np.zeros(70)))
    fails(NotImplementedError, "causal_structure", model_eq="y = intercept + geno\nage = intercept + geno", G=np.eye(2),
          causal_structure=np.array([[0.0, 0.0], [1.0, 0.0]]))

    class NoSession:
        pass
    fails(NotImplementedError, r"ss_begin, ss_set_rows, ss_impute, ss_solve_host, ss_end missing\); the package has no CPU fallback", engine=NoSession())

    class Sharded(SsOracleEngine):
        def comm_info(self):
            return (0, 2)
    fails(NotImplementedError, "shards", engine=Sharded())
    fails(TypeError, "single_step.Pedigree", pedigree="pedigree.txt")
    ph_miss = case1["ph"].copy()
    fails(ValueError, "Phenotypes for y are not found", ph_=ph_miss.drop(columns=["y"]))


def test_stream_and_device_genotypes_inputs_are_refused(case1, tmp_path):
    from jwas_jl_amd import streaming as S
    ped, gen = case1["ped"], case1["gen"]
    prefix = S.prepare_streaming_genotypes(case1["G"], tmp_path / "st", obs_ids=gen, marker_ids=list(case1["gdf"].columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, 1.0, method="BayesC", storage="stream")
        model = api.build_model("y = intercept + geno")
        with pytest.raises(ValueError, match="storage=:stream MVP does not support single_step_analysis."):
            api.runMCMC(model, case1["ph"], single_step_analysis=True, pedigree=ped, output_folder=str(tmp_path / "s"), _engine=_Spy())
        eng = SsOracleEngine()
        eng.load_dense(case1["G"].astype(np.float32))
        eng.setup_blocks(64)
        geno = api.device_genotypes(eng, 1.0, method="BayesC", obsID=gen, alleleFreq=np.full(70, 0.5), sum2pq=35.0)
        model = api.build_model("y = intercept + geno")
        with pytest.raises(NotImplementedError, match="device_genotypes"):
            api.runMCMC(model, case1["ph"], single_step_analysis=True, pedigree=ped, output_folder=str(tmp_path / "d"), _engine=eng)
    assert not (tmp_path / "s").exists() and not (tmp_path / "d").exists()


def test_refusal_without_a_pedigree_keeps_its_text(case1, tmp_path):
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(case1["gdf"], 1.0, method="BayesC")
        model = api.build_model("y = intercept + geno")
    with pytest.raises(NotImplementedError) as err:
        api.runMCMC(model, case1["ph"], single_step_analysis=True, output_folder=str(tmp_path / "e"), _engine=SsOracleEngine())
    assert str(err.value) == "runMCMC(...; single_step_analysis=...) is outside the device marker path and stays on the reference"
    with pytest.raises(NotImplementedError, match="ϵ stays on the reference"):
        api.set_random(model, "ϵ", 1.0)


def test_impute_genotypes_device_solver_on_the_standin(case1):
    """impute_genotypes(solver="device") sends one factorisation and the g x chunk blocks; same matrix as the host solver."""
    ped = case1["ped"]
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(case1["gdf"], 1.0, method="BayesC")
    ids = [v for v in case1["ph"]["ID"] if v in ped.index]
    host = SS.impute_genotypes(geno, ped, ids, return_host=True)
    eng = SsOracleEngine()
    eng.alloc_dense = lambda n, p: eng.load_dense(np.zeros((n, p), dtype=np.float32))
    dev = SS.impute_genotypes(geno, ped, ids, engine=eng, solver="device", markers_per_chunk=64)
    assert dev.storage_mode == "device" and dev.device_backend is eng
    d = np.abs(eng.X.astype(np.float64) - host.genotypes.astype(np.float64))
    assert d.max() <= 2.0 ** -22 * max(1.0, np.abs(host.genotypes).max())      # (both are Float32 roundings of solves that agree to ~1e-15)
    with pytest.raises(ValueError, match="solver"):
        SS.impute_genotypes(geno, ped, ids, engine=eng, solver="gpu")
