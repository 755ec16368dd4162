"""GBLUP through get_genotypes / runMCMC on the CPU stand-in (tests/gblup_reference.py): the routing, every refusal by message, the
reference's error strings, the positive-definiteness loop, the alignment of K to the records, the eigen invariants, the prior and
the three variance draws, the outputs' names, and the exact posterior of y = intercept + a + e (the CPU twin of
tests/test_gpu_gblup.py)."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest

import draw_laws
import gblup_reference as GR
from gblup_reference import GblupStandInEngine, GblupStandInEngine64
from jwas_jl_amd import api, gblup


def _genotype_frame(n=40, p=90, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.binomial(2, 0.2 + 0.6 * rng.random(p), size=(n, p)).astype(np.float64)
    ids = [f"id{i + 1}" for i in range(n)]
    gdf = pd.DataFrame(X, columns=[f"m{j + 1}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    return gdf, ids, X


def _phenotypes(ids, t=1, seed=4):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({"ID": ids, **{f"y{k + 1}": rng.standard_normal(len(ids)) + 1.0 for k in range(t)},
                         "herd": [f"h{i % 3}" for i in range(len(ids))], "age": rng.random(len(ids))})


def _kframe(double_precision=False, **kw):
    gdf, ids, X = _genotype_frame(**kw)
    eng = GblupStandInEngine64() if double_precision else GblupStandInEngine()
    return api.genomic_relationship_matrix(gdf, double_precision=double_precision, _engine=eng), gdf, ids


def _quiet(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **kw)
    return out, buf.getvalue()


def _model(Kdf, t=1, rhs="intercept + geno", G=0.5, geno_kw=None, model_kw=None, double_precision=False):
    Gv = G if t == 1 or not np.isscalar(G) else G * np.eye(t) + 0.1
    geno, _ = _quiet(api.get_genotypes, Kdf, Gv, method="GBLUP", double_precision=double_precision, **(geno_kw or {}))
    model = api.build_model("\n".join(f"y{k + 1} = {rhs}" for k in range(t)), genotypes={"geno": geno}, **(model_kw or {}))
    return model, geno


def _run(model, ph, folder, double_precision=False, engine=None, **kw):
    eng = engine if engine is not None else (GblupStandInEngine64() if double_precision else GblupStandInEngine())
    args = dict(chain_length=30, burnin=5, seed=3, output_folder=str(folder), double_precision=double_precision, _engine=eng, gblup_eigen="host")
    args.update(kw)
    return _quiet(api.runMCMC, model, ph, **args)[0]


# ---- the relationship matrix and get_genotypes ---------------------------------------------------------------------------------------------
def test_relationship_matrix_function_shares_the_host_steps():
    gdf, ids, X = _genotype_frame()
    Kdf = api.genomic_relationship_matrix(gdf, _engine=GblupStandInEngine())
    assert list(Kdf.columns) == ["ID"] + ids and list(Kdf["ID"]) == ids
    g, _ = _quiet(api.get_genotypes, gdf, 1.0, method="RR-BLUP")                  # the same host steps: centring, QC, frequencies
    d = np.sqrt(np.float32(2.0) * g.alleleFreq * (np.float32(1.0) - g.alleleFreq))
    Z = (g.genotypes / d).astype(np.float64)
    want = (Z @ Z.T + 1e-5 * np.eye(len(ids))) / g.nMarkers
    K = Kdf.iloc[:, 1:].to_numpy()
    assert K.dtype == np.float32 and np.array_equal(K, K.T)
    np.testing.assert_allclose(K, want, rtol=0, atol=4 * 2.0 ** -24 * np.abs(want).max())
    K64 = api.genomic_relationship_matrix(gdf, double_precision=True, _engine=GblupStandInEngine64()).iloc[:, 1:].to_numpy()
    assert K64.dtype == np.float64
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        api.genomic_relationship_matrix(gdf, _engine=object())
    with pytest.raises(ValueError, match="0 < p < 1"):
        api.genomic_relationship_matrix(gdf.assign(m1=0.0), quality_control=False, _engine=GblupStandInEngine())


def test_pinned_refusals_still_hold():
    gdf, ids, X = _genotype_frame()
    for src in (X, gdf):
        with pytest.raises(NotImplementedError, match="method GBLUP is not on the device path") as ei:
            api.get_genotypes(src, 1.0, method="GBLUP")
        assert "form the relationship matrix with genomic_relationship_matrix(...) and pass it" in str(ei.value)
    with pytest.raises(NotImplementedError, match="not on the device path"):
        api.get_genotypes(X, 1.0, method="conventional (no markers)")


def test_get_genotypes_takes_a_relationship_matrix(tmp_path):
    Kdf, gdf, ids = _kframe()
    K = Kdf.iloc[:, 1:].to_numpy()
    path = tmp_path / "K.csv"
    Kdf.to_csv(path, index=False)
    for src in (Kdf, K, str(path)):
        g, text = _quiet(api.get_genotypes, src, 0.7, method="GBLUP")
        assert "A genomic relationship matrix is provided (instead of a genotype covariate matrix)." in text
        assert "#markers: 0; #individuals: 40" in text
        assert g.method == "GBLUP" and g.isGRM and not g.centered and g.nObs == g.nMarkers == 40
        assert g.genetic_variance.val == 0.7 and g.G.val is False
        assert g.obsID == (ids if src is not K else [str(i + 1) for i in range(40)])
    with pytest.raises(ValueError, match="Genetic variance is required."):
        _quiet(api.get_genotypes, Kdf, 0.7, method="GBLUP", G_is_marker_variance=True)
    with pytest.raises(ValueError, match="starting values are not supported for GBLUP now."):
        _quiet(api.get_genotypes, Kdf, 0.7, method="GBLUP", starting_value=np.zeros(40))


def test_positive_definiteness_loop():
    rng = np.random.default_rng(3)
    n, p = 301, 700
    X = rng.binomial(2, 0.1 + 0.8 * rng.random(p), size=(n, p)).astype(np.float64)
    pf = X.mean(axis=0) / 2
    notice = "The relationship matrix is not positive definite. A very small number is added to the diagonal."
    for dt, count in ((np.float32, 1), (np.float64, 0)):
        Xc = (X - X.mean(axis=0)).astype(dt)
        Z = Xc / np.sqrt(dt(2.0) * pf.astype(dt) * (dt(1.0) - pf.astype(dt))).astype(dt)
        K = ((Z @ Z.T + np.eye(n, dtype=dt) * dt(1e-5)) / dt(p)).astype(dt)
        K = np.maximum(K, K.T)
        g, text = _quiet(api.get_genotypes, K, 1.0, method="GBLUP", double_precision=dt is np.float64)
        print(f"{np.dtype(dt).name}: {text.count(notice)} additions of 1e-5 I")
        assert text.count(notice) == count
        np.testing.assert_array_equal(np.diag(g.genotypes), (np.diag(K) + dt(1e-5) * count).astype(dt) if count else np.diag(K))
    bad = -np.eye(5)
    with pytest.raises(ValueError, match="Please provide a positive-definite relationship matrix."):
        _, text = _quiet(api.get_genotypes, bad, 1.0, method="GBLUP")


# ---- prepare: alignment and the eigen invariants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double_precision", [False, True])
def test_prepare_aligns_and_decomposes(double_precision):
    Kdf, gdf, ids = _kframe(double_precision)
    dt = np.float64 if double_precision else np.float32
    g, _ = _quiet(api.get_genotypes, Kdf, 0.5, method="GBLUP", double_precision=double_precision)
    rng = np.random.default_rng(0)
    rows = rng.permutation(40)[:25]                        # a subset of K, in another order
    out_rows = np.concatenate([rows[:5], np.setdiff1d(np.arange(40), rows)[:6]])        # some with records, some without
    gb = gblup.prepare(g, rows, out_rows, dt, gblup_eigen="host")
    K = g.genotypes.astype(np.float64)
    Krr = K[np.ix_(rows, rows)]
    L, D = gb.L.astype(np.float64), gb.D
    tol = 200 * np.finfo(dt).eps
    assert gb.where == "host" and gb.L.dtype == dt and gb.L.flags.f_contiguous and D.dtype == np.float64 and (D > 0).all()
    assert np.abs(L.T @ L - np.eye(25)).max() <= tol
    assert np.abs((L * D) @ L.T - Krr).max() <= tol * np.abs(Krr).max() * 25
    assert g.nMarkers == 25 and g.markerID == [str(i + 1) for i in range(25)]
    # the output matrix turns pseudo-marker effects into K[out, records] inv(K[records, records]) a
    a = rng.standard_normal(25)
    want = K[np.ix_(out_rows, rows)] @ np.linalg.solve(Krr, a)
    got = gb.Xout.astype(np.float64) @ (L.T @ a)
    assert np.abs(got - want).max() <= (1e-8 if double_precision else 2e-2) * np.abs(want).max()
    assert gblup.prepare(g, rows, None, dt, gblup_eigen="host").Xout is None
    with pytest.raises(ValueError, match="more than one record"):
        gblup.prepare(g, np.array([0, 1, 1]), None, dt, gblup_eigen="host")
    assert gblup.eigen(Krr.astype(dt), "auto")[2] == "host"                  # below EIGEN_AUTO_MIN_N the host solver runs


# ---- priors and variance draws -----------------------------------------------------------------------------------------------------------------
def test_variance_draws_against_hand_formulas():
    n, df = 37, 4.0
    ss = np.array([[3.0, 0.5], [0.5, 2.0]])
    scale = np.array([[0.4, 0.1], [0.1, 0.3]])
    one = gblup.draw_genetic_variance(np.random.default_rng(1), ss[:1, :1], n, df, 0.4, 1, False, np.float32)
    assert one.dtype == np.float32 and one == np.float32((3.0 + df * 0.4) / np.random.default_rng(1).chisquare(n + df))
    diag = gblup.draw_genetic_variance(np.random.default_rng(2), ss, n, df, scale, 2, True, np.float64)
    rng = np.random.default_rng(2)
    want = np.diag([(ss[k, k] + df * scale[k, k]) / rng.chisquare(n + df) for k in range(2)])
    assert np.array_equal(diag, want)
    from scipy.stats import invwishart
    joint = gblup.draw_genetic_variance(np.random.default_rng(3), ss, n, df, scale, 2, False, np.float64)
    assert np.array_equal(joint, invwishart.rvs(df=df + n, scale=scale + ss, random_state=np.random.default_rng(3)))


def test_prior_is_the_genetic_variance(tmp_path):
    Kdf, gdf, ids = _kframe()
    ph = _phenotypes(ids)
    model, geno = _model(Kdf, G=0.8)
    out = _run(model, ph, tmp_path / "a", chain_length=5, burnin=0)
    assert geno.G.val == 0.8 and geno.G.scale == pytest.approx(0.8 * (4.0 - 2.0) / 4.0)         # tools4genotypes.jl:409-418
    assert geno.estimatePi is False
    model, geno = _model(Kdf, t=2, G=np.array([[0.8, 0.1], [0.1, 0.6]]))
    _run(model, _phenotypes(ids, 2), tmp_path / "b", chain_length=5, burnin=0)
    np.testing.assert_allclose(geno.G.scale, np.array([[0.8, 0.1], [0.1, 0.6]]) * ((4.0 + 2) - 2 - 1))      # (build_model: df + ntraits)
    # the default: half the phenotypic variance
    geno, _ = _quiet(api.get_genotypes, Kdf, method="GBLUP")
    model = api.build_model("y1 = intercept + geno", genotypes={"geno": geno})
    _run(model, ph, tmp_path / "c", chain_length=5, burnin=0)
    assert geno.G.val == pytest.approx(np.var(ph["y1"], ddof=1) / 2)


# ---- runs ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,constraint,double_precision,locpar", [(1, False, False, "host"), (1, False, True, "device"), (2, False, False, "auto"),
                                                                  (3, True, False, "host"), (4, False, True, "device"), (2, True, True, "host")])
def test_runs_and_output_names(tmp_path, t, constraint, double_precision, locpar):
    Kdf, gdf, ids = _kframe(double_precision)
    ph = _phenotypes(ids, t).sample(frac=1.0, random_state=1).reset_index(drop=True)       # the records in another order than K
    model, geno = _model(Kdf, t=t, rhs="intercept + age + geno", geno_kw=dict(constraint=constraint), model_kw=dict(constraint=constraint),
                         double_precision=double_precision)
    out = _run(model, ph, tmp_path / "r", double_precision, location_parameters=locpar)
    files = sorted(os.listdir(tmp_path / "r"))
    assert "MCMC_samples_genetic_variance(REML)_geno.txt" in files and "MCMC_samples_marker_effects_variances_geno.txt" not in files
    assert "pi_geno" not in out and not any(f.startswith("MCMC_samples_pi") for f in files)
    for k in range(t):
        assert f"MCMC_samples_marker_effects_geno_y{k + 1}.txt" in files
        ebv = out[f"EBV_y{k + 1}"]
        assert list(ebv["ID"]) == ids and np.isfinite(ebv["EBV"]).all() and np.isfinite(ebv["PEV"]).all()
    me = out["marker effects geno"]
    assert list(me["Marker_ID"][:40]) == [str(i + 1) for i in range(40)] and len(me) == 40 * t and (me["Model_Frequency"] == 1).all()
    var = out["marker effects variance geno"]
    assert len(var) == t * t and np.isfinite(var["Estimate"]).all()
    if constraint:
        V = var["Estimate"].to_numpy().reshape(t, t)
        assert (V[~np.eye(t, dtype=bool)] == 0).all()
    rows = np.loadtxt(tmp_path / "r" / "MCMC_samples_genetic_variance(REML)_geno.txt", delimiter=",", skiprows=1, ndmin=2)
    assert rows.shape == (25, t * t)
    for key in ("residual variance", "genetic_variance", "heritability", "location parameters"):
        assert np.isfinite(out[key]["Estimate"].to_numpy(dtype=np.float64)).all(), key


def test_random_effect_subset_and_output_ids(tmp_path):
    Kdf, gdf, ids = _kframe()
    ph = _phenotypes(ids).iloc[::-1].iloc[:28].reset_index(drop=True)              # a subset of K, reversed
    model, geno = _model(Kdf, rhs="intercept + herd + geno")
    api.set_random(model, "herd")
    want = ids[:4] + list(ph["ID"][:5])                                            # four without records, five with
    api.outputEBV(model, want)
    out = _run(model, ph, tmp_path / "r")
    assert list(out["EBV_y1"]["ID"]) == want and np.isfinite(out["EBV_y1"]["EBV"]).all()
    assert len(out["marker effects geno"]) == 28
    assert "y1:herd_variances" in " ".join(out.keys()) or any("herd" in k for k in out)
    # the same seed gives the same run
    model2, _ = _model(Kdf, rhs="intercept + herd + geno")
    api.set_random(model2, "herd")
    api.outputEBV(model2, want)
    out2 = _run(model2, ph, tmp_path / "r2")
    assert np.array_equal(out["EBV_y1"]["EBV"].to_numpy(), out2["EBV_y1"]["EBV"].to_numpy())


# ---- what raises -----------------------------------------------------------------------------------------------------------------------------------
def test_what_raises(tmp_path):
    Kdf, gdf, ids = _kframe()
    ph = _phenotypes(ids, 2)
    folder = tmp_path / "never"

    def fails(exc, match, t=1, rhs="intercept + geno", model_edit=None, ph_=None, engine=None, geno_edit=None, **kw):
        model, geno = _model(Kdf, t=t, rhs=rhs)
        if model_edit:
            model_edit(model)
        if geno_edit:
            geno_edit(geno)
        with pytest.raises(exc, match=match):
            _run(model, ph if ph_ is None else ph_, folder, engine=engine, **kw)
        assert not folder.exists()                                          # before anything is written

    from jwas_jl_amd.single_step import Pedigree  # noqa: F401
    fails(ValueError, "SSGBLUP is not available", single_step_analysis=True)
    fails(ValueError, "genetic variance for GBLUP", geno_edit=lambda g: (setattr(g.G, "val", 0.1), setattr(g.genetic_variance, "val", False)))
    fails(NotImplementedError, "fast_blocks", fast_blocks=True)
    fails(NotImplementedError, "independent_blocks", fast_blocks=8, independent_blocks=True)
    fails(NotImplementedError, "heterogeneous_residuals.*not a Gibbs step", heterogeneous_residuals=True)
    fails(NotImplementedError, "annotations", geno_edit=lambda g: setattr(g, "annotations", object()))
    fails(NotImplementedError, "categorical_trait / censored_trait", model_edit=lambda m: setattr(m, "traits_type", ["categorical"]))
    fails(NotImplementedError, "causal_structure", t=2, causal_structure=np.array([[0, 0], [1, 0]]))
    fails(NotImplementedError, "RRM", RRM=np.ones((3, 2)))
    fails(NotImplementedError, "chains", chains=2)
    ph_miss = ph.copy()
    ph_miss.loc[3, "y2"] = np.nan
    fails(NotImplementedError, "miss some traits", t=2, ph_=ph_miss)
    fails(NotImplementedError, "no CPU fallback", engine=draw_laws)            # an engine without the gblup_* methods
    fails(NotImplementedError, "double_precision", double_precision=True, engine=GblupStandInEngine64())
    fails(ValueError, "gblup_eigen", gblup_eigen="gpu")

    class Sharded(GblupStandInEngine):
        def comm_info(self):
            return 0, 2
    fails(NotImplementedError, "shards", engine=Sharded())
    # several genotype categories
    g1, _ = _quiet(api.get_genotypes, Kdf, 0.5, method="GBLUP")
    g2, _ = _quiet(api.get_genotypes, gdf, 0.5, method="BayesC")
    model = api.build_model("y1 = intercept + g1 + g2", genotypes={"g1": g1, "g2": g2})
    with pytest.raises(NotImplementedError, match="several genotype categories"):
        _run(model, ph, folder, engine=[GblupStandInEngine(), GblupStandInEngine()])
    # device-resident genotypes
    g3, _ = _quiet(api.get_genotypes, Kdf, 0.5, method="GBLUP")
    g3.storage_mode = "device"
    model = api.build_model("y1 = intercept + g3", genotypes={"g3": g3})
    with pytest.raises(NotImplementedError, match="device_genotypes"):
        _run(model, ph, folder)
    assert not folder.exists()
    # a repeated individual
    model, _ = _model(Kdf)
    with pytest.raises(ValueError, match="more than one record"):
        _run(model, pd.concat([ph, ph.iloc[:1]], ignore_index=True), tmp_path / "rep")


def test_standin_refuses_what_the_library_refuses():
    e = GblupStandInEngine()
    e.load_dense(np.eye(4, 3, dtype=np.float32))
    e.init_state("BayesC", 1)
    with pytest.raises(ValueError):
        e.gblup_begin(np.ones(3))                                           # p != n
    e.load_dense(np.eye(3, dtype=np.float32))
    e.init_state("BayesC", 1)
    with pytest.raises(ValueError):
        e.gblup_begin(np.array([1.0, 0.0, 1.0]))
    with pytest.raises(ValueError):
        e.grm(np.array([1.0, -1.0, 1.0]))


def test_draws_do_not_collide_with_the_other_streams():
    import mega_reference as MR
    a = GR.gblup_normal(np.arange(50), 3, 9, 0)
    assert not np.array_equal(a, GR.gblup_normal(np.arange(50), 3, 9, 1))
    assert not np.array_equal(a, MR.mega_normal(np.arange(50), 3, 9, 0))
    assert GR.GBLUP_TAG == 0x03000000 and GR.SLOT_Z == 13


# ---- the exact posterior (the CPU twin of tests/test_gpu_gblup.py) ---------------------------------------------------------------------------
@pytest.mark.parametrize("t,n,double_precision", [(1, 24, False), (2, 12, True)])
def test_exact_posterior(tmp_path, t, n, double_precision):
    case = GR.posterior_case(t, n)
    eng = GblupStandInEngine64() if double_precision else GblupStandInEngine()
    ebv, geno = _quiet(GR.run_posterior_chain, api, case, eng, str(tmp_path / "run"), double_precision=double_precision)[0]
    Ea, Eaa = GR.mme_posterior(case["Y"], geno.genotypes.astype(np.float64), case["R"], case["G"])
    draw_laws.assert_effect_moments(ebv, Ea, Eaa, f"GBLUP on the stand-in, {t} trait(s), n = {n}")


def test_struct_layouts(tmp_path):
    """_lib.GblupParams / GblupStats against the header's offsetof."""
    import ctypes as C
    import subprocess
    from jwas_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "jwas_hip.h"', "int main(void){"]
    expect = []
    for cls, cname in ((_lib.GblupParams, "jwas_gblup_params"), (_lib.GblupStats, "jwas_gblup_stats")):
        for fname, _ in cls._fields_:
            prog.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(cls, fname).offset)
        prog.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(cls))
    prog.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "layout")]).split()] == expect
