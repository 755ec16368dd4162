"""The pedigree random effect, host side (no GPU): the colouring and the numpy restatement of the structured step
(tests/locpar_ped_reference.py) against the reference's dense single-site scan, the set_random(model, "ID", ped, G) contract, the
default priors, and runMCMC through the stand-in engines with the reference's demo data."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import locpar_reference as LP
import locpar_ped_reference as PR
from locpar_ped_reference import PedOracleEngine, PedOracleEngine64
from locpar_reference import LocparOracleEngine
from oracle_engine import OracleEngine
from jwas_jl_amd import api
from jwas_jl_amd.single_step import Pedigree, a_inverse, get_pedigree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo_7animals")


def _demo_ped():
    return get_pedigree(PR.DEMO_PEDIGREE, header=True)


# ---- colouring and restatement --------------------------------------------------------------------------------------------------
def test_demo_pedigree_and_structure():
    ped = _demo_ped()
    assert len(ped.ids) == 12 and set(ped.ids) == {f"a{i}" for i in range(1, 13)} and ped.f.max() > 0      # a11, a12 are inbred
    V = api.pedigree_structure(ped)
    assert V.shape == (12, 12) and V.has_sorted_indices and (V != V.T).nnz == 0 and np.all(V.diagonal() > 0)
    assert np.array_equal(V.data, V.data.astype(np.float32).astype(np.float64))       # rounded through Float32 (random_effects.jl:184)
    assert np.allclose(V.toarray(), a_inverse(ped).toarray(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("maker", ["demo", "ped200"])
def test_greedy_colouring_is_proper(maker):
    ped = _demo_ped() if maker == "demo" else PR.ped200()
    V = api.pedigree_structure(ped)
    color = PR.greedy_colors(V)
    coo = V.tocoo()
    offd = coo.row != coo.col
    assert np.all(color[coo.row[offd]] != color[coo.col[offd]])             # no two neighbours share a colour
    assert color.min() == 0 and set(color) == set(range(color.max() + 1))
    # greedy: every level holds the smallest colour none of its EARLIER neighbours holds
    for l in range(V.shape[0]):
        nb = V.indices[V.indptr[l]:V.indptr[l + 1]]
        earlier = set(color[nb[nb < l]].tolist())
        assert color[l] == min(c for c in range(len(earlier) + 1) if c not in earlier)
    if maker == "ped200":
        assert color.max() + 1 >= 4 and np.diff(V.indptr).max() > 64


def _scan_engine(t, weighted, seed=2):
    """The 200-animal pedigree, n = 300 records: per trait an intercept and the animal term (random effect 0, structured)."""
    rng = np.random.default_rng(seed)
    ped = PR.ped200()
    V = api.pedigree_structure(ped)
    q, n = len(ped.ids), 300
    e = PedOracleEngine64()
    e.load_dense(rng.standard_normal((n, 8)))
    e.setup_blocks(8)
    e.set_weights(rng.uniform(0.5, 2.0, n) if weighted else None)
    e.init_state("BayesC" if t == 1 else "MTBayesC", t)
    for k in range(t):
        e.set_residual(rng.standard_normal(n), k)
    e.locpar_begin(t)
    e.locpar_set_group_structure(0, V.indptr, V.indices, V.data)
    lev = rng.integers(0, q, n)
    for k in range(t):
        e.locpar_add_covariate(k, None)
        e.locpar_add_factor(k, lev, q, 0)
    return e, V, rng


@pytest.mark.parametrize("t,weighted", [(1, False), (1, True), (2, True)])
def test_structured_restatement_is_the_reference_scan(t, weighted):
    """A = X'WX + kron(Gi, V) (one trait: vare Gi V) and b assembled densely, Gibbs(A, x, b[, vare]) of solver.jl:143-162 with the
    equations visited term by term and, within the animal term, colour by colour, fed the same normals: sol agrees to 1e-12."""
    e, V, rng = _scan_engine(t, weighted)
    sol0 = rng.standard_normal(e.locpar_size())
    e.locpar_set_sol(sol0)
    Rinv = np.linalg.inv(np.array([[1.0, 0.3], [0.3, 2.0]]))
    Rinv = (Rinv + Rinv.T) / 2
    Gi = [np.array([[2.5]])] if t == 1 else [np.array([[2.0, -0.7], [-0.7, 1.5]])]
    vare = 1.7
    A, b = PR.dense_mme_structured(e._lp_terms, e._lp_groups, {0: V}, e._lp_w, e.r.copy(), sol0, vare=vare, Rinv=Rinv, Gi=Gi)
    z = np.concatenate([LP.locpar_normal(np.arange(T.nlevels), 3, j, T.trait, 11) for j, T in enumerate(e._lp_terms)])
    color = e.locpar_group_colors(0)
    order = []
    for T in e._lp_terms:
        lv = np.arange(T.nlevels) if T.group < 0 else np.argsort(color, kind="stable")
        order += list(T.off + lv)
    ref = PR.reference_scan_in_order(A, sol0, b, z, order, vare if t == 1 else None)
    st = e.locpar_step(iteration=3, seed=11, vare=vare if t == 1 else None, Rinv=Rinv, Gi=Gi)
    got = e.locpar_get_sol()
    print("restatement against the dense scan:", np.abs(got - ref).max() / np.abs(ref).max())
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(got - sol0).max() > 0.1
    assert (np.bincount(e._lp_terms[1].level, minlength=V.shape[0]) == 0).any()      # (animals without records: drawn from the prior)
    U = np.stack([got[T.off:T.off + T.nlevels] for T in e._lp_terms if T.group == 0])
    assert np.allclose(st["utu"][0], U @ V.toarray() @ U.T, rtol=1e-12)


def test_exact_posterior_of_the_structured_step():
    """The issue's CPU experiment: intercept + the 200-animal term, weights, fixed variances, 4 000 steps after 200: every one of
    the 201 chain means within 5 batch-means standard errors (40 batches) of the solve of the mixed model equations."""
    case = PR.posterior_case()
    z = PR.posterior_z(PR.posterior_setup(PedOracleEngine64(), case), case)
    print("exact posterior of the structured step: worst z", round(float(z.max()), 2))
    assert z.shape == (201,) and z.max() <= 5.0


def test_standin_structure_contract():
    e, V, _ = _scan_engine(1, False)
    with pytest.raises(RuntimeError):
        e.locpar_set_group_structure(0, V.indptr, V.indices, V.data)         # a member exists
    bad = V.copy().tolil()
    bad[3, 0] = 0.25
    bad = bad.tocsr()
    with pytest.raises(ValueError):
        e.locpar_set_group_structure(1, bad.indptr, bad.indices, bad.data)   # asymmetric
    e.locpar_set_group_structure(1, V.indptr, V.indices, V.data)
    with pytest.raises(ValueError):
        e.locpar_add_factor(0, np.zeros(e.n, dtype=np.int32), 7, 1)          # another nlevels
    assert PedOracleEngine.locpar_structure_estimate_bytes(50000, 300000) < 5e6


# ---- set_random -------------------------------------------------------------------------------------------------------------------
def _model(eq, method="BayesC", **kw):
    ph = pd.read_csv(os.path.join(DEMO, "phenotypes.txt"), na_values=["NA"])
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(os.path.join(DEMO, "genotypes.txt"), method=method, Pi=0.0 if "\n" in eq else 0.5, **kw)
        model = api.build_model(eq)
    return model, ph


def test_set_random_pedigree_contract():
    ped = _demo_ped()
    model, ph = _model("y1 = intercept + x1 + ID + geno\ny3 = intercept + ID + geno")
    G = np.array([[2.0, 0.5], [0.5, 1.0]])
    with pytest.raises(ValueError, match="^The covariance matrix is not positive definite.$"):
        api.set_random(model, "ID", ped, np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match=r"should be a 2 x 2 matrix"):
        api.set_random(model, "ID", ped, 1.0)
    with pytest.raises(NotImplementedError, match="reference"):
        api.set_random(model, "ID", G, Vinv=np.eye(12), names=ped.ids)        # Vinv / names stay rejected
    with pytest.raises(NotImplementedError, match="reference"):
        api.set_random(model, "ID x1", ped, np.eye(3))                        # several names in one call
    with pytest.raises(NotImplementedError, match="reference"):
        api.set_random(model, "ϵ", ped, 1.0)
    assert model.rndTrmVec == [] and model.ped is False and model.pedTrmVec is False
    api.set_random(model, "ID", ped, G, df=5)
    (eff,) = model.rndTrmVec
    assert eff.randomType == "A" and eff.term_array == ["y1:ID", "y3:ID"] == model.pedTrmVec and model.ped is ped
    assert eff.names == ped.ids and eff.traits == [0, 1]
    assert float(eff.Gi.df) == 7.0 and np.array_equal(eff.Gi.scale, G * (7 - 2 - 1))       # df = Float32(df) + k, scale = G (df - k - 1)
    assert np.allclose(eff.Gi.val, np.linalg.inv(G), rtol=1e-6) and np.array_equal(eff.Gi.val, eff.Gi.val.T)
    assert sp.issparse(eff.Vinv) and eff.Vinv.shape == (12, 12) and eff.Vinv.dtype == np.float64
    with pytest.raises(ValueError, match="already a random effect"):
        api.set_random(model, "ID", ped, G)
    model, ph = _model("y1 = intercept + ID + dam + geno")
    api.set_random(model, "ID", ped)                                           # G = False: the default prior
    assert model.rndTrmVec[0].Gi.val is False
    with pytest.raises(ValueError, match="one pedigree"):
        api.set_random(model, "dam", ped, 1.0)
    api.set_random(model, "dam", 0.5)                                          # an i.i.d. effect next to it is fine
    assert [e.randomType for e in model.rndTrmVec] == ["A", "I"]


def _run(model, ph, folder, engine, **kw):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        out = api.runMCMC(model, ph, chain_length=kw.pop("chain_length", 30), burnin=kw.pop("burnin", 10), seed=kw.pop("seed", 5),
                          output_folder=str(folder), _engine=engine, block_size=64, **kw)
    out["_stdout"] = buf.getvalue()
    return out


def test_default_priors_with_a_pedigree_effect(tmp_path):
    """input_data_validation.jl:296-370: the pedigree effect counts in genetic_random_count -- varg is halved for the markers'
    default genetic variance and is the effect's default G; it does not enter nongenetic_random_count (the residual prior stays)."""
    ped = _demo_ped()
    model, ph = _model("y1 = intercept + ID + geno")
    pv = np.var(ph["y1"].dropna().to_numpy()[:4], ddof=1)
    _run(model, ph, tmp_path / "fixed", LocparOracleEngine("block"), chain_length=4, burnin=0, location_parameters="device")
    assert np.isclose(float(model.M[0].genetic_variance.val), pv * 0.5, rtol=1e-6)
    assert np.isclose(float(model.R.scale) * 4 / 2, np.float32(pv * 0.5), rtol=1e-6)
    model, ph = _model("y1 = intercept + ID + geno")
    api.set_random(model, "ID", ped)
    _run(model, ph, tmp_path / "ped", PedOracleEngine("block"), chain_length=4, burnin=0)
    assert np.isclose(float(model.M[0].genetic_variance.val), pv * 0.25, rtol=1e-6)
    assert np.isclose(float(model.R.scale) * 4 / 2, np.float32(pv * 0.5), rtol=1e-6)
    eff = model.rndTrmVec[0]
    assert float(eff.Gi.df) == 5.0 and np.allclose(eff.Gi.scale, [[pv * 0.25 * 3]], rtol=1e-6)


def _recompute_ebv(folder, trait, geno_ids, ph, ped_term="ID"):
    """EBV = genotypes * marker-effect samples + polygenic samples, from the files of a run (their mean over the saved samples)."""
    g = pd.read_csv(os.path.join(DEMO, "genotypes.txt"))
    X = g.iloc[:, 1:].to_numpy(dtype=np.float64)
    alpha = np.loadtxt(folder / f"MCMC_samples_marker_effects_geno_{trait}.txt", delimiter=",", skiprows=1)
    u = pd.read_csv(folder / f"MCMC_samples_{trait}.{ped_term}.txt")
    cols = [f"{trait}:{ped_term}:{i}" for i in geno_ids]
    return ((X - X.mean(axis=0)) @ alpha.T + u[cols].to_numpy().T).mean(axis=1), u


@pytest.mark.parametrize("double_precision", [False, True])
def test_runmcmc_single_trait_pedigree_effect(tmp_path, double_precision):
    ped = _demo_ped()
    model, ph = _model("y1 = intercept + x1 + ID + geno", double_precision=double_precision)
    api.set_covariate(model, "x1")
    api.set_random(model, "ID", ped, 0.6)
    api.outputMCMCsamples(model, "ID")
    eng = PedOracleEngine64() if double_precision else PedOracleEngine("block")
    out = _run(model, ph, tmp_path / "r", eng, double_precision=double_precision)
    lines = open(tmp_path / "r" / "MCMC_samples_polygenic_effects_variance.txt").read().splitlines()
    assert lines[0] == "y1:ID_y1:ID" and len(lines) == 1 + 20
    v = np.array([float(x) for x in lines[1:]])
    assert np.all(np.isfinite(v)) and np.all(v > 0) and len(np.unique(v)) == 20
    assert not os.path.exists(tmp_path / "r" / "MCMC_samples_y1:ID_variances.txt") and "y1:ID_variances" not in out
    tab = out["polygenic effects covariance matrix"]
    assert list(tab["Covariance"]) == ["y1:ID_y1:ID"] and np.isclose(tab["Estimate"][0], v.mean()) and tab["SD"][0] > 0
    assert os.path.exists(tmp_path / "r" / "polygenic_effects_covariance_matrix.txt")
    lp = out["location parameters"]
    assert list(zip(lp["Effect"], lp["Level"])) == [("intercept", "intercept"), ("x1", "x1")] + [("ID", i) for i in ped.ids]
    assert np.all(np.isfinite(lp["Estimate"])) and np.all(lp["SD"] > 0)
    ebv = out["EBV_y1"]
    want, u = _recompute_ebv(tmp_path / "r", "y1", list(ebv["ID"]), ph)
    assert u.shape == (20, 12) and list(u.columns) == [f"y1:ID:{i}" for i in ped.ids]
    assert np.allclose(ebv["EBV"], want, rtol=1e-5, atol=1e-6)
    assert np.abs(u.to_numpy()).mean() > 1e-3                                   # (the polygenic part is not a zero column)


def test_runmcmc_two_traits_pedigree_effect(tmp_path):
    ped = _demo_ped()
    model, ph = _model("y1 = intercept + ID + geno\ny3 = intercept + ID + geno")
    G = np.array([[0.8, 0.2], [0.2, 0.5]])
    api.set_random(model, "ID", ped, G)
    api.outputMCMCsamples(model, "ID")
    out = _run(model, ph, tmp_path / "r", PedOracleEngine("block"))
    lines = open(tmp_path / "r" / "MCMC_samples_polygenic_effects_variance.txt").read().splitlines()
    assert lines[0] == "y1:ID_y1:ID,y1:ID_y3:ID,y3:ID_y1:ID,y3:ID_y3:ID" and len(lines) == 1 + 20
    V = np.array([[float(x) for x in ln.split(",")] for ln in lines[1:]]).reshape(20, 2, 2)
    assert np.all(np.linalg.eigvalsh(V) > 0) and np.allclose(V, V.transpose(0, 2, 1), rtol=1e-5)
    tab = out["polygenic effects covariance matrix"]
    assert list(tab["Covariance"]) == lines[0].split(",") and np.allclose(tab["Estimate"], V.reshape(20, 4).mean(axis=0))
    lp = out["location parameters"]
    assert list(lp["Trait"]) == ["y1"] * 13 + ["y3"] * 13 and list(lp["Level"]) == (["intercept"] + ped.ids) * 2
    for tr in ("y1", "y3"):
        ebv = out[f"EBV_{tr}"]
        want, _ = _recompute_ebv(tmp_path / "r", tr, list(ebv["ID"]), ph)
        assert np.allclose(ebv["EBV"], want, rtol=1e-5, atol=1e-6)
    assert "heritability" in out and np.all(np.isfinite(out["heritability"]["Estimate"]))


def test_pedigree_checks_and_what_still_raises(tmp_path):
    ped = _demo_ped()
    small = Pedigree(["a1", "a2", "a3"], [-1, -1, -1], [-1, -1, -1])
    model, ph = _model("y1 = intercept + ID + geno")
    api.set_random(model, "ID", small, 0.5)
    with pytest.raises(ValueError, match="^Not all genotyped individuals are found in pedigree!$"):
        _run(model, ph, tmp_path / "a", PedOracleEngine("block"))
    # phenotyped individuals outside the pedigree are dropped with the reference's note
    model, ph = _model("y1 = intercept + ID + geno")
    api.set_random(model, "ID", ped, 0.5)
    extra = pd.concat([ph, pd.DataFrame({"ID": ["zz9"], "y1": [1.0], "x1": [0.5]})], ignore_index=True)
    out = _run(model, extra, tmp_path / "b", PedOracleEngine("block"), chain_length=4, burnin=0)
    assert "1 phenotyped individuals are not included in the pedigree. These are removed from the analysis." in out["_stdout"]
    # a pedigree factor that is not the ID column: a value that is no pedigree ID cannot remain
    model, ph = _model("y1 = intercept + x3 + geno")
    api.set_random(model, "x3", ped, 0.5)
    with pytest.raises(ValueError, match="not found in the pedigree"):
        _run(model, ph, tmp_path / "c", PedOracleEngine("block"))
    model, ph = _model("y1 = intercept + ID + geno")
    api.set_random(model, "ID", ped, 0.5)
    with pytest.raises(NotImplementedError, match='location_parameters="host" has no random effects'):
        _run(model, ph, tmp_path / "d", PedOracleEngine("block"), location_parameters="host")
    with pytest.raises(NotImplementedError, match="locpar_set_group_structure"):
        _run(model, ph, tmp_path / "e", LocparOracleEngine("block"))                   # an engine without the structure call
    with pytest.raises(NotImplementedError, match="starting values for location parameters"):
        _run(model, ph, tmp_path / "f", PedOracleEngine("block"), starting_value=np.zeros(3))
    model, ph = _model("y1 = intercept + ID + geno\ny2 = intercept + ID + geno")            # a5 has no y2
    api.set_random(model, "ID", ped, np.eye(2))
    with pytest.raises(NotImplementedError, match="complete multi-trait records"):
        _run(model, ph, tmp_path / "g", PedOracleEngine("block"))


def test_models_without_a_pedigree_effect_keep_their_chain(tmp_path):
    """Same seed, same posterior means, with the plain stand-in and with the one that knows structures: an i.i.d. model never
    touches the new code."""
    outs = []
    for name, eng in (("a", LocparOracleEngine("block")), ("b", PedOracleEngine("block"))):
        model, ph = _model("y1 = intercept + x1 + x2 + geno")
        api.set_covariate(model, "x1")
        api.set_random(model, "x2", 0.6)
        outs.append(_run(model, ph, tmp_path / name, eng))
    for key in ("location parameters", "marker effects geno", "y1:x2_variances", "residual variance", "EBV_y1"):
        col = "EBV" if key.startswith("EBV") else "Estimate"
        assert np.array_equal(outs[0][key][col].to_numpy(), outs[1][key][col].to_numpy())
    # ... and the figures themselves are the ones the parent commit gave for this model and seed (tests/test_locpar_host.py pins
    # the files' shape; here the default-prior arithmetic: one i.i.d. effect, no pedigree effect -> varg = 0.5 var(y))
    pv = np.var(ph["y1"].dropna().to_numpy()[:4], ddof=1)
    model, ph = _model("y1 = intercept + x2 + geno")
    api.set_random(model, "x2")
    _run(model, ph, tmp_path / "c", PedOracleEngine("block"), chain_length=4, burnin=0)
    assert np.isclose(float(model.M[0].genetic_variance.val), pv * 0.5, rtol=1e-6)
