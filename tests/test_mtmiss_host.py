"""Multi-trait records that miss some traits on the device location path, host side: the record-weighted term-wise restatement
(tests/mtmiss_reference.py) IS the reference's scan over the equations the host path assembles from the per-record Ri, the
imputation restatement IS mcmc._impute_missing_residuals fed the same normals, runMCMC through the stand-in engines for the models
that used to raise, and the host path's chain is the parent commit's bit for bit (tests/golden/mtmiss_host_chain.json)."""
import contextlib
import io
import json
import os

import numpy as np
import pandas as pd
import pytest

import locpar_ped_reference as PR
import locpar_reference as LP
import mtmiss_reference as MR
from jwas_jl_amd import api, mcmc
from jwas_jl_amd.single_step import get_pedigree
from locpar_reference import LocparOracleEngine
from locpar_ped_reference import PedOracleEngine
from mtmiss_reference import MtmissOracleEngine, MtmissOracleEngine64, MtmissPedOracleEngine, MtmissPedOracleEngine64
from oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo_7animals")
U53 = 2.0 ** -53


def _spd(t, rng, scale=1.0):
    A = rng.standard_normal((t, t))
    M = (A @ A.T / t + np.eye(t)) * scale
    return (M + M.T) / 2


def _codes(n, t, rng, incomplete=0.3):
    """About `incomplete` of the records lack at least one trait; every pattern occurs."""
    full = (1 << t) - 1
    codes = np.where(rng.random(n) < incomplete, rng.integers(1, full, n), full)
    codes[:full] = np.arange(1, full + 1)
    return codes.astype(np.int32)


def test_pattern_tables():
    """B, U, C of every code against their definitions: C[o, o] inv(R[o, o]) = I and zero elsewhere, B = R[m, o] inv(R[o, o]),
    U'U = R[m, m] - R[m, o] inv(R[o, o]) R[o, m] with U upper triangular; the full pattern and code 0 have B = U = 0."""
    rng = np.random.default_rng(1)
    for t in (2, 3, 4):
        R = _spd(t, rng)
        B, U, C = mcmc.missing_pattern_tables(R)
        assert B.shape == U.shape == C.shape == (1 << t, t, t)
        assert not B[0].any() and not U[0].any() and not C[0].any() and not B[-1].any() and not U[-1].any()
        assert np.allclose(C[-1], np.linalg.inv(R), rtol=1e-12)
        for code in range(1, (1 << t) - 1):
            o = np.array([(code >> k) & 1 for k in range(t)], dtype=bool)
            m = ~o
            no, nm = int(o.sum()), int(m.sum())
            assert np.allclose(C[code][np.ix_(o, o)] @ R[np.ix_(o, o)], np.eye(no), atol=1e-12)
            assert not C[code][m].any() and not C[code][:, m].any()
            assert np.allclose(B[code, :nm, :no], R[np.ix_(m, o)] @ np.linalg.inv(R[np.ix_(o, o)]), atol=1e-12)
            Uc = U[code, :nm, :nm]
            assert np.array_equal(Uc, np.triu(Uc))
            assert np.allclose(Uc.T @ Uc, R[np.ix_(m, m)] - B[code, :nm, :no] @ R[np.ix_(o, m)], atol=1e-12)
            assert not B[code, nm:].any() and not B[code, :, no:].any() and not U[code, nm:].any() and not U[code, :, nm:].any()


def _scan_engine(t, seed=2):
    """The 200-animal pedigree of tests/test_locpar_ped_host.py, n = 300 weighted records: per trait an intercept, a covariate, a
    fixed factor of 5 levels and an i.i.d. random one of 37 (each declared with one more level than has records) and the animal
    term (random effect 1, structured); 30 % of the records lack a trait, every pattern occurs."""
    rng = np.random.default_rng(seed)
    ped = PR.ped200()
    V = api.pedigree_structure(ped)
    q, n = len(ped.ids), 300
    e = MtmissPedOracleEngine64()
    e.load_dense(rng.standard_normal((n, 8)))
    e.setup_blocks(8)
    e.set_weights(rng.uniform(0.5, 2.0, n))
    e.init_state("MTBayesC", t)
    for k in range(t):
        e.set_residual(rng.standard_normal(n), k)
    e.locpar_begin(t)
    e.locpar_set_group_structure(1, V.indptr, V.indices, V.data)
    f5, f37, lev = rng.integers(0, 5, n), rng.integers(0, 37, n), rng.integers(0, q, n)
    for k in range(t):
        e.locpar_add_covariate(k, None)
        e.locpar_add_covariate(k, rng.standard_normal(n))
        e.locpar_add_factor(k, f5, 6, -1)
        e.locpar_add_factor(k, f37, 38, 0)
        e.locpar_add_factor(k, lev, q, 1)
    e.mtmiss_begin(_codes(n, t, rng))
    return e, V, rng


@pytest.mark.parametrize("t", [2, 3])
def test_record_weighted_restatement_is_the_reference_scan(t):
    """A = X' Ri X + prior and b = X' Ri (r + X sol) assembled densely from the per-record Ri = w_i C[code_i] exactly as the host
    path does, Gibbs(A, x, b) of solver.jl:143-162 with the equations visited term by term (the animal term colour by colour) fed
    the same normals: sol agrees with the record-weighted term-wise step to 1e-12 max|sol| (the bar of tests/test_locpar_ped_host.py,
    the stricter of the two restatement tests)."""
    e, V, rng = _scan_engine(t)
    sol0 = rng.standard_normal(e.locpar_size())
    e.locpar_set_sol(sol0)
    R0 = _spd(t, rng)
    _, _, Ctab = mcmc.missing_pattern_tables(R0)
    Gi = [_spd(t, rng, 2.0), _spd(t, rng, 0.7)]
    assert abs(Gi[0][0, 1]) > 1e-3 and abs(Gi[1][0, 1]) > 1e-3              # (off-diagonal Gi)
    observed = np.array([[(c >> k) & 1 for k in range(t)] for c in e._mt_codes], dtype=bool)
    Ri_rows = mcmc._impute_missing_residuals([e.r[k].copy() for k in range(t)], observed, R0, np.random.default_rng(0))
    assert np.array_equal(Ri_rows, Ctab[e._mt_codes])                       # the table IS getRi's RZ of every record
    Ri_rows = Ri_rows * e._lp_w[:, None, None]
    A, b = MR.dense_mme_w(e._lp_terms, e._lp_groups, {1: V}, e._lp_w, Ri_rows, e.r.copy(), sol0, Gi=Gi)
    z = np.concatenate([LP.locpar_normal(np.arange(T.nlevels), 3, j, T.trait, 11) for j, T in enumerate(e._lp_terms)])
    color = e.locpar_group_colors(1)
    order = []
    for T in e._lp_terms:
        lv = np.arange(T.nlevels) if T.group != 1 else np.argsort(color, kind="stable")
        order += list(T.off + lv)
    ref = PR.reference_scan_in_order(A, sol0, b, z, order, None)
    e.mtmiss_set_record_weights(Ctab)
    r_before = e.r.copy()
    st = e.locpar_step(iteration=3, seed=11, Rinv=None, Gi=Gi)
    got = e.locpar_get_sol()
    print("record-weighted restatement against the dense scan:", np.abs(got - ref).max() / np.abs(ref).max())
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(got - sol0).max() > 0.1
    for k in range(t):                                                      # the residual went with it
        Xk = np.zeros((e.n, len(got)))
        for T in e._lp_terms:
            if T.trait == k:
                Xk[np.arange(e.n), T.off + T.level] = T.x
        assert np.allclose(e.r[k], r_before[k] - Xk @ (got - sol0), rtol=0, atol=1e-12)
    Um = np.stack([got[T.off:T.off + T.nlevels] for T in e._lp_terms if T.group == 1])
    assert np.allclose(st["utu"][1], Um @ V.toarray() @ Um.T, rtol=1e-12)
    # switching back: the plain step of the stand-in without the mixin
    e.mtmiss_set_record_weights(None)
    Rinv = np.linalg.inv(R0)
    Rinv = (Rinv + Rinv.T) / 2
    plain = PR.PedOracleEngine64.locpar_step
    sol1, r1 = e.locpar_get_sol(), e.r.copy()
    e.locpar_step(iteration=4, seed=11, Rinv=Rinv, Gi=Gi)
    got_sol, got_r = e.locpar_get_sol(), e.r.copy()
    e.locpar_set_sol(sol1)
    e.r[:] = r1
    plain(e, iteration=4, seed=11, Rinv=Rinv, Gi=Gi)
    assert np.array_equal(got_sol, e.locpar_get_sol()) and np.array_equal(got_r, e.r)


class _FedGenerator:
    """Stands in for numpy's Generator in mcmc._impute_missing_residuals: hands out the prepared blocks of normals in order."""

    def __init__(self, blocks):
        self.blocks = list(blocks)

    def standard_normal(self, shape):
        blk = self.blocks.pop(0)
        assert blk.shape == tuple(shape)
        return blk


@pytest.mark.parametrize("t", [2, 3, 4])
def test_imputation_restatement_is_the_host_imputation(t):
    """The restatement and mcmc._impute_missing_residuals on the same normals.  Observed cells: bit for bit the input in both.
    Missing cells: the host forms (e_o inv(Ro)) Rc' + z U with matrix products, the restatement sum_j B_cj e_o,j + sum_a z_a U_ac
    with B = (inv(Ro) Rc')' -- the same products of doubles associated differently; every evaluation is a sum of at most t (t + 1)
    products, so they agree within 4 t (t + 1) u (|e_o| |inv(Ro)| |Rc'| + |z| |U|), u = 2^-53."""
    rng = np.random.default_rng(5 + t)
    n = 257
    R0 = _spd(t, rng)
    codes = _codes(n, t, rng)
    observed = np.array([[(c >> k) & 1 for k in range(t)] for c in codes], dtype=bool)
    r0 = rng.standard_normal((t, n)) * 1.3
    Z = rng.standard_normal((n, t))
    blocks, bound = [], np.zeros((t, n))
    for code in np.unique(codes):
        if code == (1 << t) - 1:
            continue
        rows = np.flatnonzero(codes == code)
        pm = mcmc._missing_pattern_matrices(R0, int(code))
        blocks.append(Z[np.ix_(rows, np.flatnonzero(pm["m"]))])
        amp = np.abs(r0[pm["o"]][:, rows].T) @ np.abs(pm["Ro_inv"]) @ np.abs(pm["Rc"].T) + np.abs(blocks[-1]) @ np.abs(pm["U"])
        bound[np.ix_(np.flatnonzero(pm["m"]), rows)] = 4 * t * (t + 1) * U53 * amp.T
    res = [r0[k].copy() for k in range(t)]
    mcmc._impute_missing_residuals(res, observed, R0, _FedGenerator(blocks))
    host = np.stack(res)
    B, U, _ = mcmc.missing_pattern_tables(R0)
    mine = MR.impute(r0, codes, B, U, iteration=1, seed=1, normals=Z)
    assert np.array_equal(mine[observed.T], r0[observed.T]) and np.array_equal(host[observed.T], r0[observed.T])
    miss = ~observed.T
    ratio = float(np.max(np.abs(mine - host)[miss] / bound[miss]))
    print(f"imputation restatement against the host, t = {t}: {ratio:.3f} of the bound")
    assert ratio <= 1.0
    assert np.abs(mine - r0)[miss].min() > 0                                 # (every missing cell was redrawn)
    # the counter normals: another iteration, trait or seed gives other values; mean 0, variance 1
    z = MR.mtmiss_normal(np.arange(200000), 1, 0, 1)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    for other in (MR.mtmiss_normal(np.arange(50), 2, 0, 1), MR.mtmiss_normal(np.arange(50), 1, 1, 1), MR.mtmiss_normal(np.arange(50), 1, 0, 2),
                  LP.locpar_normal(np.arange(50), 1, 0, 0, 1)):
        assert not np.any(z[:50] == other)


def test_fixed_level_without_an_observed_record_keeps_its_sol():
    """Every record of level 3 of a fixed factor lacks trait 1: D_3 = 0 for the trait-1 term, the level is left alone (solver.jl:145)
    and its records' residuals are not touched; the same level of the trait-0 term moves."""
    rng = np.random.default_rng(9)
    n, t = 120, 2
    e = MtmissOracleEngine64()
    e.load_dense(rng.standard_normal((n, 8)))
    e.setup_blocks(8)
    e.init_state("MTBayesC", t)
    for k in range(t):
        e.set_residual(rng.standard_normal(n), k)
    lev = rng.integers(0, 5, n)
    codes = np.where(lev == 3, 1, 3)
    e.locpar_begin(t)
    for k in range(t):
        e.locpar_add_factor(k, lev, 5, -1)
    e.mtmiss_begin(codes)
    _, _, Ctab = mcmc.missing_pattern_tables(_spd(t, rng))
    e.mtmiss_set_record_weights(Ctab)
    sol0 = rng.standard_normal(10)
    e.locpar_set_sol(sol0)
    r0 = e.r.copy()
    det = []
    e.locpar_step(iteration=1, seed=3, Gi=[], details=det)
    got = e.locpar_get_sol()
    assert got[5 + 3] == sol0[5 + 3] and det[1]["D"][3] == 0.0 and not det[1]["live"][3]
    assert np.all(got[:5] != sol0[:5]) and np.all(np.delete(got[5:], 3) != np.delete(sol0[5:], 3))
    assert np.array_equal(e.r[1][lev == 3], r0[1][lev == 3]) and np.all(e.r[1][lev != 3] != r0[1][lev != 3])


def test_standin_refuses_what_the_library_refuses():
    e = MtmissOracleEngine64()
    e.load_dense(np.random.default_rng(0).standard_normal((20, 8)))
    e.setup_blocks(8)
    e.init_state("MTBayesC", 2)
    tabs = mcmc.missing_pattern_tables(np.eye(2))
    with pytest.raises(RuntimeError):
        e.mtmiss_impute(iteration=1, seed=1, B=tabs[0], U=tabs[1])           # before _begin
    with pytest.raises(RuntimeError):
        e.mtmiss_set_record_weights(tabs[2])
    for bad in (np.zeros(20), np.full(20, 4), np.ones(19)):
        with pytest.raises(ValueError):
            e.mtmiss_begin(bad.astype(np.int32))
    e.mtmiss_begin(np.full(20, 3, dtype=np.int32))
    bad = tabs[0].copy()
    bad[1, 0, 0] = np.nan
    with pytest.raises(ValueError):
        e.mtmiss_impute(iteration=1, seed=1, B=bad, U=tabs[1])
    with pytest.raises(ValueError):
        e.mtmiss_set_record_weights(bad)
    assert MtmissOracleEngine.mtmiss_estimate_bytes(50000) == 12 * 50000 + 6144


# ---- runMCMC --------------------------------------------------------------------------------------------------------------------
def _demo():
    return os.path.join(DEMO, "genotypes.txt"), pd.read_csv(os.path.join(DEMO, "phenotypes.txt"), na_values=["NA"])


def _model(eq, **kw):
    gfile, ph = _demo()
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gfile, method="BayesC", Pi=0.0)
        model = api.build_model(eq, **kw)
    return model, ph


def _run(model, ph, folder, engine, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return api.runMCMC(model, ph, chain_length=kw.pop("chain_length", 30), burnin=kw.pop("burnin", 10), seed=kw.pop("seed", 5),
                           output_folder=str(folder), _engine=engine, block_size=64, **kw)


def _finite(out, traits):
    for key in ["location parameters", "marker effects geno", "residual variance"] + [f"EBV_{tr}" for tr in traits]:
        col = "EBV" if key.startswith("EBV") else "Estimate"
        assert np.all(np.isfinite(out[key][col].to_numpy(dtype=np.float64))), key


def test_runmcmc_two_traits_random_effect_with_a_missing_trait(tmp_path):
    """a5 has no y2: raised NotImplementedError before."""
    model, ph = _model("y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno")
    api.set_random(model, "x2", np.array([[0.8, 0.2], [0.2, 0.5]]))
    out = _run(model, ph, tmp_path / "r", MtmissOracleEngine("block"))
    V = np.loadtxt(tmp_path / "r" / "MCMC_samples_y1:x2_y2:x2_variances.txt", delimiter=",", skiprows=1).reshape(20, 2, 2)
    assert np.all(np.isfinite(V)) and np.all(np.linalg.eigvalsh((V + V.transpose(0, 2, 1)) / 2) > 0)
    lp = out["location parameters"]
    assert list(lp["Trait"]) == ["y1"] * 3 + ["y2"] * 3 and list(lp["Level"]) == ["intercept", "1.0", "2.0"] * 2
    assert np.all(lp["SD"] > 0)
    _finite(out, ["y1", "y2"])
    assert np.all(np.isfinite(out["y1:x2_y2:x2_variances"]["Estimate"]))


def test_runmcmc_pedigree_effect_with_a_missing_trait(tmp_path):
    """The model tests/test_locpar_ped_host.py expects to raise with a stand-in that has no mtmiss methods."""
    ped = get_pedigree(PR.DEMO_PEDIGREE, header=True)
    model, ph = _model("y1 = intercept + ID + geno\ny2 = intercept + ID + geno")
    with contextlib.redirect_stdout(io.StringIO()):
        api.set_random(model, "ID", ped, np.eye(2))
    out = _run(model, ph, tmp_path / "r", MtmissPedOracleEngine("block"))
    V = np.loadtxt(tmp_path / "r" / "MCMC_samples_polygenic_effects_variance.txt", delimiter=",", skiprows=1)
    assert V.shape == (20, 4) and np.all(np.isfinite(V))
    lp = out["location parameters"]
    assert list(lp["Trait"]) == ["y1"] * 13 + ["y2"] * 13
    _finite(out, ["y1", "y2"])
    assert "heritability" in out and np.all(np.isfinite(out["heritability"]["Estimate"]))


def test_runmcmc_fixed_only_model_on_request(tmp_path):
    model, ph = _model("y1 = intercept + x1 + x3 + geno\ny2 = intercept + x3 + geno")
    api.set_covariate(model, "x1")
    out = _run(model, ph, tmp_path / "r", MtmissOracleEngine64(), location_parameters="device", double_precision=True)
    lp = out["location parameters"]
    assert list(lp["Level"]) == ["intercept", "x1", "f", "m", "intercept", "f", "m"]
    _finite(out, ["y1", "y2"])
    assert os.path.exists(tmp_path / "r" / "MCMC_samples_residual_variance.txt")


def test_runmcmc_three_traits_one_categorical(tmp_path):
    gfile, ph = _demo()
    ph["c"] = np.where(np.isfinite(ph["y3"]), (ph["y3"] > -1.0) + 1.0, np.nan)
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gfile, method="BayesC", Pi=0.0)
        model = api.build_model("y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno\nc = intercept + x2 + geno", categorical_trait=["c"])
    api.set_random(model, "x2", np.array([[0.8, 0.2, 0.0], [0.2, 0.5, 0.1], [0.0, 0.1, 0.6]]))
    out = _run(model, ph, tmp_path / "r", MtmissOracleEngine("block"))
    V = np.loadtxt(tmp_path / "r" / "MCMC_samples_y1:x2_y2:x2_c:x2_variances.txt", delimiter=",", skiprows=1)
    assert V.shape == (20, 9) and np.all(np.isfinite(V))
    assert os.path.exists(tmp_path / "r" / "MCMC_samples_liabilities_c.txt")
    assert len(out["location parameters"]) == 9
    _finite(out, ["y1", "y2", "c"])


# ---- unchanged behaviour --------------------------------------------------------------------------------------------------------
def test_host_chain_is_the_parent_commits_bit_for_bit(tmp_path):
    """A fixed-only model with missing traits under "auto" takes the host scan; its posterior means are those the parent commit
    produced (tests/golden/mtmiss_host_chain.json), bit for bit, after _impute_missing_residuals moved onto the shared helper."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "mtmiss_host_chain.json")))
    cases = (("two_traits", "y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno", {}),
             ("three_traits_weighted", "y1 = intercept + x1 + x3 + geno\ny2 = intercept + x3 + geno\ny3 = intercept + x1 + geno",
              {"heterogeneous_residuals": True}))
    for name, eq, kw in cases:
        model, ph = _model(eq)
        if "x1" in eq:
            api.set_covariate(model, "x1")
        out = _run(model, ph, tmp_path / name, OracleEngine("block"), **kw)
        assert set(want[name]) == {"location parameters", "residual variance", "marker effects geno"}
        for key, vals in want[name].items():
            assert [float(v) for v in out[key]["Estimate"]] == vals, (name, key)


def test_an_engine_without_the_new_methods_still_raises(tmp_path):
    model, ph = _model("y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno")
    api.set_random(model, "x2", np.eye(2))
    with pytest.raises(NotImplementedError, match="complete multi-trait records.*mtmiss_begin"):
        _run(model, ph, tmp_path / "a", LocparOracleEngine("block"))
    model, ph = _model("y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno")
    with pytest.raises(NotImplementedError, match="complete multi-trait records"):
        _run(model, ph, tmp_path / "b", PedOracleEngine("block"), location_parameters="device")


def test_abi_agreement():
    """Header, ctypes list and exports name the five entry points; the estimate is the stand-in's; the params mirror has the
    header's layout (two 32-bit words, the seed, two pointers)."""
    import ctypes as C
    from test_abi import _declared
    from jwas_jl_amd import _lib
    names = [s for s in _declared() if "mtmiss" in s]
    assert sorted(names) == sorted(["jwas_hip_mtmiss_begin", "jwas_hip_mtmiss_impute", "jwas_hip_mtmiss_set_record_weights",
                                    "jwas_hip_mtmiss_estimate_bytes", "jwas_hip_mtmiss_end"])
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(hasattr(L, s) for s in names)
    assert L.jwas_hip_mtmiss_estimate_bytes(50000) == MtmissOracleEngine.mtmiss_estimate_bytes(50000)
    assert C.sizeof(_lib.MtmissParams) == 32 and [getattr(_lib.MtmissParams, f).offset for f, _ in _lib.MtmissParams._fields_] == [0, 4, 8, 16, 24]
