"""Location parameters on the device, host side: the term-wise restatement (tests/locpar_reference.py) IS the reference's
single-site scan, the set_random contract, runMCMC with a random effect through the stand-in engines, the exact posterior of the
step, and the layout of the new ABI structs -- all on the CPU.  The tests of the restatement, the normals, the stand-in's refusals
and the exact posterior exercise tests/locpar_reference.py alone (they define what the device is compared with); the others go
through api.set_random / runMCMC and the library's exports."""
import contextlib
import ctypes as C
import hashlib
import io
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import locpar_reference as LP
from locpar_reference import LocparOracleEngine, LocparOracleEngine64
from oracle_engine import OracleEngine
from jwas_jl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo_7animals")


def scan_case(t, weighted, seed=1):
    """n = 211: per trait an intercept, a covariate, a fixed factor of 5 levels and a random one of 37 levels, each declared with
    one more level than has records (an empty level: a zero diagonal for the fixed term, the prior alone for the random one)."""
    rng = np.random.default_rng(seed)
    n = 211
    e = LocparOracleEngine64()
    e.load_dense(rng.standard_normal((n, 8)))
    e.setup_blocks(8)
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    e.set_weights(w)
    e.init_state("BayesC" if t == 1 else "MTBayesC", t)
    for k in range(t):
        e.set_residual(rng.standard_normal(n), k)
    e.locpar_begin(t)
    f5, f37 = rng.integers(0, 5, n), rng.integers(0, 37, n)
    for k in range(t):
        e.locpar_add_covariate(k, None)
        e.locpar_add_covariate(k, rng.standard_normal(n))
        e.locpar_add_factor(k, f5, 6, -1)
        e.locpar_add_factor(k, f37, 38, 0)
    return e, rng


@pytest.mark.parametrize("t,weighted", [(1, True), (1, False), (2, True)])
def test_termwise_restatement_is_the_reference_scan(t, weighted):
    """A = X'WX + prior and b = X'W(r + X sol) assembled densely (two traits: with kron(inv(R), diag(w)) and an off-diagonal Gi),
    the scan of solver.jl:143-162 in equation order fed the same normals: sol agrees with the term-wise step to 1e-10 max|sol|."""
    e, rng = scan_case(t, weighted)
    sol0 = rng.standard_normal(e.locpar_size())
    e.locpar_set_sol(sol0)
    Rinv = np.linalg.inv(np.array([[1.0, 0.3], [0.3, 2.0]]))
    Rinv = (Rinv + Rinv.T) / 2
    Gi = [np.array([[2.5]])] if t == 1 else [np.array([[2.0, -0.7], [-0.7, 1.5]])]
    vare = 1.7
    A, b = LP.dense_mme(e._lp_terms, e._lp_groups, e._lp_w, e.r.copy(), sol0, vare=vare, Rinv=Rinv, Gi=Gi)
    assert (np.diag(A) == 0).sum() == t                     # the empty level of every fixed factor
    z = np.concatenate([LP.locpar_normal(np.arange(T.nlevels), 3, j, T.trait, 11) for j, T in enumerate(e._lp_terms)])
    ref = LP.reference_scan(A, sol0, b, z, vare if t == 1 else None)
    r_before = e.r.copy()
    st = e.locpar_step(iteration=3, seed=11, vare=vare if t == 1 else None, Rinv=Rinv, Gi=Gi)
    got = e.locpar_get_sol()
    assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.abs(got - sol0).max() > 0.1                   # (the step moved)
    # the residual went with it: r' = r - X (sol' - sol)
    for k in range(t):
        Xk = np.zeros((e.n, len(got)))
        for T in e._lp_terms:
            if T.trait == k:
                Xk[np.arange(e.n), T.off + T.level] = T.x
        assert np.allclose(e.r[k], r_before[k] - Xk @ (got - sol0), rtol=0, atol=1e-12)
    U = np.stack([got[T.off:T.off + T.nlevels] for T in e._lp_terms if T.group == 0])
    assert np.allclose(st["utu"][0], U @ U.T, rtol=1e-14)


def test_normals_do_not_collide_with_the_other_streams():
    """(level, iteration, 0x20000000 | term, 3 + 16 trait): the repetition word's tag differs from the liabilities' 0x40000000, the
    Wishart draws' 0x80000000 and the marker samplers' small counts; a different term, trait, iteration or seed gives another normal."""
    base = LP.locpar_normal(np.arange(50), 2, 1, 0, 9)
    for other in (LP.locpar_normal(np.arange(50), 3, 1, 0, 9), LP.locpar_normal(np.arange(50), 2, 2, 0, 9),
                  LP.locpar_normal(np.arange(50), 2, 1, 1, 9), LP.locpar_normal(np.arange(50), 2, 1, 0, 10)):
        assert not np.any(base == other)
    z = LP.locpar_normal(np.arange(200000), 1, 0, 0, 1)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01 and np.abs(z).max() < 8.5


# ---- set_random ---------------------------------------------------------------------------------------------------------------
def _demo():
    ph = pd.read_csv(os.path.join(DEMO, "phenotypes.txt"), na_values=["NA"])
    return os.path.join(DEMO, "genotypes.txt"), ph


def _model(eq, method="BayesC", **kw):
    gfile, ph = _demo()
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gfile, method=method, Pi=0.0 if "\n" in eq else 0.5, **kw)
        model = api.build_model(eq)
    return model, ph


def test_set_random_contract():
    model, ph = _model("y1 = intercept + x1 + x2 + geno\ny3 = intercept + x2 + geno")
    quiet = contextlib.redirect_stdout(io.StringIO())
    with pytest.raises(ValueError, match="^The covariance matrix is not positive definite.$"):
        api.set_random(model, "x2", np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match="^The covariance matrix is not positive definite.$"):
        api.set_random(model, "x2", -1.0)
    with pytest.raises(ValueError, match="^Constraint for variance of random term is not supported now.$"):
        api.set_random(model, "x2", np.eye(2), constraint=True)
    with pytest.raises(ValueError, match="^Estimate scale for variance of random term is not supported now.$"):
        api.set_random(model, "x2", np.eye(2), estimate_scale=True)
    with quiet, pytest.raises(ValueError, match="^herd is not found in model equation.$"):
        api.set_random(model, "herd", 1.0)
    with pytest.raises(ValueError, match=r"^Dimensions must match. The covariance matrix \(G\) should be a 2 x 2 matrix.\n$"):
        api.set_random(model, "x2", 1.0)
    with quiet, pytest.raises(ValueError, match=r"should be a 1 x 1 matrix"):
        api.set_random(model, "x1", np.eye(2))
    with pytest.raises(NotImplementedError, match="reference"):
        api.set_random(model, "x1 x2", np.eye(3))
    with pytest.raises(NotImplementedError, match="reference"):
        api.set_random(model, "x2", np.eye(2), Vinv=np.eye(2), names=["1", "2"])
    with pytest.raises(NotImplementedError, match="reference"):
        api.set_random(model, "ϵ", 1.0)
    assert model.rndTrmVec == []
    G = np.array([[2.0, 0.5], [0.5, 1.0]])
    api.set_random(model, "x2", G, df=5)
    with quiet:
        api.set_random(model, "x1", 0.25)                    # a scalar G is a 1 x 1 matrix; x1 is in the first equation only
    e2, e1 = model.rndTrmVec
    assert e2.term_array == ["y1:x2", "y3:x2"] and e2.traits == [0, 1] and e2.randomType == "I"
    assert float(e2.Gi.df) == 7.0 and np.array_equal(e2.Gi.scale, G * (7 - 2 - 1))        # df = Float32(df) + k, scale = G (df - k - 1)
    assert np.allclose(e2.Gi.val, np.linalg.inv(G), rtol=1e-6) and np.array_equal(e2.Gi.val, e2.Gi.val.T)
    assert e1.term_array == ["y1:x1"] and float(e1.Gi.df) == 5.0 and np.array_equal(e1.Gi.scale, [[0.25 * 3]])
    assert e1.Gi.val.shape == (1, 1) and e1.Gi.val[0, 0] == 4.0
    with pytest.raises(ValueError, match="already a random effect"):
        api.set_random(model, "x2", G)


def _run(model, ph, folder, engine, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return api.runMCMC(model, ph, chain_length=kw.pop("chain_length", 30), burnin=kw.pop("burnin", 10), seed=kw.pop("seed", 5),
                           output_folder=str(folder), _engine=engine, block_size=64, **kw)


def test_default_priors_with_a_random_term(tmp_path):
    """input_data_validation.jl:296-365: nongenetic_random_count = 1 + the set_random terms halves the DEFAULT residual prior, and
    the random effect's default G is that residual prior (Gi.scale = G (df - k - 1)); a model without one keeps today's prior."""
    model, ph = _model("y1 = intercept + x2 + geno")
    _run(model, ph, tmp_path / "fixed", OracleEngine("block"), chain_length=4, burnin=0)
    pv = np.var(ph["y1"].dropna().to_numpy()[:4], ddof=1)                  # the four records with y1 (all genotyped)
    assert np.isclose(float(model.R.scale) * 4 / 2, np.float32(pv * 0.5), rtol=1e-6)
    model, ph = _model("y1 = intercept + x2 + geno")
    api.set_random(model, "x2")
    assert model.rndTrmVec[0].Gi.val is False
    _run(model, ph, tmp_path / "random", LocparOracleEngine("block"), chain_length=4, burnin=0)
    assert np.isclose(float(model.R.scale) * 4 / 2, np.float32(pv * 0.25), rtol=1e-6)
    eff = model.rndTrmVec[0]
    assert float(eff.Gi.df) == 5.0 and np.allclose(eff.Gi.scale, [[pv * 0.25 * 3]], rtol=1e-6)      # (the phenotypes are held in Float32)


@pytest.mark.parametrize("double_precision", [False, True])
def test_runmcmc_single_trait_random_effect(tmp_path, double_precision):
    model, ph = _model("y1 = intercept + x1 + x2 + geno", double_precision=double_precision)
    api.set_covariate(model, "x1")
    api.set_random(model, "x2", 0.6)
    api.outputMCMCsamples(model, "x2")
    eng = LocparOracleEngine64() if double_precision else LocparOracleEngine("block")
    out = _run(model, ph, tmp_path / "r", eng, double_precision=double_precision)
    lines = open(tmp_path / "r" / "MCMC_samples_y1:x2_variances.txt").read().splitlines()
    assert lines[0] == "y1:x2_y1:x2" and len(lines) == 1 + 20
    v = np.array([float(x) for x in lines[1:]])
    assert np.all(np.isfinite(v)) and np.all(v > 0) and len(np.unique(v)) == 20
    lp = out["location parameters"]
    assert list(zip(lp["Effect"], lp["Level"])) == [("intercept", "intercept"), ("x1", "x1"), ("x2", "1.0"), ("x2", "2.0")]
    assert np.all(np.isfinite(lp["Estimate"])) and np.all(lp["SD"] > 0)
    tab = out["y1:x2_variances"]
    assert list(tab["Covariance"]) == ["y1:x2_y1:x2"] and np.isclose(tab["Estimate"][0], v.mean()) and tab["SD"][0] > 0
    s = np.loadtxt(tmp_path / "r" / "MCMC_samples_y1.x2.txt", delimiter=",", skiprows=1)
    assert s.shape == (20, 2) and np.allclose(s.mean(axis=0), lp["Estimate"][2:4], rtol=1e-12)
    assert os.path.exists(tmp_path / "r" / "y1:x2_variances.txt")


def test_runmcmc_two_traits_random_effect(tmp_path):
    model, ph = _model("y1 = intercept + x2 + geno\ny3 = intercept + x2 + geno")
    G = np.array([[0.8, 0.2], [0.2, 0.5]])
    api.set_random(model, "x2", G)
    out = _run(model, ph, tmp_path / "r", LocparOracleEngine("block"))
    lines = open(tmp_path / "r" / "MCMC_samples_y1:x2_y3:x2_variances.txt").read().splitlines()
    assert lines[0] == "y1:x2_y1:x2,y1:x2_y3:x2,y3:x2_y1:x2,y3:x2_y3:x2" and len(lines) == 1 + 20
    V = np.array([[float(x) for x in ln.split(",")] for ln in lines[1:]]).reshape(20, 2, 2)
    assert np.all(np.linalg.eigvalsh(V) > 0) and np.allclose(V, V.transpose(0, 2, 1), rtol=1e-5)
    lp = out["location parameters"]
    assert list(lp["Trait"]) == ["y1"] * 3 + ["y3"] * 3 and list(lp["Level"]) == ["intercept", "1.0", "2.0"] * 2
    assert np.allclose(out["y1:x2_y3:x2_variances"]["Estimate"], V.reshape(20, 4).mean(axis=0))
    # fixed variance: estimate_variance=False keeps G at its prior
    model, ph = _model("y1 = intercept + x2 + geno\ny3 = intercept + x2 + geno")
    api.set_random(model, "x2", G, estimate_variance=False)
    _run(model, ph, tmp_path / "f", LocparOracleEngine("block"))
    V = np.loadtxt(tmp_path / "f" / "MCMC_samples_y1:x2_y3:x2_variances.txt", delimiter=",", skiprows=1)
    assert np.allclose(V, np.tile(G.ravel(), (20, 1)), rtol=1e-5)


def _digest(folder):
    h = hashlib.sha256()
    for f in sorted(os.listdir(folder)):
        h.update(f.encode())
        h.update(open(os.path.join(folder, f), "rb").read())
    return h.hexdigest()


def test_host_path_is_untouched_and_auto_chooses_it(tmp_path):
    """A fixed-only model: "auto" is the host path (the numpy generator's chain, byte for byte the files of "host"); "device" on
    the same model is another chain (the counter generator) with the same tables."""
    digests = {}
    for mode in ("host", "auto", "device"):
        model, ph = _model("y1 = intercept + x1 + x3 + geno")
        api.set_covariate(model, "x1")
        out = _run(model, ph, tmp_path / mode, LocparOracleEngine("block") if mode == "device" else OracleEngine("block"),
                   location_parameters=mode)
        digests[mode] = _digest(tmp_path / mode)
        assert list(out["location parameters"]["Level"]) == ["intercept", "x1", "f", "m"]
    assert digests["host"] == digests["auto"] != digests["device"]


def test_what_raises(tmp_path):
    model, ph = _model("y1 = intercept + x2 + geno")
    api.set_random(model, "x2", 0.5)
    with pytest.raises(NotImplementedError, match="locpar_begin.*missing"):          # an injected engine without the new methods
        _run(model, ph, tmp_path / "a", OracleEngine("block"))
    with pytest.raises(NotImplementedError, match='location_parameters="host" has no random effects'):
        _run(model, ph, tmp_path / "b", LocparOracleEngine("block"), location_parameters="host")
    with pytest.raises(ValueError, match="location_parameters must be"):
        _run(model, ph, tmp_path / "c", LocparOracleEngine("block"), location_parameters="gpu")
    with pytest.raises(NotImplementedError, match="starting values for location parameters"):
        _run(model, ph, tmp_path / "d", LocparOracleEngine("block"), starting_value=np.zeros(3))
    # partially missing multi-trait records (a5 has no y2): a random term raises, a fixed-only model falls back to the host
    model, ph = _model("y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno")
    api.set_random(model, "x2", np.eye(2))
    with pytest.raises(NotImplementedError, match="complete multi-trait records"):
        _run(model, ph, tmp_path / "e", LocparOracleEngine("block"))
    model, ph = _model("y1 = intercept + x2 + geno\ny2 = intercept + x2 + geno")
    with pytest.raises(NotImplementedError, match="complete multi-trait records"):
        _run(model, ph, tmp_path / "f", LocparOracleEngine("block"), location_parameters="device")
    _run(model, ph, tmp_path / "g", OracleEngine("block"), chain_length=4, burnin=0)
    # a random covariate
    model, ph = _model("y1 = intercept + x1 + geno")
    api.set_covariate(model, "x1")
    api.set_random(model, "x1", 0.5)
    with pytest.raises(NotImplementedError, match="random covariates stay on the reference"):
        _run(model, ph, tmp_path / "h", LocparOracleEngine("block"))


def test_auto_goes_to_the_device_above_2048_levels(tmp_path):
    from jwas_jl_amd import mcmc
    assert mcmc.LOCPAR_AUTO_LEVELS == 2048
    rng = np.random.default_rng(3)
    n, p = 2100, 70
    X = rng.integers(0, 3, (n, p)).astype(np.float32)
    gdf = pd.DataFrame(X, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", [f"i{i}" for i in range(n)])
    ph = pd.DataFrame({"ID": gdf["ID"], "y": rng.standard_normal(n), "hys": [f"h{i % 2050:04d}" for i in range(n)]})
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC", Pi=0.9)
        model = api.build_model("y = intercept + hys + geno")
    with pytest.raises(NotImplementedError, match="need an engine with the locpar step"):
        _run(model, ph, tmp_path / "a", OracleEngine("block"), chain_length=2, burnin=0)
    out = _run(model, ph, tmp_path / "b", LocparOracleEngine("block"), chain_length=3, burnin=0)
    assert len(out["location parameters"]) == 2051 and np.all(np.isfinite(out["location parameters"]["Estimate"]))


def test_auto_falls_back_to_the_host_for_fixed_models_with_missing_traits(tmp_path):
    """More than 2 048 levels would send "auto" to the device, but one record misses a trait and the model has no random term: the
    run takes the host scan (an engine without the locpar methods is enough); with a random term it raises."""
    rng = np.random.default_rng(4)
    n, p = 2100, 70
    X = rng.integers(0, 3, (n, p)).astype(np.float32)
    gdf = pd.DataFrame(X, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", [f"i{i}" for i in range(n)])
    y2 = rng.standard_normal(n)
    y2[7] = np.nan
    ph = pd.DataFrame({"ID": gdf["ID"], "y1": rng.standard_normal(n), "y2": y2, "hys": [f"h{i % 2050:04d}" for i in range(n)]})
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC")
        model = api.build_model("y1 = intercept + hys + geno\ny2 = intercept + geno")
    out = _run(model, ph, tmp_path / "a", OracleEngine("block"), chain_length=2, burnin=0)
    assert len(out["location parameters"]) == 2052
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC")
        model = api.build_model("y1 = intercept + hys + geno\ny2 = intercept + geno")
        api.set_random(model, "hys", 0.5)
    with pytest.raises(NotImplementedError, match="complete multi-trait records"):
        _run(model, ph, tmp_path / "b", LocparOracleEngine("block"), chain_length=2, burnin=0)


def test_standin_refuses_what_the_library_refuses():
    e, _ = scan_case(1, False)
    with pytest.raises(ValueError):
        e.locpar_step(iteration=0, seed=1, vare=1.0, Gi=[np.eye(1)])
    with pytest.raises(ValueError):
        e.locpar_step(iteration=1, seed=1, vare=-1.0, Gi=[np.eye(1)])
    with pytest.raises(ValueError):
        e.locpar_step(iteration=1, seed=1, vare=1.0, Gi=[])
    with pytest.raises(ValueError):
        e.locpar_step(iteration=1, seed=1, vare=1.0, Gi=[np.eye(1)], first_term=3, last_term=9)
    with pytest.raises(NotImplementedError):
        e.locpar_add_factor(0, np.zeros(e.n, dtype=np.int32), 38, 0)        # a second term of trait 0 in random effect 0
    e.locpar_step(iteration=1, seed=1, vare=1.0, Gi=[np.eye(1)])
    with pytest.raises(ValueError):
        e.locpar_add_covariate(0, None)                                     # after the first use of sol
    with pytest.raises(ValueError):
        e.locpar_add_factor(0, np.full(e.n, 40), 38, -1)


def test_exact_posterior_of_the_step():
    """Variances fixed, the step is a Gibbs sampler on a Gaussian whose mean solves the MME: 4 000 steps at n = 403, every chain
    mean within 5 batch-means standard errors (40 batches) of the solve; at the committed seed the stand-in stays below 3.5."""
    case = LP.posterior_case()
    z = LP.posterior_z(LP.posterior_engine(LocparOracleEngine64(), case), case)
    print("exact posterior, z per location parameter:", np.round(z, 2))
    assert z.max() <= 3.5


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_locpar_struct_layouts(tmp_path):
    """jwas_locpar_params / jwas_locpar_stats: the header (gcc's offsetof / sizeof), the ctypes mirrors of _lib.py and the isbits
    mirrors of julia/JWASHip.jl (natural alignment) agree; the symbols are declared, listed and exported."""
    from test_abi import _declared
    from jwas_jl_amd import _lib
    src = open(os.path.join(ROOT, "julia", "JWASHip.jl")).read()
    size = {"Int32": 4, "UInt32": 4, "UInt64": 8, "Int64": 8, "Float32": 4, "Float64": 8}
    for jl, cname, mirror in (("HipLocparParams", "jwas_locpar_params", _lib.LocparParams), ("HipLocparStats", "jwas_locpar_stats", _lib.LocparStats)):
        body = re.search(r"struct %s\n(.*?)\nend" % jl, src, re.S).group(1)
        off, fields, maxal = 0, [], 1
        for line in body.strip().splitlines():
            fname, ftype = [v.strip() for v in line.strip().split("::")]
            m = re.match(r"NTuple\{(\d+),(\w+)\}", ftype)
            cnt, el = (int(m.group(1)), size[m.group(2)]) if m else (1, size[ftype])
            off = (off + el - 1) // el * el
            fields.append((fname, off))
            off += cnt * el
            maxal = max(maxal, el)
        expect = [o for _, o in fields] + [(off + maxal - 1) // maxal * maxal]
        prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "jwas_hip.h"', "int main(void){"]
        prog += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in fields]
        prog += [f'printf("%zu\\n", sizeof({cname}));', "return 0;}"]
        (tmp_path / f"{cname}.c").write_text("\n".join(prog))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / f"{cname}.c"), "-o", str(tmp_path / cname)])
        assert [int(v) for v in subprocess.check_output([str(tmp_path / cname)]).split()] == expect
        assert C.sizeof(mirror) == expect[-1] and [getattr(mirror, f).offset for f, _ in fields] == expect[:-1]
        assert [f for f, _ in mirror._fields_] == [f for f, _ in fields]
    names = [s for s in _declared() if "locpar" in s]
    assert len(names) == 11 and set(names) <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(hasattr(L, s) for s in names)
    assert L.jwas_hip_locpar_estimate_bytes(50000, 3, 50002) == LocparOracleEngine.locpar_estimate_bytes(50000, 3, 50002)
    assert L.jwas_hip_locpar_estimate_bytes(50000, 3, 50002) < 8e6
