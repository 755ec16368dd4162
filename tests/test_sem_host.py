"""runMCMC(causal_structure=...) on the CPU stand-in (tests/sem_reference.py): the reference's contract, the files, and four
properties of the step that do not depend on the device -- the residual stays (I - Lambda) y - fitted, the draws follow the exact
conditional, the coefficient of the design column (i, j) is lambda_ij at t = 4, and the indirect / overall tables are what the
saved samples give."""
import contextlib
import io
import os

import numpy as np
import pytest

import sem_reference as SR
from sem_reference import SemLocparOracleEngine, SemLocparOracleEngine64, SemOracleEngine64

FULL3 = np.tril(np.ones((3, 3)), -1)
EQ3 = "a = intercept + geno\nb = intercept + geno\nc = intercept + geno"


def _run(small_data, tmp_path, name, *, traits=("a", "b", "c"), equations=EQ3, cs=FULL3, engine=None, double=True, ph_edit=None,
         geno_kw=None, model_kw=None, nmarkers=None, **kw):
    from jwas_jl_amd import api
    gdf, ph = SR.sem_phenotypes(small_data, list(traits), nmarkers=nmarkers)
    if ph_edit is not None:
        ph_edit(ph)
    if engine is None:
        engine = SemLocparOracleEngine64() if double else SemLocparOracleEngine("block")
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC", double_precision=double, **(geno_kw or {}))       # noqa: F841 (build_model finds it)
        model = api.build_model(equations, **(model_kw or {}))
        args = dict(chain_length=30, burnin=10, seed=13, double_precision=double, causal_structure=cs, output_folder=str(tmp_path / name),
                    _engine=engine)
        args.update(kw)
        out = api.runMCMC(model, ph, **args)
    return out, model, engine, ph


# ---- 1. the contract --------------------------------------------------------------------------------------------------------------
def test_contract_errors(small_data, tmp_path):
    def fails(exc, match, name, **kw):
        with pytest.raises(exc, match=match):
            _run(small_data, tmp_path, name, nmarkers=64, **kw)

    upper = FULL3.copy(); upper[0, 2] = 1.0
    fails(ValueError, "The causal structue needs to be a lower triangular matrix.", "e1", cs=upper)
    fails(ValueError, "Causal strutures are only allowed in multi-trait analysis", "e2", traits=("a",), equations="a = intercept + geno",
          cs=np.zeros((1, 1)))
    fails(ValueError, "3 x 3", "e3", cs=np.tril(np.ones((2, 2)), -1))
    fails(ValueError, "3 x 3", "e4", cs=np.zeros(9))
    half = FULL3.copy(); half[1, 0] = 0.5
    fails(ValueError, "0 and 1", "e5", cs=half)
    diag = FULL3.copy(); diag[1, 1] = 1.0
    fails(ValueError, "zero diagonal", "e6", cs=diag)

    def one_missing(ph):
        ph.loc[5, "b"] = np.nan
    fails(ValueError, "missing", "e7", ph_edit=one_missing)

    def binary(ph):
        ph["c"] = np.digitize(ph["c"], [np.median(ph["c"])]) + 1.0
    fails(NotImplementedError, "categorical / censored", "e8", ph_edit=binary, model_kw=dict(categorical_trait=["c"]))
    fails(NotImplementedError, "heterogeneous_residuals", "e9", heterogeneous_residuals=True)
    fails(NotImplementedError, "marker starting values", "e10", geno_kw=dict(starting_value=np.full(3 * 64, 0.01), quality_control=False))
    from locpar_reference import LocparOracleEngine64
    with pytest.raises(NotImplementedError, match="no CPU fallback") as ei:
        _run(small_data, tmp_path, "e11", nmarkers=64, engine=LocparOracleEngine64())
    for m in ("sem_begin", "sem_step", "sem_accumulate", "sem_get_effects", "sem_end"):
        assert m in str(ei.value)

    class Sharded(SemLocparOracleEngine64):
        def comm_info(self):
            return (0, 2)
    fails(NotImplementedError, "marker shards", "e12", engine=Sharded())
    # the other flags of the catch-all stay rejected
    for flag in ("single_step_analysis", "RRM", "prediction_equation"):
        fails(NotImplementedError, flag, "e13" + flag, **{flag: True})
    fails(NotImplementedError, "update_priors_frequency", "e14", update_priors_frequency=5)


# ---- 2. it runs and writes every file -----------------------------------------------------------------------------------------------
def test_runs_and_writes_every_file(small_data, tmp_path):
    cs = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    out, model, engine, ph = _run(small_data, tmp_path, "r", cs=cs, missing_phenotypes=True)
    folder = tmp_path / "r"
    assert model.R.constraint is True                                    # forced (JWAS.jl:331-333)
    rv = np.loadtxt(folder / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1)
    assert rv.shape == (20, 9) and np.all(rv[:, [1, 2, 3, 5, 6, 7]] == 0.0) and np.all(rv[:, [0, 4, 8]] > 0.0)
    lam = np.loadtxt(folder / "structure_coefficient_MCMC_samples.txt", delimiter=",")
    assert lam.shape == (20, 9)                                          # no header; vec(Lambda) column-major: (i, j) at j t + i
    L = lam.reshape(20, 3, 3).transpose(0, 2, 1)
    assert np.all(L[:, np.triu_indices(3)[0], np.triu_indices(3)[1]] == 0.0) and np.all(L[:, [1, 2, 2], [0, 0, 1]] != 0.0)
    assert np.array_equal(L[-1], engine._sem_lam)
    for kind in ("indirect", "overall"):
        for tr in "abc":
            for ext in ("bin", "txt"):
                assert os.path.exists(folder / f"MCMC_samples_{kind}_marker_effects_geno_{tr}.{ext}"), (kind, tr, ext)
    for nm in ("direct", "indirect", "overall"):
        tab = np.genfromtxt(folder / f"{nm}_marker_effects_geno.txt", delimiter=",", names=True, dtype=None, encoding="utf-8")
        assert tab.dtype.names == ("Trait", "Marker_ID", "Estimate", "SD", "Model_Frequency") and len(tab) == 3 * 640
    assert os.path.exists(folder / "structure_coefficients.txt")
    sc = out["structure coefficients"]
    assert list(sc.columns) == ["Trait", "Parent", "Estimate", "SD"]
    assert list(zip(sc["Trait"], sc["Parent"])) == [("b", "a"), ("c", "a"), ("c", "b")]
    np.testing.assert_allclose(sc["Estimate"], L.mean(axis=0)[[1, 2, 2], [0, 0, 1]], rtol=1e-12)
    np.testing.assert_allclose(sc["SD"], L.std(axis=0)[[1, 2, 2], [0, 0, 1]], rtol=1e-8)
    # the data were built with b <- 0.5 a and c <- 0.5 b - 0.3 a (and a shared genetic part, which the direct paths pick up too)
    print("structure coefficients:\n", sc)
    assert sc["Estimate"][0] > 0.3 and sc["Estimate"][2] > 0.3 and sc["Estimate"][1] < sc["Estimate"][2]
    ind, ov, dr = out["indirect marker effects geno"], out["overall marker effects geno"], out["marker effects geno"]
    assert np.all(ind["Estimate"][:640] == 0.0)                           # nothing acts on the first trait
    np.testing.assert_allclose(ov["Estimate"], dr["Estimate"].to_numpy(dtype=np.float64) + ind["Estimate"], rtol=0, atol=1e-12)


# ---- 3. the residual identity -------------------------------------------------------------------------------------------------------
def test_residual_identity(small_data, tmp_path):
    """After 30 iterations of a Float64 chain (3 traits, full structure, intercept + geno, location parameters on the stand-in's
    device path so that the final intercepts can be read) the resident residual is (I - Lambda) y - fitted recomputed from the final
    lambda, intercepts and alpha.  Bound per element: 2^-53 N A.  N: an element of trait i receives, per iteration, at most one update
    per marker, one for the intercept and one per parent, each a rounded product and a rounded sum: N = 30 * 2 (p + 1 + |P_i|).
    A: the sum of the absolute terms of the recomputation, |y_i| + sum |lambda_ij y_j| + |mu_i| + sum_m |x_m alpha_im|, at the final
    state (the effects start from zero and the data are fixed, so the earlier states' terms are of this size)."""
    out, model, engine, ph = _run(small_data, tmp_path, "r", chain_length=30, burnin=0, location_parameters="device")
    t, its = 3, 30
    y = np.stack([ph[tr].to_numpy(dtype=np.float64) for tr in "abc"])
    lam, mu, alpha, X = engine._sem_lam, engine._lp_sol, engine.alpha, engine.X
    assert mu.shape == (3,) and np.all(lam[np.tril_indices(3, -1)] != 0.0)
    worst = 0.0
    for i in range(t):
        want = y[i] - lam[i] @ y - mu[i] - X @ alpha[i]
        A = np.abs(y[i]) + np.abs(lam[i]) @ np.abs(y) + abs(mu[i]) + np.abs(X) @ np.abs(alpha[i])
        N = its * 2 * (X.shape[1] + 1 + i)
        err = np.abs(engine.r[i] - want)
        bound = 2.0 ** -53 * N * A
        print(f"residual identity trait {i}: max error {err.max():.3e}, min bound {bound.min():.3e}, worst ratio {(err / bound).max():.3e}")
        worst = max(worst, (err / bound).max())
    assert worst <= 1.0


# ---- 4. the exact conditional ---------------------------------------------------------------------------------------------------------
def test_exact_conditional():
    """Everything else held fixed, 4 000 steps from one state are i.i.d. N(mu, inv(F)): every mean within 5 sqrt(V_kk / N) of mu,
    every sample variance within 5 V_kk sqrt(2 / (N - 1)) of V_kk."""
    case = SR.conditional_case()
    rows = SR.conditional_check(SR.conditional_engine(SemOracleEngine64(), case), case)
    for i, j, zm, zv in rows:
        print(f"exact conditional lambda[{i},{j}]: mean {zm:.2f} se, variance {zv:.2f} se")
    assert len(rows) == 3 and max(max(zm, zv) for _, _, zm, zv in rows) <= 5.0


# ---- 5. t = 4: the coefficient of the column (i, j) is lambda_ij ------------------------------------------------------------------
def test_t4_coefficient_order(small_data, tmp_path):
    """Structure {(3,2), (4,1)} (1-based): the reference's design holds the columns in row order [(3,2), (4,1)] and maps its draw
    back in column order [(4,1), (3,2)].  Only trait 2 drives trait 3 here, so lambda_32 is the coefficient that moves."""
    cs = np.zeros((4, 4)); cs[2, 1] = 1.0; cs[3, 0] = 1.0
    eq = "\n".join(f"{tr} = intercept + geno" for tr in "abcd")

    def drive(ph):
        rng = np.random.default_rng(5)
        n = len(ph)
        ph["a"] = rng.standard_normal(n)
        ph["b"] = rng.standard_normal(n)
        ph["c"] = 0.8 * ph["b"] + 0.3 * rng.standard_normal(n)
        ph["d"] = rng.standard_normal(n)
    out, model, engine, ph = _run(small_data, tmp_path, "r", traits=tuple("abcd"), equations=eq, cs=cs, ph_edit=drive, nmarkers=64)
    sc = out["structure coefficients"]
    print("t = 4 structure coefficients:\n", sc)
    assert list(zip(sc["Trait"], sc["Parent"])) == [("c", "b"), ("d", "a")]
    assert abs(sc["Estimate"][0] - 0.8) < 0.1 and abs(sc["Estimate"][1]) < 0.2
    lam = np.loadtxt(tmp_path / "r" / "structure_coefficient_MCMC_samples.txt", delimiter=",")
    assert lam.shape == (20, 16)
    nz = np.flatnonzero(np.any(lam != 0.0, axis=0))
    assert list(nz) == [0 * 4 + 3, 1 * 4 + 2]                             # column-major: (4,1) at 3, (3,2) at 6
    assert abs(lam[:, 6].mean() - 0.8) < 0.1 and abs(lam[:, 3].mean()) < 0.2


# ---- 6. the indirect and overall tables ----------------------------------------------------------------------------------------------
def test_indirect_and_overall_tables(small_data, tmp_path):
    """A Float32 stand-in run: the saved direct samples are the chain's Float32 effects exactly, the lambda file holds the doubles
    exactly, so the tables must be the running means of K alpha and alpha + K alpha evaluated in numpy."""
    from jwas_jl_amd import samples as SM
    out, model, engine, ph = _run(small_data, tmp_path, "r", double=False)
    folder = tmp_path / "r"
    direct = np.stack([SM.read_dense(str(folder / f"MCMC_samples_marker_effects_geno_{tr}.bin"))[0] for tr in "abc"], axis=1)   # samples x t x p
    lam = np.loadtxt(folder / "structure_coefficient_MCMC_samples.txt", delimiter=",").reshape(-1, 3, 3).transpose(0, 2, 1)
    ns, t, p = direct.shape
    assert ns == 20 and lam.shape == (20, 3, 3)
    acc = {kind: [np.zeros((t, p)) for _ in range(3)] for kind in ("indirect", "overall")}
    for s in range(ns):
        ind, ov = SR.indirect_overall(SR.indirect_matrix(lam[s]), direct[s])
        for kind, v in (("indirect", ind), ("overall", ov)):
            m, m2, f = acc[kind]
            m += (v - m) / (s + 1)
            m2 += (v * v - m2) / (s + 1)
            f += ((v != 0.0) - f) / (s + 1)
            saved = np.stack([SM.read_dense(str(folder / f"MCMC_samples_{kind}_marker_effects_geno_{tr}.bin"))[0][s] for tr in "abc"]) if s in (0, ns - 1) else None
            if saved is not None:
                assert np.array_equal(saved, v.astype(np.float32).astype(np.float64)), (kind, s)
    for kind in ("indirect", "overall"):
        tab = out[f"{kind} marker effects geno"]
        m, m2, f = acc[kind]
        d_est = np.abs(tab["Estimate"].to_numpy() - m.ravel()).max()
        d_sd = np.abs(tab["SD"].to_numpy() - np.sqrt(np.abs(m2 - m ** 2)).ravel()).max()
        d_f = np.abs(tab["Model_Frequency"].to_numpy() - f.ravel()).max()
        print(f"{kind} table against numpy: estimate {d_est:.3e}, SD {d_sd:.3e}, frequency {d_f:.3e}")
        assert d_est <= 1e-15 and d_sd <= 1e-12 and d_f <= 1e-15
        assert list(tab["Trait"]) == ["a"] * p + ["b"] * p + ["c"] * p
    assert np.any(out["indirect marker effects geno"]["Estimate"][p:] != 0.0)
