"""Threshold (binary / ordered categorical) and censored traits on the host: the build_model / runMCMC contract, the numpy
restatement of the device's truncated-normal formula against a 50-digit evaluation, and a statistical check -- all on the CPU
through the stand-in engines of tests/liability_reference.py (the liability methods of HipEngine on OracleEngine)."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest

import liability_reference as LR
import oracle as O
from liability_reference import LiabilityOracleEngine, LiabilityOracleEngine64
from oracle_engine import OracleEngine
from jwas_jl_amd import api

# The restatement (scipy ndtr / ndtri) against the 50-digit evaluation of the same formula on mpmath_cases().  Bound per case,
# relative to max(1, |z|), in units of 2^-52: ndtri is a 4-ulp function; S(lo) and S(hi) are 2-ulp functions and the combination
# q = a - u (a - b) adds one rounding (no cancellation: b <= q <= a), so q carries an ABSOLUTE error of up to 3 ulp of a, which
# z(q) passes on with the factor 1 / phi(z).  That factor is the formula's own conditioning: a draw that lands on the far side
# of zero from the tail its branch works in (q near 1) is known only to 2^-53 / phi(z) -- 1e-14 at 3 sigma, with probability
# 1e-3; it does not show in any moment of the chain.  MEASURED on this machine (scipy 1.15.3, mpmath 1.3.0): worst relative
# error 2.2e-15 over the 400 cases, at (lo, hi) = (-5.31, Inf) with the draw at z = -2.77; 6.4e-16 over the other 399.
def case_bound(lo, hi, z):
    from scipy.special import ndtr
    mirror = lo + hi < 0
    a = float(ndtr(hi if mirror else -lo))
    phi = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    return 2.0 ** -52 * (4 + 3 * a / (phi * max(1.0, abs(z))))


def mpmath_cases(ncases=400, seed=20260):
    """One-sided and two-sided standardised intervals whose nearer bound lies up to 10 sigma from the mean on either side."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(ncases):
        b = rng.uniform(-10.0, 10.0)
        kind = i % 4
        if kind == 0:
            lo, hi = b, np.inf
        elif kind == 1:
            lo, hi = -np.inf, b
        elif kind == 2:
            lo, hi = b, b + rng.uniform(0.01, 3.0)
        else:
            lo, hi = b - rng.uniform(1e-6, 0.01), b
        cases.append((lo, hi, float(LR.liability_uniform([i], 1, 0, 0, seed)[0])))
    return cases


def restatement_error(cases):
    worst = 0.0
    for lo, hi, u in cases:
        z = float(LR.truncated_std_normal(lo, hi, u))
        zm = LR.truncated_std_normal_mp(lo, hi, u)
        assert lo <= z <= hi
        err = float(abs(z - zm) / max(1, abs(zm)))
        assert err <= case_bound(lo, hi, z), (lo, hi, u, z, err)
        worst = max(worst, err)
    return worst


def test_philox_restatement_matches_the_oracle():
    rng = np.random.default_rng(1)
    for _ in range(20):
        ctr = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64).astype(np.uint32)
        key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64).astype(np.uint32)
        got = [int(v) for v in LR.philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1])]
        assert got == [int(v) for v in O.philox(ctr, key)]
    u = LR.liability_uniform(np.arange(1000), 3, 2, 1, 77)
    assert u.min() > 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.05


def test_restatement_against_mpmath():
    worst = restatement_error(mpmath_cases())
    print(f"restatement vs 50-digit evaluation: worst relative error {worst:.3e}")


def test_truncated_normal_never_leaves_its_bounds():
    """Every branch, the exponential tail beyond ~37.5 sigma and degenerate widths included: finite and inside [lo, hi]."""
    lo = np.array([40.0, -60.0, -np.inf, 3.0, 37.4, 37.6, -np.inf, 1e3, -5.0, 0.0])
    hi = np.array([np.inf, -45.0, np.inf, 3.0 + 1e-9, np.inf, 38.0, -50.0, np.inf, 5.0, 1e-300])
    for u in (2.0 ** -53, 0.5, 1 - 2.0 ** -53):
        z = LR.truncated_std_normal(lo, hi, np.full(lo.shape, u))
        assert np.all(np.isfinite(z)) and np.all(z >= lo) and np.all(z <= hi)


def test_conditional_matches_numpy():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((4, 4))
    R = A @ A.T + np.eye(4)
    B, sd = LR.conditional(R)
    for k in range(4):
        o = [j for j in range(4) if j != k]
        np.testing.assert_allclose(B[k, o], R[k, o] @ np.linalg.inv(R[np.ix_(o, o)]), rtol=1e-12)
        np.testing.assert_allclose(sd[k] ** 2, R[k, k] - R[k, o] @ np.linalg.inv(R[np.ix_(o, o)]) @ R[o, k], rtol=1e-12)
    B0, sd0 = LR.conditional(R, init=True)
    assert not B0.any() and np.allclose(sd0 ** 2, np.diag(R))


def _simulate(n, p, seed, ncausal=30, h2=0.5):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.5, p)
    X = (rng.random((n, p)) < f).astype(np.float32) + (rng.random((n, p)) < f)
    b = np.zeros(p)
    b[rng.choice(p, ncausal, replace=False)] = rng.standard_normal(ncausal)
    g = (X - X.mean(0)) @ b
    g *= np.sqrt(h2 / g.var())
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(X, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    return gdf, ids, g, g + rng.standard_normal(n) * np.sqrt(1 - h2)


def _run(gdf, ph, eq, folder, engine, chain_length=30, burnin=10, double_precision=False, seed=5, Pi=0.9, method="BayesC", **build):
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method=method, Pi=Pi, double_precision=double_precision)
        model = api.build_model(eq, **build)
        out = api.runMCMC(model, ph, chain_length=chain_length, burnin=burnin, seed=seed, output_folder=str(folder), _engine=engine,
                          block_size=64, double_precision=double_precision)
    return model, out


def test_build_model_records_trait_types_and_keeps_refusing_unknown_keywords():
    gdf, ids, g, liab = _simulate(60, 40, 1)
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC")
    m = api.build_model("a = intercept + geno\nb = intercept + geno\nc = intercept + geno", categorical_trait=["a"], censored_trait=["c"])
    assert m.traits_type == ["categorical", "continuous", "censored"]
    assert api.build_model("a = intercept + geno").traits_type == ["continuous"]
    with pytest.raises(NotImplementedError, match="stays on the reference path"):
        api.build_model("a = intercept + geno", nonlinear_function="tanh")


@pytest.mark.parametrize("double_precision", [False, True])
def test_binary_and_categorical_contract(tmp_path, double_precision):
    n = 240
    gdf, ids, g, liab = _simulate(n, 150, 2)
    eng = LiabilityOracleEngine64 if double_precision else (lambda: LiabilityOracleEngine("block"))
    # binary: two categories become categorical(binary); R fixed at 1 and not sampled; threshold file constant
    ph = pd.DataFrame({"ID": ids, "y": (liab > 0.3) + 1.0})
    model, out = _run(gdf, ph, "y = intercept + geno", tmp_path / "bin", eng(), double_precision=double_precision, categorical_trait=["y"])
    assert model.traits_type == ["categorical(binary)"]
    assert float(model.R.val) == 1.0 and model.R.estimate_variance is False
    rv = np.loadtxt(tmp_path / "bin" / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1)
    assert np.all(rv == 1.0) and float(out["residual variance"]["Estimate"][0]) == 1.0
    th = np.loadtxt(tmp_path / "bin" / "MCMC_samples_threshold_y.txt", delimiter=",")
    L = np.loadtxt(tmp_path / "bin" / "MCMC_samples_liabilities_y.txt", delimiter=",")
    assert th.shape == (20, 3) and L.shape == (20, n)
    assert np.all(th[:, 0] == -np.inf) and np.all(th[:, 1] == 0) and np.all(th[:, 2] == np.inf)
    y = ph["y"].to_numpy()
    assert np.all(L[:, y == 1] <= 0) and np.all(L[:, y == 2] >= 0) and np.all(np.isfinite(L))
    # four categories: thresholds ordered, t1 = 0, the free ones move, liabilities between their thresholds
    y4 = np.digitize(liab, [-0.6, 0.1, 0.9]) + 1.0
    ph = pd.DataFrame({"ID": ids, "y": y4})
    model, out = _run(gdf, ph, "y = intercept + geno", tmp_path / "cat", eng(), double_precision=double_precision, categorical_trait=["y"])
    assert model.traits_type == ["categorical"] and float(model.R.val) == 1.0
    th = np.loadtxt(tmp_path / "cat" / "MCMC_samples_threshold_y.txt", delimiter=",")
    L = np.loadtxt(tmp_path / "cat" / "MCMC_samples_liabilities_y.txt", delimiter=",")
    assert th.shape == (20, 5) and np.all(th[:, 1] == 0) and np.all(np.diff(th, axis=1) > 0)
    assert len(np.unique(th[:, 2])) > 1 and len(np.unique(th[:, 3])) > 1
    tol = 0 if double_precision else 1e-6                  # (Float32 liabilities: a threshold is a double between two of them)
    for c in (1, 2, 3, 4):
        sel = y4 == c
        assert np.all(L[:, sel] >= th[:, [c - 1]] - tol) and np.all(L[:, sel] <= th[:, [c]] + tol)
    assert np.corrcoef(out["EBV_y"]["EBV"], g)[0, 1] > 0.3


def test_reference_error_texts(tmp_path):
    gdf, ids, g, liab = _simulate(80, 50, 3)
    ph = pd.DataFrame({"ID": ids, "y": np.where(liab > 0, 3.0, 1.0)})
    with pytest.raises(ValueError, match=r"For categorical trait y, the categories should be \[1, 2\] ; instead of \[1, 3\]"):
        _run(gdf, ph, "y = intercept + geno", tmp_path / "e1", LiabilityOracleEngine("block"), categorical_trait=["y"])
    ph = pd.DataFrame({"ID": ids, "y": liab})
    with pytest.raises(ValueError, match="y_l and y_u"):
        _run(gdf, ph, "y = intercept + geno", tmp_path / "e2", LiabilityOracleEngine("block"), censored_trait=["y"])
    ph = pd.DataFrame({"ID": ids, "y": (liab > 0) + 1.0})
    with pytest.raises(TypeError, match="liability_begin.*liability_end missing"):
        _run(gdf, ph, "y = intercept + geno", tmp_path / "e3", OracleEngine("block"), categorical_trait=["y"])
    ph = pd.DataFrame({"ID": ids, "y": (liab > 0) + 1.0, "weights": np.ones(len(ids))})
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC")
        model = api.build_model("y = intercept + geno", categorical_trait=["y"])
        with pytest.raises(NotImplementedError, match="heterogeneous_residuals"):
            api.runMCMC(model, ph, chain_length=2, heterogeneous_residuals=True, output_folder=str(tmp_path / "e4"),
                        _engine=LiabilityOracleEngine("block"))


def test_censored_trait_contract(tmp_path):
    n = 240
    gdf, ids, g, liab = _simulate(n, 150, 4)
    lo = np.where(liab > 0.5, 0.5, liab)
    up = np.where(liab > 0.5, np.inf, liab)
    lo[:10], up[:10] = -0.25, 0.75                                      # interval-censored records
    ph = pd.DataFrame({"ID": ids, "y_l": lo, "y_u": up})
    model, out = _run(gdf, ph, "y = intercept + geno", tmp_path / "c", LiabilityOracleEngine("block"), censored_trait=["y"])
    assert model.traits_type == ["censored"] and model.R.estimate_variance is True
    L = np.loadtxt(tmp_path / "c" / "MCMC_samples_liabilities_y.txt", delimiter=",")
    assert not os.path.exists(tmp_path / "c" / "MCMC_samples_threshold_y.txt")
    exact = lo == up
    assert exact.sum() > 50
    np.testing.assert_array_equal(L[:, exact], np.broadcast_to(lo[exact].astype(np.float32).astype(np.float64), (20, int(exact.sum()))))
    assert np.all(L >= lo.astype(np.float32)) and np.all(L <= up.astype(np.float32)) and np.all(np.isfinite(L))
    rv = np.loadtxt(tmp_path / "c" / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1)
    assert len(np.unique(rv)) > 1                                       # sampled, unlike a threshold trait's
    assert np.corrcoef(out["EBV_y"]["EBV"], g)[0, 1] > 0.5


def test_multitrait_thresholds_and_binary_variance(tmp_path):
    """Multi-trait: t1 = 0 AND t2 = 1 of a categorical trait are fixed, a binary trait keeps unit variance
    (sample_from_conditional_inverse_Wishart), nGibbs = 5 rounds per iteration, a missing category is code 0."""
    n = 200
    gdf, ids, g, liab = _simulate(n, 120, 5)
    rng = np.random.default_rng(9)
    y4 = np.digitize(liab + 0.3 * rng.standard_normal(n), [-0.6, 0.1, 0.9]) + 1.0
    y4[:7] = np.nan
    ph = pd.DataFrame({"ID": ids, "a": (liab > 0.2) + 1.0, "b": 2 * liab + 1 + 0.5 * rng.standard_normal(n), "c": y4})
    eq = "a = intercept + geno\nb = intercept + geno\nc = intercept + geno"
    spy_calls = []

    class Spy(LiabilityOracleEngine):
        def liability_sample(self, **kw):
            spy_calls.append(kw["ngibbs"])
            return super().liability_sample(**kw)

    model, out = _run(gdf, ph, eq, tmp_path / "mt", Spy("block"), Pi=0.0, categorical_trait=["a", "c"])
    assert model.traits_type == ["categorical(binary)", "continuous", "categorical"]
    assert set(spy_calls) == {5} and len(spy_calls) == 30
    th = np.loadtxt(tmp_path / "mt" / "MCMC_samples_threshold_c.txt", delimiter=",")
    assert th.shape == (20, 5) and np.all(th[:, 1] == 0) and np.all(th[:, 2] == 1) and np.all(np.diff(th, axis=1) > 0)
    assert len(np.unique(th[:, 3])) > 1
    rv = np.loadtxt(tmp_path / "mt" / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1).reshape(-1, 3, 3)
    assert np.all(rv[:, 0, 0] == 1.0) and len(np.unique(rv[:, 1, 1])) > 1
    assert np.all(np.linalg.eigvalsh(rv) > 0)
    L = np.loadtxt(tmp_path / "mt" / "MCMC_samples_liabilities_c.txt", delimiter=",")
    assert L.shape == (20, n) and np.all(np.isfinite(L))
    for c in (1, 2, 3, 4):
        sel = y4 == c
        assert np.all(L[:, sel] >= th[:, [c - 1]] - 1e-6) and np.all(L[:, sel] <= th[:, [c]] + 1e-6)


@pytest.mark.parametrize("t,binary", [(3, [0]), (4, [2]), (4, [1, 3])])
def test_conditional_inverse_wishart_is_exactly_symmetric(t, binary):
    """The device refuses an R that is not exactly symmetric; inv() of the Wishart block is symmetric up to rounding only."""
    from jwas_jl_amd.mcmc import sample_from_conditional_inverse_wishart
    rng = np.random.default_rng(17)
    A = rng.standard_normal((t, t))
    S = np.linalg.inv(A @ A.T + t * np.eye(t))
    for _ in range(500):
        for ftype in (np.float64, np.float32):
            R = sample_from_conditional_inverse_wishart(rng, 200.0, S, binary).astype(ftype)
            assert np.array_equal(R, R.T)


def test_multitrait_double_precision_chain_with_a_binary_trait(tmp_path):
    """binary + continuous + categorical in Float64 on a stand-in that refuses what the library refuses: every R the chain draws
    must be exactly symmetric and positive definite."""
    n = 160
    gdf, ids, g, liab = _simulate(n, 100, 6)
    rng = np.random.default_rng(2)
    ph = pd.DataFrame({"ID": ids, "a": (liab > 0.2) + 1.0, "b": 2 * liab + 1 + 0.5 * rng.standard_normal(n),
                       "c": np.digitize(liab + 0.3 * rng.standard_normal(n), [-0.5, 0.6]) + 1.0})
    eq = "a = intercept + geno\nb = intercept + geno\nc = intercept + geno"
    model, out = _run(gdf, ph, eq, tmp_path / "mt64", LiabilityOracleEngine64(), chain_length=60, double_precision=True, Pi=0.0,
                      categorical_trait=["a", "c"])
    rv = np.loadtxt(tmp_path / "mt64" / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1).reshape(-1, 3, 3)
    assert rv.shape[0] == 50 and np.all(rv[:, 0, 0] == 1.0) and np.array_equal(rv, rv.transpose(0, 2, 1))


def test_standin_refuses_what_the_library_refuses():
    e = LiabilityOracleEngine64()
    e.load_dense(np.zeros((5, 2)))
    e.init_state("MTBayesC", 2)
    e.liability_begin(2)
    good, skew = np.array([[1.0, 0.3], [0.3, 2.0]]), np.array([[1.0, 0.3], [0.3 + 1e-17 + 6e-17, 2.0]])
    with pytest.raises(ValueError, match="no trait"):
        e.liability_init(seed=1, R=good)
    e.set_categorical(0, np.array([1, 2, 1, 2, 0], dtype=np.int32), [-np.inf, 0.0, np.inf])
    with pytest.raises(ValueError, match="liability_init has not"):
        e.liability_sample(iteration=1, seed=1, ngibbs=5, R=good)
    assert skew[0, 1] != skew[1, 0]
    for bad, msg in ((skew, "symmetric"), (np.array([[0.0, 0.0], [0.0, 1.0]]), "positive definite"), (np.array([[1.0, np.nan], [np.nan, 1.0]]), "finite")):
        with pytest.raises(ValueError, match=msg):
            e.liability_init(seed=1, R=bad)
    e.liability_init(seed=1, R=good)
    for kw, msg in ((dict(iteration=0, ngibbs=5), "iteration"), (dict(iteration=1, ngibbs=0), "ngibbs"), (dict(iteration=1, ngibbs=1001), "ngibbs")):
        with pytest.raises(ValueError, match=msg):
            e.liability_sample(seed=1, R=good, **kw)
    with pytest.raises(ValueError, match="symmetric"):
        e.liability_sample(iteration=1, seed=1, ngibbs=5, R=skew)
    with pytest.raises(ValueError, match="positive definite"):         # (the set-up draw reads the diagonal only)
        e.liability_sample(iteration=1, seed=1, ngibbs=5, R=np.array([[1.0, 2.0], [2.0, 1.0]]))
    e.liability_sample(iteration=1, seed=1, ngibbs=5, R=good)
    e.init_state("MTBayesC", 2)                                        # the residual is zeroed: the set-up draw has to be repeated
    with pytest.raises(ValueError, match="liability_init has not"):
        e.liability_sample(iteration=2, seed=1, ngibbs=5, R=good)


def test_build_model_symmetrises_r_and_refuses_unknown_trait_names():
    gdf, ids, g, liab = _simulate(40, 30, 1)
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method="BayesC")
    R = np.array([[1.0, 0.3], [0.3 + 1e-12, 2.0]])
    m = api.build_model("a = intercept + geno\nb = intercept + geno", R, categorical_trait=["a"])
    assert np.array_equal(m.R.val, m.R.val.T) and np.array_equal(m.R.scale, m.R.scale.T)
    with pytest.raises(ValueError, match=r"categorical_trait: \['y'\] not among the traits"):
        api.build_model("a = intercept + geno", categorical_trait=["y"])
    with pytest.raises(ValueError, match="censored_trait"):
        api.build_model("a = intercept + geno\nb = intercept + geno", categorical_trait=["a"], censored_trait=["c"])


def test_julia_liability_params_layout(tmp_path):
    """julia/JWASHip.jl mirrors jwas_liability_params as an isbits struct: its natural-alignment layout against gcc's offsetof /
    sizeof of the header's struct (the check tests/test_abi.py makes for the sweep structs)."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "julia", "JWASHip.jl")).read()
    size = {"Int32": 4, "UInt32": 4, "UInt64": 8, "Int64": 8, "Float32": 4, "Float64": 8}
    body = re.search(r"struct HipLiabilityParams\n(.*?)\nend", src, re.S).group(1)
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
    prog += [f'printf("%zu\\n", offsetof(jwas_liability_params, {f}));' for f, _ in fields]
    prog += ['printf("%zu\\n", sizeof(jwas_liability_params));', "return 0;}"]
    (tmp_path / "l.c").write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "l")]).split()] == expect
    from jwas_jl_amd import _lib
    import ctypes as C
    assert C.sizeof(_lib.LiabilityParams) == expect[-1] and [getattr(_lib.LiabilityParams, f).offset for f, _ in fields] == expect[:-1]


def test_conditional_inverse_wishart_keeps_binary_traits_at_unit_variance():
    from jwas_jl_amd.mcmc import sample_from_conditional_inverse_wishart
    rng = np.random.default_rng(3)
    A = rng.standard_normal((4, 4))
    S = np.linalg.inv(A @ A.T + 4 * np.eye(4))
    for _ in range(20):
        R = sample_from_conditional_inverse_wishart(rng, 50.0, S, [1, 3])
        assert R[1, 1] == 1.0 and R[3, 3] == 1.0 and R[1, 3] == 0.0
        assert np.allclose(R, R.T) and np.all(np.linalg.eigvalsh(R) > 0)
    assert np.array_equal(sample_from_conditional_inverse_wishart(rng, 50.0, S[:2, :2], [0, 1]), np.eye(2))


# cor(EBV, true genetic value) of a binary trait (n = 2000, p = 500, 30 causal markers, prevalence ~ 0.2, BayesC, 300
# iterations) analysed as a threshold trait minus the same 0/1 trait analysed as continuous, seeds 101..105 on the CPU
# stand-in: -0.0024, +0.0025, -0.0051, +0.0056, +0.0104 (mean +0.002, standard deviation 0.006).  The margin is three of
# those standard deviations, rounded up.
STAT_MARGIN = 0.02


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_threshold_model_predicts_no_worse_than_the_linear_model(tmp_path, seed):
    gdf, ids, g, liab = _simulate(2000, 500, seed)
    ph = pd.DataFrame({"ID": ids, "y": (liab > 0.8) + 1.0})
    cor = {}
    for name, build in (("threshold", dict(categorical_trait=["y"])), ("linear", {})):
        _, out = _run(gdf, ph, "y = intercept + geno", tmp_path / name, LiabilityOracleEngine("block"), chain_length=300, burnin=100,
                      seed=seed, **build)
        cor[name] = np.corrcoef(out["EBV_y"]["EBV"], g)[0, 1]
    print(f"seed {seed}: threshold {cor['threshold']:.4f}, linear {cor['linear']:.4f}")
    assert cor["threshold"] > 0.8
    assert cor["threshold"] > cor["linear"] - STAT_MARGIN
