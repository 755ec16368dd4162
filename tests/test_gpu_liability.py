"""Threshold and censored traits on the device (csrc/liability.hpp) through the C ABI and runMCMC, against the numpy restatement
of tests/liability_reference.py on the same Philox counters.

Float64 contexts: device and restatement evaluate one formula with two libms.  The bound is measured, not chosen: the
restatement's own worst error against a 50-digit replay (mpmath) of every record of the test's inputs, relative to
max(1, |x|); the device gets four times that.  Float32 contexts: bit-equal after rounding, except where the restatement's
double lies within that bound of a float32 rounding boundary (one float32 ulp allowed there, on fewer than 1 in 10 000
elements).  Every test prints the figures it measured before it asserts."""
import contextlib
import functools
import io

import numpy as np
import pandas as pd
import pytest

import liability_reference as LR
from conftest import make_dataset
from liability_reference import CATEGORICAL, CENSORED, CONTINUOUS, LiabilityOracleEngine, LiabilityOracleEngine64

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
CASES = {                               # name: (trait kinds, ngibbs)
    "binary": ((CATEGORICAL,), 1), "four_categories": ((CATEGORICAL,), 1), "censored": ((CENSORED,), 1),
    "t2_binary_continuous": ((CATEGORICAL, CONTINUOUS), 5), "t3_categorical_continuous_censored": ((CATEGORICAL, CONTINUOUS, CENSORED), 5),
}
THRESHOLDS = {"binary": [-np.inf, 0.0, np.inf], "four_categories": [-np.inf, 0.0, 0.4, 1.1, np.inf],
              "t2_binary_continuous": [-np.inf, 0.0, np.inf], "t3_categorical_continuous_censored": [-np.inf, 0.0, 1.0, np.inf]}


def _inputs(case, n, seed=11):
    """Means mostly within 2 sigma of the bounds, one record in eight up to 10 sigma away, on either side; censored records
    one-sided, two-sided and exact; categorical codes with a few missing (0) in the multi-trait cases."""
    kinds, ngibbs = CASES[case]
    t = len(kinds)
    rng = np.random.default_rng(seed + 1000 * t)
    A = rng.standard_normal((t, t))
    R = np.array([[1.0]]) if t == 1 and kinds[0] == CATEGORICAL else (A @ A.T / t + np.eye(t)) * 0.7
    spec = []
    for k, kind in enumerate(kinds):
        cmean = np.where(rng.random(n) < 0.125, rng.uniform(-10, 10, n), 2.0 * rng.standard_normal(n))
        if kind == CATEGORICAL:
            ncat = len(THRESHOLDS[case]) - 1
            codes = rng.integers(1, ncat + 1, n).astype(np.int32)
            if t > 1:
                codes[rng.random(n) < 0.03] = 0
            spec.append(dict(kind=kind, cmean=cmean, codes=codes, thresholds=np.array(THRESHOLDS[case])))
        elif kind == CENSORED:
            a = cmean + rng.uniform(-3, 3, n)
            w = rng.uniform(0.05, 2.0, n)
            which = rng.integers(0, 4, n)
            lo = np.where(which == 1, -np.inf, a)
            up = np.where(which == 0, np.inf, np.where(which == 3, a, a + w))
            spec.append(dict(kind=kind, cmean=cmean, lower=lo, upper=up))
        else:
            spec.append(dict(kind=kind, resid=rng.standard_normal(n)))
    return kinds, ngibbs, R, spec


def _engines(precision, n, t, p=64):
    import jwas_jl_amd as J
    X = np.asfortranarray(make_dataset(n=n, p=p, ncausal=4, seed=5)["X"].astype(np.float64 if precision == 64 else np.float32))
    hip = J.HipEngine(0, precision=precision)
    ref = LiabilityOracleEngine64() if precision == 64 else LiabilityOracleEngine("block")
    for e in (hip, ref):
        e.load_dense(X)
        e.setup_blocks(64, "f64")
        e.init_state("BayesC" if t == 1 else "MTBayesC", t)
    return hip, ref


def _declare(e, spec):
    e.liability_begin(len(spec))
    for k, s in enumerate(spec):
        if s["kind"] == CATEGORICAL:
            e.set_categorical(k, s["codes"], s["thresholds"])
        elif s["kind"] == CENSORED:
            e.set_censored(k, s["lower"], s["upper"])
    for k, s in enumerate(spec):                 # the residual is y - cmean for the placeholder y the engine holds
        e.set_residual(s["resid"] if s["kind"] == CONTINUOUS else e.liabilities(k) - s["cmean"], k)


def _steps(case, ngibbs, R):
    yield "init", dict(seed=9, R=R)
    yield "sample", dict(iteration=1, seed=9, ngibbs=ngibbs, R=R)
    if case == "four_categories":
        yield "thresholds", np.array([-np.inf, 0.0, 0.55, 0.9, np.inf])
    if ngibbs == 1:                          # (the multi-trait cases draw 5 rounds per call: one call is enough)
        yield "sample", dict(iteration=2, seed=9, ngibbs=ngibbs, R=R)


def _apply(e, what, arg):
    if what == "init":
        e.liability_init(**arg)
    elif what == "sample":
        e.liability_sample(**arg)
    else:
        e.set_thresholds(0, arg)


def _state(e, kinds):
    t = len(kinds)
    return [e.get_residual(k).astype(np.float64) for k in range(t)], [None if kinds[k] == CONTINUOUS else e.liabilities(k) for k in range(t)]


@functools.lru_cache(maxsize=None)
def restatement_error(case, n=64):
    """Worst |restatement - 50-digit replay| / max(1, |replay|) over the liabilities and residuals of every record and step of the
    Float64 parity inputs of `case` (each step replayed from the restatement's own state before it)."""
    kinds, ngibbs, R, spec = _inputs(case, n)
    ref = LiabilityOracleEngine64()
    ref.n, ref.p = n, 1
    ref.ntraits, ref.r = len(kinds), np.zeros((len(kinds), n))
    _declare(ref, spec)
    worst = 0.0
    for what, arg in _steps(case, ngibbs, R):
        if what != "thresholds":
            r0, y0 = [v.copy() for v in ref.r], [None if v is None else v.copy() for v in ref._ly]
            lo, up = list(ref._llo), list(ref._lup)
        _apply(ref, what, arg)
        if what == "thresholds":
            continue
        kw = dict(iteration=arg.get("iteration", 0), seed=arg["seed"], ngibbs=arg.get("ngibbs", 1), R=R, init=what == "init")
        for i in range(n):
            rm, ym = LR.liability_draw_mp(i, r0, y0, kinds, lo, up, **kw)
            for k in range(len(kinds)):
                if kinds[k] != CONTINUOUS:
                    for got, want in ((ref.r[k][i], rm[k]), (ref._ly[k][i], ym[k])):
                        worst = max(worst, float(abs(got - want) / max(1, abs(want))))
    return worst


@pytest.mark.parametrize("case", list(CASES))
def test_draw_parity_float64(case):
    n = 64
    kinds, ngibbs, R, spec = _inputs(case, n)
    bound = 4 * restatement_error(case, n)
    hip, ref = _engines(64, n, len(kinds))
    worst = 0.0
    try:
        for e in (hip, ref):
            _declare(e, spec)
        for what, arg in _steps(case, ngibbs, R):
            for e in (hip, ref):
                _apply(e, what, arg)
            (rh, yh), (rr, yr) = _state(hip, kinds), _state(ref, kinds)
            for k in range(len(kinds)):
                for got, want in ((rh[k], rr[k]),) + (() if yh[k] is None else ((yh[k], yr[k]),)):
                    assert np.all(np.isfinite(got))
                    worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1, np.abs(want)))))
        print(f"{case}: restatement vs mpmath {bound / 4:.3e}, device vs restatement {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound
    finally:
        hip.close()


@pytest.mark.parametrize("case", list(CASES))
def test_draw_parity_float32(case):
    n = 20000 + 37
    kinds, ngibbs, R, spec = _inputs(case, n)
    bound = 4 * restatement_error(case)
    hip, ref = _engines(32, n, len(kinds))
    nelem = nexc = 0
    clean = np.ones(n, dtype=bool)              # records that never used the exception (a record that did has another state afterwards)
    try:
        for e in (hip, ref):
            _declare(e, spec)
        for what, arg in _steps(case, ngibbs, R):
            if what != "thresholds":
                kw = dict(iteration=arg.get("iteration", 0), seed=arg["seed"], ngibbs=arg.get("ngibbs", 1), R=R, init=what == "init")
                r64, y64 = LR.liability_draw(ref.r, ref._ly, ref._lk, ref._llo, ref._lup, dtype=np.float32, unrounded=True, **kw)
            for e in (hip, ref):
                _apply(e, what, arg)
            if what == "thresholds":
                continue
            for k in range(len(kinds)):
                if kinds[k] == CONTINUOUS:
                    assert np.array_equal(hip.get_residual(k), ref.get_residual(k))
                    continue
                for got, want, dbl in ((hip.get_residual(k), ref.get_residual(k), r64[k]), (hip.liabilities(k).astype(np.float32), ref._ly[k], y64[k])):
                    differ = (got != want) & clean
                    nelem += got.size
                    if differ.any():
                        # allowed only where the double sits within `bound` of the midpoint between the two float32 neighbours, and
                        # then by one float32 ulp
                        d, g, w = dbl[differ], got[differ].astype(np.float64), want[differ].astype(np.float64)
                        near = np.abs(d - (g + w) / 2) <= bound * np.maximum(1, np.abs(d))
                        one_ulp = np.abs(g - w) <= np.spacing(np.abs(want[differ])).astype(np.float64) * 1.0000001
                        assert np.all(near & one_ulp), (case, what, k, d[~(near & one_ulp)][:5], g[~(near & one_ulp)][:5], w[~(near & one_ulp)][:5])
                        nexc += int(differ.sum())
                        clean &= ~differ
        print(f"{case}: {nelem} float32 elements, {nexc} at a rounding boundary (bound {bound:.3e})")
        assert nexc * 10000 < nelem
    finally:
        hip.close()


def _central_moments(a, b):
    """Mean, variance and fourth central moment of the standard normal truncated to [a, b] (quadrature on a density scaled by
    its value at the bound nearest zero, so the +8 sigma tail does not underflow)."""
    from scipy.integrate import quad
    x0 = a if a > 0 else (b if b < 0 else 0.0)
    hi = min(b, max(a, 0) + 40.0)
    lo = max(a, min(b, 0) - 40.0)
    w = lambda x: np.exp(-0.5 * (x * x - x0 * x0))       # noqa: E731
    opts = dict(epsabs=0, epsrel=1e-13, limit=400)
    z = quad(w, lo, hi, **opts)[0]
    m = quad(lambda x: x * w(x), lo, hi, **opts)[0] / z
    v = quad(lambda x: (x - m) ** 2 * w(x), lo, hi, **opts)[0] / z
    m4 = quad(lambda x: (x - m) ** 4 * w(x), lo, hi, **opts)[0] / z
    return m, v, m4


@pytest.mark.parametrize("name,a,b", [("centre", -1.0, 1.5), ("one_sided_3_sigma", 3.0, np.inf), ("two_sided_narrow", 0.5, 0.6),
                                      ("tail_8_sigma", 8.0, np.inf), ("beyond_40_sigma", 41.0, np.inf)])
def test_distribution_of_a_million_draws(name, a, b):
    """1 000 000 draws at a fixed mean (200 000 records x 5 iterations, unit residual variance): all finite and inside the
    bounds; mean and variance within 5 standard errors of the truncated normal's."""
    import jwas_jl_amd as J
    n, cmean = 200000, 0.3
    hip = J.HipEngine(0, precision=64)
    try:
        hip.load_dense(np.asfortranarray(make_dataset(n=n, p=4, ncausal=2, seed=1)["X"].astype(np.float64)))
        hip.setup_blocks(4, "f64")
        hip.init_state("BayesC", 1)
        hip.liability_begin(1)
        lo, up = np.full(n, cmean + a), np.full(n, cmean + b)
        hip.set_censored(0, lo, up)
        hip.set_residual(hip.liabilities(0) - cmean, 0)
        hip.liability_init(seed=3, R=[[1.0]])
        draws = []
        for it in range(1, 6):
            hip.liability_sample(iteration=it, seed=3, ngibbs=1, R=[[1.0]])
            y = hip.liabilities(0)
            np.testing.assert_allclose(y - hip.get_residual(0), cmean, rtol=0, atol=1e-13 * max(1, abs(a)))
            assert np.all(np.isfinite(y)) and y.min() >= lo[0] and y.max() <= up[0]
            draws.append(y - cmean)
        z = np.concatenate(draws)
        if name == "beyond_40_sigma":
            print(f"{name}: {z.size} draws in [{z.min():.6f}, {z.max():.6f}]")
            return
        m, v, m4 = _central_moments(a, b)
        se_m, se_v = np.sqrt(v / z.size), np.sqrt((m4 - v * v) / z.size)
        print(f"{name}: mean {z.mean():.8f} (exact {m:.8f}, {abs(z.mean() - m) / se_m:.2f} SE), "
              f"variance {z.var():.8g} (exact {v:.8g}, {abs(z.var() - v) / se_v:.2f} SE)")
        assert abs(z.mean() - m) <= 5 * se_m
        assert abs(z.var() - v) <= 5 * se_v
    finally:
        hip.close()


@pytest.mark.parametrize("precision,n", [(32, 1077), (64, 1077), (32, 65_869), (64, 65_869)], ids=["32", "64", "32-65869", "64-65869"])
def test_minmax_equals_numpy(precision, n):
    """n = 1077: not a multiple of 256.  n = 65 869: 258 workgroups, so k_liability_minmax_reduce's threads 0 and 1 take a second
    trip over the partials; category 4 has members only at records >= 65 536 (its extremes are in the partials 256 and 257 alone)
    and the single-member category 3 lies there too."""
    rng = np.random.default_rng(8)
    if n <= 65_536:
        codes = rng.choice(np.array([0, 1, 2, 4], dtype=np.int32), size=n, p=[0.1, 0.3, 0.3, 0.3])
        single = 513
    else:
        codes = rng.choice(np.array([0, 1, 2], dtype=np.int32), size=n, p=[0.1, 0.45, 0.45])
        codes[65_536:] = rng.choice(np.array([0, 1, 2, 4], dtype=np.int32), size=n - 65_536, p=[0.1, 0.3, 0.3, 0.3])
        single = 65_700
        assert (n + 255) // 256 == 258 and (codes[65_536:] == 4).sum() > 50
    codes[single] = 3                                           # a category with a single member
    th = np.array([-np.inf, 0.0, 0.7, 1.3, np.inf])
    hip, _ = _engines(precision, n, 1)
    try:
        hip.liability_begin(1)
        hip.set_categorical(0, codes, th)
        # before any draw the liabilities are the codes: the stand-alone kernel
        mx, mn = hip.liability_minmax(0)
        want = LR.category_minmax(codes.astype(np.float64), codes, 5)
        assert np.array_equal(mx, want[0]) and np.array_equal(mn, want[1])
        hip.set_residual(hip.liabilities(0) - rng.standard_normal(n), 0)
        hip.liability_init(seed=2, R=[[1.0]])
        for it in (0, 1, 2):                                    # after the set-up draw and after two draws: the fused tail
            if it:
                hip.liability_sample(iteration=it, seed=2, ngibbs=1, R=[[1.0]])
            mx, mn = hip.liability_minmax(0)
            y = hip.liabilities(0)
            want = LR.category_minmax(y, codes, 5)
            assert np.array_equal(mx, want[0]) and np.array_equal(mn, want[1])
            assert mx[3] == y[single] and mn[2] == y[single]
            assert mx[0] == -np.inf and mn[0] == -np.inf and mx[4] == np.inf and mn[4] == np.inf
            assert np.isfinite(mx[1:4]).all() and np.isfinite(mn[1:4]).all() and mn[3] == y[codes == 4].min()
    finally:
        hip.close()


def _phenotypes(kind, n=160, p=120, seed=21):
    d = make_dataset(n=n, p=p, ncausal=6, seed=seed, center=False)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(d["raw"], columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    y = d["y"].astype(np.float64)
    cuts = [np.median(y)] if kind == "binary" else list(np.quantile(y, [0.3, 0.7]))
    return gdf, pd.DataFrame({"ID": ids, "y": np.digitize(y, cuts) + 1.0}), d["raw"], ids


@pytest.mark.parametrize("kind", ["binary", "three_categories"])
def test_runmcmc_double_precision_gpu_vs_standin(tmp_path, kind):
    """runMCMC(double_precision=true) on a threshold trait: the device against the same host loop on the stand-in, same seed, at
    the chain length and tolerances of test_gpu_f64_multitrait.py (1e-8 effects, 1e-7 EBVs); saved thresholds and liabilities
    to 1e-9."""
    from jwas_jl_amd import api
    gdf, ph, _, _ = _phenotypes(kind)
    outs = {}
    for name, engine in (("ref", LiabilityOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", Pi=0.9, double_precision=True)
            model = api.build_model("y = intercept + geno", categorical_trait=["y"])
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True, output_folder=str(tmp_path / name),
                                     _engine=engine)
    eo, eh = outs["ref"]["marker effects geno"], outs["hip"]["marker effects geno"]
    d_eff = np.abs(eh["Estimate"].to_numpy(dtype=np.float64) - eo["Estimate"].to_numpy(dtype=np.float64)).max()
    d_ebv = np.abs(outs["hip"]["EBV_y"]["EBV"].to_numpy(dtype=np.float64) - outs["ref"]["EBV_y"]["EBV"].to_numpy(dtype=np.float64)).max()
    files = {}
    for f in ("threshold", "liabilities"):
        a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{f}_y.txt", delimiter=",") for nm in ("ref", "hip"))
        assert a.shape == b.shape and a.shape[0] == 30
        files[f] = float(np.max(np.abs(np.where(np.isinf(a), 0, a) - np.where(np.isinf(b), 0, b))))
        assert np.array_equal(np.isinf(a), np.isinf(b))
    print(f"{kind}: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, thresholds {files['threshold']:.3e}, liabilities {files['liabilities']:.3e}")
    assert d_eff <= 1e-8 and d_ebv <= 1e-7
    np.testing.assert_allclose(eh["Model_Frequency"].to_numpy(dtype=np.float64), eo["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)
    assert files["threshold"] <= 1e-9 and files["liabilities"] <= 1e-9


def test_runmcmc_double_precision_multitrait_gpu_vs_standin(tmp_path):
    """A binary, a continuous and a 3-category trait (one record in twenty without its category) in Float64: 5 Gibbs rounds,
    the conditional inverse Wishart for R, code 0 for the missing records -- device against the stand-in, same seed, the
    tolerances of the single-trait runs."""
    from jwas_jl_amd import api
    gdf, ph1, _, ids = _phenotypes("binary")
    rng = np.random.default_rng(4)
    d = make_dataset(n=160, p=120, ncausal=6, seed=21, center=False)
    y = d["y"].astype(np.float64)
    c = np.digitize(y + 0.3 * rng.standard_normal(160), list(np.quantile(y, [0.3, 0.7]))) + 1.0
    c[::20] = np.nan
    ph = pd.DataFrame({"ID": ids, "a": ph1["y"], "b": y + 0.5 * rng.standard_normal(160), "c": c})
    outs = {}
    for name, engine in (("ref", LiabilityOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", double_precision=True)
            model = api.build_model("a = intercept + geno\nb = intercept + geno\nc = intercept + geno", categorical_trait=["a", "c"])
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True, output_folder=str(tmp_path / name),
                                     _engine=engine)
        assert model.traits_type == ["categorical(binary)", "continuous", "categorical"]
    eo, eh = outs["ref"]["marker effects geno"], outs["hip"]["marker effects geno"]
    d_eff = np.abs(eh["Estimate"].to_numpy(dtype=np.float64) - eo["Estimate"].to_numpy(dtype=np.float64)).max()
    d_ebv = max(np.abs(outs["hip"][f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64) - outs["ref"][f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64)).max() for k in "abc")
    worst = {}
    for f in ("threshold_c", "liabilities_a", "liabilities_c", "residual_variance"):
        a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{f}.txt", delimiter=",", skiprows=1 if f == "residual_variance" else 0) for nm in ("ref", "hip"))
        assert a.shape == b.shape and a.shape[0] == 30 and np.array_equal(np.isinf(a), np.isinf(b))
        worst[f] = float(np.max(np.abs(np.where(np.isinf(a), 0, a) - np.where(np.isinf(b), 0, b))))
    print(f"multi-trait: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert d_eff <= 1e-8 and d_ebv <= 1e-7
    assert all(v <= 1e-9 for v in worst.values())
    rv = np.loadtxt(tmp_path / "hip" / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1).reshape(-1, 3, 3)
    assert np.all(rv[:, 0, 0] == 1.0) and len(np.unique(rv[:, 1, 1])) > 1


@pytest.mark.parametrize("method,constraint", [("BayesB", False), ("BayesC", True), ("BayesA", True)])
def test_runmcmc_float32_multitrait_other_samplers_contract(tmp_path, method, constraint, _engine=None):
    """A binary and a continuous trait in Float32 under multi-trait BayesB and constraint=true (megaBayesABC), the contract only:
    finite outputs, every saved liability on its side of zero, EBVs of the binary trait that follow the status."""
    from jwas_jl_amd import api
    gdf, ph1, _, ids = _phenotypes("binary", n=300, p=200)
    d = make_dataset(n=300, p=200, ncausal=6, seed=21, center=False)
    ph = pd.DataFrame({"ID": ids, "a": ph1["y"], "b": d["y"].astype(np.float64)})
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(gdf, method=method, constraint=constraint)
        model = api.build_model("a = intercept + geno\nb = intercept + geno", categorical_trait=["a"], constraint=constraint)
        out = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=3, output_folder=str(tmp_path / "run"), _engine=_engine)
    L = np.loadtxt(tmp_path / "run" / "MCMC_samples_liabilities_a.txt", delimiter=",")
    y = ph["a"].to_numpy()
    assert L.shape == (30, 300) and np.all(np.isfinite(L)) and np.all(L[:, y == 1] <= 0) and np.all(L[:, y == 2] >= 0)
    for key in ("marker effects geno", "EBV_a", "EBV_b", "residual variance"):
        assert np.all(np.isfinite(out[key].select_dtypes(include=[np.number]).to_numpy()))
    assert np.corrcoef(out["EBV_a"]["EBV"], y)[0, 1] > 0.2


def test_runmcmc_float32_packed_storage_contract(tmp_path):
    """One Float32 run on 2-bit packed storage, the contract only: finite outputs, every saved liability on its side of the
    thresholds (a Float32 liability against the Float32 rounding of a threshold: rounding is monotone)."""
    from jwas_jl_amd import api
    from jwas_jl_amd import streaming as S
    gdf, ph, raw, ids = _phenotypes("three_categories", n=300, p=400)
    prefix = S.prepare_streaming_genotypes(raw.astype(np.float64), tmp_path / "st", obs_ids=ids, marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", Pi=0.9, storage="stream")
        model = api.build_model("y = intercept + geno", categorical_trait=["y"])
        out = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=3, output_folder=str(tmp_path / "run"), block_size=128)
    th = np.loadtxt(tmp_path / "run" / "MCMC_samples_threshold_y.txt", delimiter=",")
    L = np.loadtxt(tmp_path / "run" / "MCMC_samples_liabilities_y.txt", delimiter=",")
    assert th.shape == (30, 4) and L.shape == (30, 300) and np.all(np.isfinite(L))
    assert np.all(th[:, 1] == 0) and np.all(np.diff(th, axis=1) > 0)
    th32 = th.astype(np.float32).astype(np.float64)
    y = ph["y"].to_numpy()
    for c in (1, 2, 3):
        assert np.all(L[:, y == c] >= th32[:, [c - 1]]) and np.all(L[:, y == c] <= th32[:, [c]])
    for key in ("marker effects geno", "EBV_y", "residual variance"):
        assert np.all(np.isfinite(out[key].select_dtypes(include=[np.number]).to_numpy()))


def test_error_contract():
    """Every entry point decides its errors before any launch: JWAS_HIP_ESTATE before _begin / without a residual,
    JWAS_HIP_EINVAL for codes outside 0..ncat, unsorted thresholds, lower > upper."""
    import jwas_jl_amd as J
    n = 300
    X = np.asfortranarray(make_dataset(n=n, p=64, ncausal=4, seed=5)["X"])
    hip = J.HipEngine(0)

    def code_of(fn, *a, **k):
        with pytest.raises(J.JwasHipError) as ei:
            fn(*a, **k)
        return ei.value.code

    try:
        hip.load_dense(X)
        hip.setup_blocks(64, "f64")
        assert code_of(hip.liability_begin, 1) == ESTATE                        # no residual yet (init_state)
        hip.init_state("BayesC", 1)
        codes, th = np.ones(n, dtype=np.int32), [-np.inf, 0.0, np.inf]
        for fn, args, kw in ((hip.set_categorical, (0, codes, th), {}), (hip.set_censored, (0, np.zeros(n), np.ones(n)), {}),
                             (hip.set_thresholds, (0, th), {}), (hip.liability_init, (), dict(seed=1, R=[[1.0]])),
                             (hip.liability_sample, (), dict(iteration=1, seed=1, ngibbs=1, R=[[1.0]])),
                             (hip.liability_minmax, (0,), {}), (hip.liabilities, (0,), {})):
            assert code_of(fn, *args, **kw) == ESTATE, fn.__name__            # before _begin
        hip.liability_end()                                                     # (ending nothing is fine)
        assert code_of(hip.liability_begin, 2) == EINVAL                        # not the traits of init_state
        hip.liability_begin(1)
        assert code_of(hip.liability_init, seed=1, R=[[1.0]]) == ESTATE         # no trait declared
        assert code_of(hip.set_categorical, 1, codes, th) == EINVAL
        assert code_of(hip.set_categorical, 0, codes[:-1], th) == EINVAL
        bad = codes.copy(); bad[7] = 3
        assert code_of(hip.set_categorical, 0, bad, th) == EINVAL
        bad[7] = -1
        assert code_of(hip.set_categorical, 0, bad, th) == EINVAL
        assert code_of(hip.set_categorical, 0, codes, [-np.inf, 0.5, 0.2, np.inf]) == EINVAL
        assert code_of(hip.set_categorical, 0, codes, [0.0, 1.0, np.inf]) == EINVAL
        assert code_of(hip.set_categorical, 0, codes, [-np.inf, np.inf]) == EINVAL
        lo, up = np.zeros(n), np.ones(n)
        up[5] = -1.0
        assert code_of(hip.set_censored, 0, lo, up) == EINVAL
        up[5] = np.nan
        assert code_of(hip.set_censored, 0, lo, up) == EINVAL
        assert code_of(hip.set_thresholds, 0, th) == ESTATE                     # not categorical (yet)
        assert code_of(hip.liability_minmax, 0) == ESTATE
        assert code_of(hip.liabilities, 0) == ESTATE                            # continuous: no liabilities
        hip.set_categorical(0, codes, [-np.inf, 0.0, 1.0, np.inf])
        assert code_of(hip.set_thresholds, 0, th) == EINVAL                     # another count
        assert code_of(hip.set_thresholds, 0, [-np.inf, 0.0, -1.0, np.inf]) == EINVAL
        assert code_of(hip.liability_sample, iteration=1, seed=1, ngibbs=1, R=[[1.0]]) == ESTATE      # before the set-up draw
        hip.set_residual(hip.liabilities(0), 0)
        assert code_of(hip.liability_init, seed=1, R=[[0.0]]) == EINVAL
        hip.liability_init(seed=1, R=[[1.0]])
        assert code_of(hip.liability_sample, iteration=0, seed=1, ngibbs=1, R=[[1.0]]) == EINVAL
        assert code_of(hip.liability_sample, iteration=1, seed=1, ngibbs=0, R=[[1.0]]) == EINVAL
        assert code_of(hip.liability_sample, iteration=1, seed=1, ngibbs=1, R=[[-1.0]]) == EINVAL
        y0 = hip.liabilities(0)
        assert np.all(y0 <= 0)                                                  # nothing above changed the state
        hip.liability_sample(iteration=1, seed=1, ngibbs=1, R=[[1.0]])
        hip.init_state("BayesC", 1)                                             # a new chain state: the residual was zeroed,
        assert code_of(hip.liability_sample, iteration=2, seed=1, ngibbs=1, R=[[1.0]]) == ESTATE      # so the set-up draw is due again
        skew = [[1.0, 0.3], [0.3000000000000001, 2.0]]
        hip.init_state("MTBayesC", 2)
        hip.liability_begin(2)
        hip.set_categorical(0, codes, th)
        assert code_of(hip.liability_init, seed=1, R=skew) == EINVAL            # R must be exactly symmetric
        hip.load_dense(X)                                                       # loading genotypes frees the liabilities
        hip.setup_blocks(64, "f64")
        hip.init_state("BayesC", 1)
        assert code_of(hip.liabilities, 0) == ESTATE
        hip.liability_begin(1)
        hip.liability_end()
        assert code_of(hip.liabilities, 0) == ESTATE
    finally:
        hip.close()
