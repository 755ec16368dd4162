"""Location parameters on the device (csrc/locpar.hpp) through the C ABI and runMCMC, against the numpy restatement of
tests/locpar_reference.py on the same Philox counters.

TERM BY TERM the device and the restatement start from one common state (residual and sol are uploaded from the stand-in before
every single-term step).  Both evaluate the same formulas in double; they differ in the ORDER of the level sums (the device's
term layout against np.bincount) and in the libm behind Box-Muller.  Bound per level, u = 2^-53:

    |d sol_l| <= 2 (n_l + t + 4) u A_l / lhs_l + 16 u (|mean_l| + sd_l) + 2^-46 sd_l
    A_l = sum_{i in l} w_i |x_i| sum_m |c_km r_m,i| + |d_l c_kk sol_l| + sum_m |Gi_km u_m,l|

The first term: any two summation orders of the same n_l + t + 2 doubles (and the division); the second: the few roundings of
mean + z sd; the last: Box-Muller -- the angle 2 pi u2 carries one rounding, which the cosine passes on as an absolute error and
the radius (<= 8.5) multiplies, plus a few ulp of the library functions.

THE RESIDUAL of the stepped trait is checked twice.  (a) The apply kernel alone: r' against T(double(r) - x_i delta_l) with
delta_l = sol_l' - sol_l taken from the DEVICE's own sol -- the same IEEE operations on the same doubles: within
4 u (|r| + |x delta|) in a Float64 context, bit-equal in a Float32 one.  (b) Against the stand-in's residual, whose delta differs
by d sol_l: within |x_i| bound_l + 4 u (|r| + |x delta|) in Float64; in Float32 equal to the stand-in's single rounding or one
Float32 ulp of it where the double-level difference crosses a rounding boundary.
Every test prints the figures it measured before it asserts."""
import contextlib
import functools
import io

import numpy as np
import pandas as pd
import pytest

import locpar_reference as LP
from conftest import make_dataset
from locpar_reference import LocparOracleEngine, LocparOracleEngine64

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4


@functools.lru_cache(maxsize=None)
def _genotypes(n, precision):
    return np.asfortranarray(make_dataset(n=n, p=64, ncausal=4, seed=5)["X"].astype(np.float64 if precision == 64 else np.float32))


def _terms(n, t, random, seed=3):
    """Per trait: intercept; covariate; 7 levels (>= 64 records each); 401 levels (2-3 records each); n levels (one record each);
    10 levels with 90 % of the records in the first; 6 declared levels of which the last has no record; 5 levels with one record
    in ten in no level (-1).  random: the 401-level, the n-level and the empty-level factor are random effects 0, 1, 2."""
    rng = np.random.default_rng(seed)
    f7 = rng.permutation(np.arange(n) % 7)
    f401 = rng.permutation(np.arange(n) % 401)
    fn = rng.permutation(n)
    fbig = np.where(rng.random(n) < 0.9, 0, rng.integers(1, 10, n))
    fempty = rng.integers(0, 5, n)
    fneg = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 5, n))
    spec = []
    for k in range(t):
        spec += [(k, "cov", None), (k, "cov", rng.standard_normal(n) + 0.5),
                 (k, "fac", (f7, 7, -1)), (k, "fac", (f401, 401, 0 if random else -1)), (k, "fac", (fn, n, 1 if random else -1)),
                 (k, "fac", (fbig, 10, -1)), (k, "fac", (fempty, 6, 2 if random else -1)), (k, "fac", (fneg, 5, -1))]
    return spec


def _spd(t, rng, scale):
    A = rng.standard_normal((t, t))
    M = (A @ A.T / t + np.eye(t)) * scale
    return (M + M.T) / 2


def _setup(precision, n, t, weighted, random, seed=3):
    import jwas_jl_amd as J
    rng = np.random.default_rng(seed + 17 * t)
    X = _genotypes(n, precision)
    hip = J.HipEngine(0, precision=precision)
    ref = LocparOracleEngine64() if precision == 64 else LocparOracleEngine("block")
    w = rng.uniform(0.25, 4.0, n) if weighted else None
    r0 = rng.standard_normal((t, n)) * 1.3
    for e in (hip, ref):
        e.load_dense(X)
        e.set_weights(None if w is None else w.astype(X.dtype))
        e.setup_blocks(64, "f64")
        e.init_state("BayesC" if t == 1 else "MTBayesC", t)
        for k in range(t):
            e.set_residual(r0[k].astype(X.dtype), k)
        e.locpar_begin(t)
        for k, kind, v in _terms(n, t, random):
            if kind == "cov":
                e.locpar_add_covariate(k, v)
            else:
                e.locpar_add_factor(k, v[0], v[1], v[2])
    kw = dict(vare=1.7) if t == 1 else dict(Rinv=np.linalg.inv(_spd(t, rng, 0.8)))
    if t > 1:
        kw["Rinv"] = (kw["Rinv"] + kw["Rinv"].T) / 2
    kw["Gi"] = [_spd(t, rng, s) for s in (2.0, 0.7, 1.2)] if random else []
    sol0 = rng.standard_normal(ref.locpar_size())
    return hip, ref, kw, sol0


def _level_bound(det, t):
    sd = det["sd"]
    lhs = np.where(det["live"], det["lhs"], 1.0)
    b = 2 * (det["n_l"] + t + 4) * U * det["A"] / lhs + 16 * U * (np.abs(det["mean"]) + sd) + 2.0 ** -46 * sd
    return np.where(det["live"], b, 0.0)


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


PARITY_CASES = [(p, 1003, t, w, rnd) for p in (64, 32) for t in (1, 3) for w in (False, True) for rnd in (False, True)] \
    + [(64, 20011, 1, True, True), (32, 20011, 1, False, True)]


@pytest.mark.parametrize("precision,n,t,weighted,random", PARITY_CASES)
def test_term_by_term_parity(precision, n, t, weighted, random):
    hip, ref, kw, sol0 = _setup(precision, n, t, weighted, random)
    dtype = np.float64 if precision == 64 else np.float32
    try:
        assert hip.locpar_size() == ref.locpar_size() == len(sol0)
        ref.locpar_set_sol(sol0)
        worst_sol = worst_res = 0.0
        flips = total = 0
        nterms = len(ref._lp_terms)
        for j in range(nterms):
            T = ref._lp_terms[j]
            k = T.trait
            for m in range(t):                                   # the common state
                hip.set_residual(ref.get_residual(m), m)
            before_sol, before_r = ref.locpar_get_sol(), ref.get_residual(k).astype(np.float64)
            hip.locpar_set_sol(before_sol)
            det = []
            ref.locpar_step(iteration=2, seed=77, first_term=j, last_term=j + 1, details=det, **kw)
            st = hip.locpar_step(iteration=2, seed=77, first_term=j, last_term=j + 1, **kw)
            got, want = hip.locpar_get_sol(), ref.locpar_get_sol()
            sl = slice(T.off, T.off + T.nlevels)
            other = np.ones(len(got), dtype=bool)
            other[sl] = False
            assert np.array_equal(got[other], before_sol[other])            # only this term moved
            bound = _level_bound(det[0], t)
            err = np.abs(got[sl] - want[sl])
            dead = ~det[0]["live"]
            assert np.array_equal(got[sl][dead], before_sol[sl][dead])       # lhs == 0: left alone
            ratio = float(np.max(err[~dead] / bound[~dead])) if (~dead).any() else 0.0
            worst_sol = max(worst_sol, ratio)
            assert ratio <= 1.0, (j, ratio)
            # the residual
            for m in range(t):
                if m != k:
                    assert np.array_equal(hip.get_residual(m), ref.get_residual(m))
            r_dev, r_ref = hip.get_residual(k).astype(np.float64), ref.get_residual(k).astype(np.float64)
            delta_dev = got[sl] - before_sol[sl]
            own = LP.term_apply(T, before_r.astype(dtype), delta_dev, dtype).astype(np.float64)
            lvl = np.maximum(T.level, 0)
            xd = np.where(T.inl, np.abs(T.x * delta_dev[lvl]), 0.0)
            slack = 4 * U * (np.abs(before_r) + xd)
            if precision == 64:
                assert np.all(np.abs(r_dev - own) <= slack)
                lim = np.where(T.inl, np.abs(T.x) * bound[lvl], 0.0) + slack
                worst_res = max(worst_res, float(np.max(np.abs(r_dev - r_ref) / np.maximum(lim, 1e-300))))
                assert np.all(np.abs(r_dev - r_ref) <= lim)
            else:
                assert np.array_equal(r_dev, own)
                diff = np.abs(r_dev - r_ref)
                assert np.all(diff <= _ulp32(r_ref))
                flips += int((diff != 0).sum())
                total += n
            assert np.array_equal(r_dev[~T.inl], before_r[~T.inl])           # records in no level are not touched
        print(f"locpar-ratio parity p{precision} n{n} t{t} w{int(weighted)} r{int(random)}: sol {worst_sol:.3f}"
              + (f", residual {worst_res:.3f}" if precision == 64 else f", float32 roundings that differ {flips} of {total}"))
        assert flips <= max(1, total // 10000)
    finally:
        hip.close()


@pytest.mark.parametrize("precision,t", [(64, 1), (64, 3), (32, 1), (32, 3)])
def test_whole_steps(precision, t):
    """5 iterations of the full scan from one common start.  Float64: sol within the per-term bound times the number of
    term-steps taken.  Float32: within k 2^-23 A_l / lhs_l after k term-steps (flipped roundings of the residual feed later sums:
    loose by construction, the check for formula errors)."""
    n = 1003
    hip, ref, kw, sol0 = _setup(precision, n, t, True, True)
    try:
        for e in (hip, ref):
            e.locpar_set_sol(sol0)
        nterms = len(ref._lp_terms)
        worst = 0.0
        for it in range(1, 6):
            det = []
            st_r = ref.locpar_step(iteration=it, seed=5, details=det, **kw)
            st_h = hip.locpar_step(iteration=it, seed=5, **kw)
            got, want = hip.locpar_get_sol(), ref.locpar_get_sol()
            ksteps = it * nterms
            for T, d in zip(ref._lp_terms, det):
                sl = slice(T.off, T.off + T.nlevels)
                if precision == 64:
                    bound = ksteps * _level_bound(d, t)
                else:
                    bound = ksteps * 2.0 ** -23 * d["A"] / np.where(d["live"], d["lhs"], 1.0)
                live = d["live"] & (bound > 0)
                err = np.abs(got[sl] - want[sl])
                assert np.array_equal(got[sl][~d["live"]], want[sl][~d["live"]])
                if live.any():
                    worst = max(worst, float(np.max(err[live] / bound[live])))
            for g in range(3):
                assert np.allclose(st_h["utu"][g], st_r["utu"][g], rtol=1e-9 if precision == 64 else 1e-3)
        print(f"locpar-ratio whole-steps p{precision} t{t}: {worst:.3f}")
        assert worst <= 1.0
    finally:
        hip.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_same_seed_same_bits(precision):
    outs = []
    for rep in range(2):
        hip, ref, kw, sol0 = _setup(precision, 1003, 3, True, True)
        try:
            hip.locpar_set_sol(sol0)
            for it in range(1, 6):
                hip.locpar_step(iteration=it, seed=5, **kw)
            outs.append((hip.locpar_get_sol(), [hip.get_residual(k) for k in range(3)]))
        finally:
            hip.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs[0][0], sol0)


def test_cross_products_and_running_means():
    """U'U against the direct product of _get_sol within 2 q u sum |u_k u_m|; _get_means equals the recurrence
    mean += (sol - mean) / k over the per-iteration read-backs (the same IEEE operations) and their plain mean."""
    n, t = 1003, 3
    hip, ref, kw, sol0 = _setup(64, n, t, False, True)
    try:
        hip.locpar_set_sol(sol0)
        sols = []
        mean, mean2 = np.zeros(len(sol0)), np.zeros(len(sol0))
        for it in range(1, 7):
            st = hip.locpar_step(iteration=it, seed=9, **kw)
            sol = hip.locpar_get_sol()
            worst = 0.0
            for g, members in sorted(ref._lp_groups.items()):
                Um = np.stack([sol[ref._lp_terms[j].off:ref._lp_terms[j].off + ref._lp_terms[j].nlevels] for j in members])
                q = Um.shape[1]
                lim = 2 * q * U * (np.abs(Um) @ np.abs(Um).T)
                assert st["utu"][g].shape == (t, t) and np.array_equal(st["utu"][g], st["utu"][g].T)
                worst = max(worst, float(np.max(np.abs(st["utu"][g] - Um @ Um.T) / lim)))
                assert np.all(np.abs(st["utu"][g] - Um @ Um.T) <= lim)
            if it > 2:
                k = it - 2
                hip.locpar_accumulate(k)
                sols.append(sol)
                mean += (sol - mean) / k
                mean2 += (sol * sol - mean2) / k
        m, m2 = hip.locpar_get_means()
        print(f"locpar-ratio cross-products: {worst:.3f}")
        assert np.array_equal(m, mean) and np.array_equal(m2, mean2)
        assert np.allclose(m, np.mean(sols, axis=0), rtol=1e-13, atol=1e-15)
    finally:
        hip.close()


def test_exact_posterior_on_the_device():
    """The CPU test's case and seed (tests/test_locpar_host.py): 4 000 steps, every chain mean within 5 batch-means standard
    errors of the solve of the mixed model equations."""
    import jwas_jl_amd as J
    case = LP.posterior_case()
    hip = J.HipEngine(0, precision=64)
    try:
        z = LP.posterior_z(LP.posterior_engine(hip, case), case)
        print("exact posterior on the device, z per location parameter:", np.round(z, 2))
        assert z.max() <= 5.0
    finally:
        hip.close()


def test_error_contract():
    """A sharded context and calls out of order return the documented codes before any launch."""
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    n = 300
    X = _genotypes(n, 32)
    hip = J.HipEngine(0)
    try:
        def code(fn, *a, **kw):
            with pytest.raises(_lib.JwasHipError) as ei:
                fn(*a, **kw)
            return ei.value.code
        hip.n = n
        assert code(hip.locpar_begin, 1) == ESTATE                           # no residual yet
        hip.load_dense(X)
        hip.setup_blocks(64, "f64")
        assert code(hip.locpar_begin, 1) == ESTATE                           # before init_state
        hip.init_state("BayesC", 1)
        assert code(hip.locpar_add_covariate, 0, None) == ESTATE             # before _begin
        assert code(hip.locpar_size) == ESTATE
        hip._locpar_groups = {}
        assert code(hip.locpar_step, iteration=1, seed=1, vare=1.0) == ESTATE
        assert code(hip.locpar_begin, 2) == EINVAL                           # ntraits differs from init_state's
        hip.locpar_begin(1)
        lev = np.arange(n, dtype=np.int32) % 5
        assert code(hip.locpar_add_covariate, 1, None) == EINVAL             # trait outside the model
        assert code(hip.locpar_add_covariate, 0, np.zeros(n - 1)) == EINVAL
        assert code(hip.locpar_add_covariate, 0, np.full(n, np.nan)) == EINVAL
        assert code(hip.locpar_add_factor, 0, lev, 4) == EINVAL              # a level outside 0..3
        assert code(hip.locpar_add_factor, 0, lev - 2, 5) == EINVAL          # below -1
        assert code(hip.locpar_add_factor, 0, lev, 5, 8) == EINVAL           # random effect outside 0..7
        hip.locpar_add_covariate(0, None)
        hip.locpar_add_factor(0, lev, 5, 0)
        assert code(hip.locpar_add_factor, 0, lev, 5, 0) == EUNSUP           # two terms of one trait in one random effect
        hip._locpar_groups = {0: 1}
        assert hip.locpar_size() == 6
        for bad in (dict(iteration=0, vare=1.0), dict(iteration=1, vare=0.0), dict(iteration=1, vare=np.inf),
                    dict(iteration=1, vare=1.0, first_term=2, last_term=1), dict(iteration=1, vare=1.0, last_term=3)):
            assert code(hip.locpar_step, seed=1, Gi=[np.eye(1)], **bad) == EINVAL
        assert code(hip.locpar_step, iteration=1, seed=1, vare=1.0, Gi=[-np.eye(1)]) == EINVAL
        assert code(hip.locpar_set_sol, np.zeros(5)) == EINVAL
        assert np.array_equal(hip.locpar_get_sol(), np.zeros(6)) and np.array_equal(hip.get_residual(0), np.zeros(n, dtype=np.float32))
        assert code(hip.locpar_add_covariate, 0, None) == ESTATE             # after the first use of sol
        assert code(hip.locpar_accumulate, 0) == EINVAL
        hip.locpar_step(iteration=1, seed=1, vare=1.0, Gi=[np.eye(1)])
        hip.init_state("MTBayesC", 2)
        assert code(hip.locpar_step, iteration=1, seed=1, vare=1.0, Gi=[np.eye(1)]) == ESTATE       # init_state changed the traits
        hip.init_state("BayesC", 1)
        hip.locpar_end()
        assert code(hip.locpar_get_sol) == ESTATE
        hip.locpar_begin(1)
        hip.locpar_add_covariate(0, None)
        hip.load_dense(X)                                                    # loading genotypes frees the state
        hip.setup_blocks(64, "f64")
        hip.init_state("BayesC", 1)
        assert code(hip.locpar_size) == ESTATE
        # a sharded context
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.locpar_begin, 1) == EUNSUP
        hip.comm_destroy()
    finally:
        hip.close()


# ---- runMCMC ------------------------------------------------------------------------------------------------------------------
def _phenotypes(small_data, traits):
    n, p = small_data["raw"].shape
    rng = np.random.default_rng(31)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(small_data["raw"].astype(np.float64), columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    herd = rng.integers(0, 12, n)
    hv = rng.standard_normal(12) * 0.6
    y = small_data["y"].astype(np.float64)
    ph = pd.DataFrame({"ID": ids, "herd": [f"h{h:02d}" for h in herd], "age": rng.uniform(1, 5, n), "weights": rng.uniform(0.5, 2.0, n)})
    for k, tr in enumerate(traits):
        ph[tr] = y + hv[herd] * (1 + 0.3 * k) + 0.4 * k * rng.standard_normal(n)
    return gdf, ph


def _compare(outs, tmp_path, traits, key):
    eo, eh = outs["ref"]["marker effects geno"], outs["hip"]["marker effects geno"]
    d_eff = np.abs(eh["Estimate"].to_numpy(dtype=np.float64) - eo["Estimate"].to_numpy(dtype=np.float64)).max()
    d_ebv = max(np.abs(outs["hip"][f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64) - outs["ref"][f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64)).max()
                for tr in traits)
    lo, lh = outs["ref"]["location parameters"], outs["hip"]["location parameters"]
    assert list(lo["Level"]) == list(lh["Level"]) and len(lo) == len(traits) * 14
    d_lp = np.abs(lh["Estimate"].to_numpy(dtype=np.float64) - lo["Estimate"].to_numpy(dtype=np.float64)).max()
    a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{key}.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
    assert a.shape == b.shape and a.shape[0] == 30
    d_var = float(np.abs(a - b).max())
    print(f"runMCMC {key}: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, location parameters {d_lp:.3e}, variance samples {d_var:.3e}")
    assert d_eff <= 1e-8 and d_ebv <= 1e-7 and d_lp <= 1e-9 and d_var <= 1e-9
    np.testing.assert_allclose(eh["Model_Frequency"].to_numpy(dtype=np.float64), eo["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)


def test_runmcmc_single_trait_weighted_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = _phenotypes(small_data, ["y"])
    outs = {}
    for name, engine in (("ref", LocparOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", Pi=0.9, double_precision=True)
            model = api.build_model("y = intercept + age + herd + geno")
            api.set_covariate(model, "age")
            api.set_random(model, "herd", 0.3)
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True, heterogeneous_residuals=True,
                                     output_folder=str(tmp_path / name), _engine=engine)
    _compare(outs, tmp_path, ["y"], "y:herd_variances")


def test_runmcmc_three_traits_one_threshold_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = _phenotypes(small_data, ["a", "b", "c"])
    ph["c"] = np.digitize(ph["c"], [np.median(ph["c"])]) + 1.0
    outs = {}
    for name, engine in (("ref", LocparOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", double_precision=True)
            model = api.build_model("a = intercept + age + herd + geno\nb = intercept + age + herd + geno\nc = intercept + age + herd + geno",
                                    categorical_trait=["c"])
            api.set_covariate(model, "age")
            api.set_random(model, "herd", np.array([[0.3, 0.1, 0.0], [0.1, 0.4, 0.05], [0.0, 0.05, 0.2]]))
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True,
                                     output_folder=str(tmp_path / name), _engine=engine)
    _compare(outs, tmp_path, ["a", "b", "c"], "a:herd_b:herd_c:herd_variances")


def test_runmcmc_float32_packed_storage_contract(tmp_path, small_data):
    """A Float32 run on 2-bit packed storage: it runs, the files are present, all values finite."""
    from jwas_jl_amd import api, streaming as S
    gdf, ph = _phenotypes(small_data, ["y"])
    ph["ID"] = [str(i) for i in range(len(ph))]
    prefix = S.prepare_streaming_genotypes(small_data["raw"].astype(np.float64), tmp_path / "st", obs_ids=list(ph["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", Pi=0.9, storage="stream")
        model = api.build_model("y = intercept + age + herd + geno")
        api.set_covariate(model, "age")
        api.set_random(model, "herd")
        out = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, output_folder=str(tmp_path / "r"))
    v = np.loadtxt(tmp_path / "r" / "MCMC_samples_y:herd_variances.txt", delimiter=",", skiprows=1)
    assert v.shape == (30,) and np.all(np.isfinite(v)) and np.all(v > 0)
    lp = out["location parameters"]
    assert len(lp) == 14 and np.all(np.isfinite(lp["Estimate"])) and np.all(np.isfinite(lp["SD"]))
    assert np.all(np.isfinite(out["y:herd_variances"]["Estimate"])) and np.all(np.isfinite(out["EBV_y"]["EBV"]))
    assert np.all(np.isfinite(out["marker effects geno"]["Estimate"]))
