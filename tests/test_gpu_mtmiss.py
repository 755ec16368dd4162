"""Multi-trait records that miss some traits on the device (csrc/mtmiss.hpp and the per-record-weight instantiations of
csrc/locpar.hpp) through the C ABI and runMCMC, against the numpy restatement of tests/mtmiss_reference.py on the same Philox
counters and the same host-made tables.

IMPUTATION.  Device and restatement start from one uploaded state and evaluate, per missing cell, the same N = |o| + c + 1
products in double.  Bound per missing cell in a Float64 context, u = 2^-53, derived the way tests/test_gpu_locpar.py derives its
own:

    |d e| <= 2 (N + 2) u A + 4 u |e| + 2^-46 sum_{a <= c} |U[a][c]|
    A = sum_j |B[c][j] e_o[j]| + sum_{a <= c} |z_a U[a][c]|

The first term: any two summation orders of the same N products; the second: the roundings of the final sum; the last:
Box-Muller -- the angle 2 pi u2 carries one rounding, which the cosine passes on as an absolute error the radius (<= 8.5)
multiplies, plus a few ulp of the library functions (the 2^-46 sd_l term of tests/test_gpu_locpar.py with |U| in the place of sd).
In a Float32 context the cell equals the restatement's single rounding, or one Float32 ulp of it where the double-level
difference crosses a rounding boundary.  Observed cells and complete records are bit-equal to the input.

RECORD-WEIGHTED STEP, term by term from a common state: the bound of tests/test_gpu_locpar.py (_level_bound) with c replaced by
the record's row of C[code] and d_l c_kk by D_l (tests/mtmiss_reference.term_draw_w fills the same detail fields); a pedigree
term under the bound of tests/test_gpu_locpar_ped.py (_structured_bound) on the device's own colours.
Every test prints the figures it measured before it asserts."""
import contextlib
import io

import numpy as np
import pytest

import locpar_reference as LP
import locpar_ped_reference as PR
from jwas_jl_amd import mcmc
from mtmiss_reference import MtmissOracleEngine, MtmissOracleEngine64, MtmissPedOracleEngine, MtmissPedOracleEngine64
from test_gpu_locpar import _compare, _genotypes, _level_bound, _phenotypes, _spd, _terms, _ulp32
from test_gpu_locpar_ped import _pedigree, _records, _structured_bound

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4
N = 1003


def _codes(n, t, rng):
    """About 30 % of the records are incomplete.  t >= 3: every pattern occurs except one (code 1), and one pattern (code 2) has
    a single record.  t = 2 has only two incomplete patterns, so both occur: code 1 has a single record, code 2 the others."""
    full = (1 << t) - 1
    if t == 2:
        codes = np.where(rng.random(n) < 0.3, 2, full)
        codes[codes == 1] = 2
        codes[11] = 1
    else:
        codes = np.where(rng.random(n) < 0.3, rng.integers(3, full, n), full)
        codes[11] = 2
        for c in range(3, full):                                 # (each of the others at least twice)
            codes[20 + 2 * c:22 + 2 * c] = c
    counts = np.bincount(codes, minlength=full + 1)
    assert counts[0] == 0 and (counts[1:] == 0).sum() == (0 if t == 2 else 1) and (counts == 1).sum() == 1
    assert 0.2 < 1 - counts[full] / n < 0.4
    return codes.astype(np.int32)


def _engines(precision, t, weighted, rng, ped=False):
    import jwas_jl_amd as J
    X = _genotypes(N, precision)
    hip = J.HipEngine(0, precision=precision)
    if ped:
        ref = MtmissPedOracleEngine64() if precision == 64 else MtmissPedOracleEngine("block")
    else:
        ref = MtmissOracleEngine64() if precision == 64 else MtmissOracleEngine("block")
    w = rng.uniform(0.25, 4.0, N) if weighted else None
    r0 = rng.standard_normal((t, N)) * 1.3
    for e in (hip, ref):
        e.load_dense(X)
        e.set_weights(None if w is None else w.astype(X.dtype))
        e.setup_blocks(64, "f64")
        e.init_state("MTBayesC", t)
        for k in range(t):
            e.set_residual(r0[k].astype(X.dtype), k)
    return hip, ref, r0.astype(X.dtype)


@pytest.mark.parametrize("precision,t", [(p, t) for p in (64, 32) for t in (2, 3, 4)])
def test_imputation_parity(precision, t):
    rng = np.random.default_rng(40 + t)
    hip, ref, r0 = _engines(precision, t, False, rng)
    try:
        codes = _codes(N, t, rng)
        B, Ut, _ = mcmc.missing_pattern_tables(_spd(t, rng, 0.8))
        for e in (hip, ref):
            e.mtmiss_begin(codes)
        det = {}
        ref.mtmiss_impute(iteration=2, seed=77, B=B, U=Ut, details=det)
        hip.mtmiss_impute(iteration=2, seed=77, B=B, U=Ut)
        got = np.stack([hip.get_residual(k) for k in range(t)])
        want = np.stack([ref.get_residual(k) for k in range(t)])
        assert got.dtype == want.dtype == r0.dtype
        observed = np.array([[(c >> k) & 1 for k in range(t)] for c in codes], dtype=bool).T          # t x n
        assert np.array_equal(got[observed], r0[observed]) and np.array_equal(want[observed], r0[observed])
        full = codes == (1 << t) - 1
        assert np.array_equal(got[:, full], r0[:, full])
        miss = ~observed
        assert miss.sum() > 0.25 * N and np.all(got[miss] != r0[miss])        # every missing cell was redrawn
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        if precision == 64:
            bound = 2 * (det["nterms"] + 2) * U * det["A"] + 4 * U * np.abs(want) + 2.0 ** -46 * det["absU"]
            ratio = float(np.max(diff[miss] / bound[miss]))
            print(f"mtmiss-ratio imputation p64 t{t}: {ratio:.3f} of the bound over {int(miss.sum())} cells")
            assert ratio <= 1.0
        else:
            flips = int((diff[miss] != 0).sum())
            print(f"mtmiss imputation p32 t{t}: float32 roundings that differ {flips} of {int(miss.sum())}")
            assert np.all(diff[miss] <= _ulp32(want[miss]))
            assert flips <= max(1, int(miss.sum()) // 10000)
        # the cells follow their conditional: another iteration gives other values on the missing cells only
        hip.mtmiss_impute(iteration=3, seed=77, B=B, U=Ut)
        again = np.stack([hip.get_residual(k) for k in range(t)])
        assert np.array_equal(again[observed], r0[observed]) and np.all(again[miss] != got[miss])
    finally:
        hip.close()


def _setup_terms(precision, t, weighted, random, seed=3):
    rng = np.random.default_rng(seed + 17 * t)
    hip, ref, _ = _engines(precision, t, weighted, rng)
    for e in (hip, ref):
        e.locpar_begin(t)
        for k, kind, v in _terms(N, t, random):
            if kind == "cov":
                e.locpar_add_covariate(k, v)
            else:
                e.locpar_add_factor(k, v[0], v[1], v[2])
    R0 = _spd(t, rng, 0.8)
    kw = {"Gi": [_spd(t, rng, s) for s in (2.0, 0.7, 1.2)] if random else []}
    codes = _codes(N, t, rng)
    for e in (hip, ref):
        e.mtmiss_begin(codes)
    return hip, ref, kw, R0, codes, rng.standard_normal(ref.locpar_size())


def _setup_ped(precision, t, weighted, seed=3):
    """Per trait: intercept; the animal term over the 200-animal pedigree (random effect 0, structured); a 7-level herd term
    (random effect 1, i.i.d.) -- the layout of tests/test_gpu_locpar_ped.py."""
    rng = np.random.default_rng(seed + 17 * t)
    ped, V = _pedigree(200)
    q = len(ped.ids)
    hip, ref, _ = _engines(precision, t, weighted, rng, ped=True)
    lev, herd = _records(q, N, rng), rng.integers(0, 7, N).astype(np.int32)
    for e in (hip, ref):
        e.locpar_begin(t)
        e.locpar_set_group_structure(0, V.indptr, V.indices, V.data)
        for k in range(t):
            e.locpar_add_covariate(k, None)
            e.locpar_add_factor(k, lev, q, 0)
            e.locpar_add_factor(k, herd, 7, 1)
    R0 = _spd(t, rng, 0.8)
    kw = {"Gi": [_spd(t, rng, s) for s in (2.0, 0.7)]}
    color = hip.locpar_group_colors(0)
    ref._lp_struct[0] = PR.prepare_structure(V, color)           # the stand-in visits the DEVICE's colours
    codes = _codes(N, t, rng)
    for e in (hip, ref):
        e.mtmiss_begin(codes)
    return hip, ref, kw, R0, codes, rng.standard_normal(ref.locpar_size())


def _parity(hip, ref, kw, sol0, precision, t, tag):
    """tests/test_gpu_locpar.py's term-by-term parity on two engines whose record weights are switched on."""
    dtype = np.float64 if precision == 64 else np.float32
    assert hip.locpar_size() == ref.locpar_size() == len(sol0)
    ref.locpar_set_sol(sol0)
    worst_sol = worst_res = 0.0
    flips = total = dead_levels = 0
    structs = getattr(ref, "_lp_struct", {})
    for j, T in enumerate(ref._lp_terms):
        k = T.trait
        for m in range(t):                                       # the common state
            hip.set_residual(ref.get_residual(m), m)
        before_sol, before_r = ref.locpar_get_sol(), ref.get_residual(k).astype(np.float64)
        hip.locpar_set_sol(before_sol)
        det = []
        ref.locpar_step(iteration=2, seed=77, first_term=j, last_term=j + 1, details=det, **kw)
        hip.locpar_step(iteration=2, seed=77, first_term=j, last_term=j + 1, **kw)
        got, want = hip.locpar_get_sol(), ref.locpar_get_sol()
        sl = slice(T.off, T.off + T.nlevels)
        other = np.ones(len(got), dtype=bool)
        other[sl] = False
        assert np.array_equal(got[other], before_sol[other])      # only this term moved
        bound = _structured_bound(det[0], t, structs[T.group]) if T.group in structs else _level_bound(det[0], t)
        err = np.abs(got[sl] - want[sl])
        dead = ~det[0]["live"]
        dead_levels += int(dead.sum())
        assert np.array_equal(got[sl][dead], before_sol[sl][dead])          # lhs == 0: left alone
        ratio = float(np.max(err[~dead] / bound[~dead])) if (~dead).any() else 0.0
        worst_sol = max(worst_sol, ratio)
        assert ratio <= 1.0, (j, ratio)
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
            total += N
        assert np.array_equal(r_dev[~T.inl], before_r[~T.inl])
    print(f"mtmiss-ratio {tag}: sol {worst_sol:.3f}"
          + (f", residual {worst_res:.3f}" if precision == 64 else f", float32 roundings that differ {flips} of {total}") + f", levels left alone {dead_levels}")
    assert flips <= max(1, total // 10000)
    return dead_levels


@pytest.mark.parametrize("precision,t,weighted,random", [(p, t, w, r) for p in (64, 32) for t in (2, 3) for w in (False, True) for r in (False, True)])
def test_record_weighted_term_by_term_parity(precision, t, weighted, random):
    hip, ref, kw, R0, codes, sol0 = _setup_terms(precision, t, weighted, random)
    try:
        _, _, Ctab = mcmc.missing_pattern_tables(R0)
        for e in (hip, ref):
            e.mtmiss_set_record_weights(Ctab)
        dead = _parity(hip, ref, kw, sol0, precision, t, f"parity p{precision} t{t} w{int(weighted)} r{int(random)}")
        if not random:          # the n-level factor has one record per level: fixed, a level whose record lacks the trait is left alone
            assert dead > t     # (more than the declared-but-empty level of every trait)
    finally:
        hip.close()


@pytest.mark.parametrize("precision,t", [(64, 2), (64, 3), (32, 2), (32, 3)])
def test_record_weighted_pedigree_parity(precision, t):
    hip, ref, kw, R0, codes, sol0 = _setup_ped(precision, t, True)
    try:
        _, _, Ctab = mcmc.missing_pattern_tables(R0)
        for e in (hip, ref):
            e.mtmiss_set_record_weights(Ctab)
        _parity(hip, ref, kw, sol0, precision, t, f"ped parity p{precision} t{t}")
    finally:
        hip.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_weights_switch_and_same_seed_same_bits(precision):
    """set_record_weights(None) after a weighted step: the next step is the plain step bit for bit (compared with an engine whose
    weights were never switched on).  Imputation and three weighted steps twice with one seed: identical bits."""
    t = 3
    outs = []
    for rep in range(3):
        hip, ref, kw, R0, codes, sol0 = _setup_terms(precision, t, True, True)
        try:
            B, Ut, Ctab = mcmc.missing_pattern_tables(R0)
            Rinv = np.linalg.inv(R0)
            Rinv = (Rinv + Rinv.T) / 2
            r0 = [hip.get_residual(k) for k in range(t)]
            if rep < 2:
                hip.locpar_set_sol(sol0)
                hip.mtmiss_set_record_weights(Ctab)
                for it in range(1, 4):
                    hip.mtmiss_impute(iteration=it, seed=5, B=B, U=Ut)
                    hip.locpar_step(iteration=it, seed=5, **kw)
                outs.append((hip.locpar_get_sol(), [hip.get_residual(k) for k in range(t)]))
                hip.mtmiss_set_record_weights(None)
            # the plain step from the common start
            hip.locpar_set_sol(sol0)
            for k in range(t):
                hip.set_residual(r0[k], k)
            hip.locpar_step(iteration=4, seed=5, Rinv=Rinv, **kw)
            outs.append((hip.locpar_get_sol(), [hip.get_residual(k) for k in range(t)]))
        finally:
            hip.close()
    weighted_a, plain_a, weighted_b, plain_b, never = outs
    for x, y in ((weighted_a, weighted_b), (plain_a, plain_b), (plain_a, never)):
        assert np.array_equal(x[0], y[0])
        for a, b in zip(x[1], y[1]):
            assert np.array_equal(a, b)
    assert not np.array_equal(weighted_a[0], plain_a[0]) and not np.array_equal(weighted_a[0], sol0)


def test_error_contract():
    """Calls out of order, bad codes and tables, one trait and a sharded context return the documented codes before any launch."""
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
        hip.ntraits = 2
        full = np.full(n, 3, dtype=np.int32)
        B, Ut, Ctab = mcmc.missing_pattern_tables(np.array([[1.0, 0.3], [0.3, 2.0]]))
        assert code(hip.mtmiss_begin, full) == ESTATE                         # no residual yet
        hip.load_dense(X)
        hip.setup_blocks(64, "f64")
        assert code(hip.mtmiss_begin, full) == ESTATE                         # before init_state
        hip.init_state("MTBayesC", 2)
        assert code(hip.mtmiss_impute, iteration=1, seed=1, B=B, U=Ut) == ESTATE          # before _begin
        assert code(hip.mtmiss_set_record_weights, Ctab) == ESTATE
        assert code(hip.mtmiss_set_record_weights, None) == ESTATE
        bad = full.copy()
        bad[7] = 0
        assert code(hip.mtmiss_begin, bad) == EINVAL                          # a code of 0
        bad[7] = 4
        assert code(hip.mtmiss_begin, bad) == EINVAL                          # >= 2^t
        assert code(hip.mtmiss_begin, full[:-1]) == EINVAL                    # a wrong n
        codes = full.copy()
        codes[::3] = 1
        hip.mtmiss_begin(codes)
        nan = B.copy()
        nan[1, 0, 0] = np.nan
        inf = Ctab.copy()
        inf[2, 1, 1] = np.inf
        assert code(hip.mtmiss_impute, iteration=1, seed=1, B=nan, U=Ut) == EINVAL
        assert code(hip.mtmiss_impute, iteration=1, seed=1, B=B, U=nan) == EINVAL
        assert code(hip.mtmiss_impute, iteration=0, seed=1, B=B, U=Ut) == EINVAL
        assert code(hip.mtmiss_set_record_weights, inf) == EINVAL
        assert np.array_equal(hip.get_residual(1), np.zeros(n, dtype=np.float32))            # nothing was launched
        hip.init_state("BayesC", 1)                                           # the number of traits changed
        hip.ntraits = 2
        assert code(hip.mtmiss_impute, iteration=1, seed=1, B=B, U=Ut) == ESTATE
        assert code(hip.mtmiss_set_record_weights, Ctab) == ESTATE
        hip.ntraits = 1
        hip.mtmiss_begin(np.ones(n, dtype=np.int32))
        assert code(hip.mtmiss_set_record_weights, np.ones((2, 1, 1))) == ESTATE             # record weights with one trait
        hip.mtmiss_set_record_weights(None)
        hip.mtmiss_end()
        assert code(hip.mtmiss_set_record_weights, None) == ESTATE
        hip.init_state("MTBayesC", 2)
        hip.mtmiss_begin(codes)
        hip.load_dense(X)                                                     # loading genotypes frees the state
        hip.setup_blocks(64, "f64")
        hip.init_state("MTBayesC", 2)
        assert code(hip.mtmiss_impute, iteration=1, seed=1, B=B, U=Ut) == ESTATE
        assert J.HipEngine.mtmiss_estimate_bytes(50000) == MtmissOracleEngine.mtmiss_estimate_bytes(50000) < 1e6
        # a sharded context
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mtmiss_begin, codes) == EUNSUP
        hip.comm_destroy()
        hip.mtmiss_begin(codes)
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.mtmiss_impute, iteration=1, seed=1, B=B, U=Ut) == EUNSUP
        assert code(hip.mtmiss_set_record_weights, Ctab) == EUNSUP
        hip.comm_destroy()
    finally:
        hip.close()


# ---- runMCMC ------------------------------------------------------------------------------------------------------------------
def _with_missing(ph, traits, seed=8):
    """About 20 % of the records lack one of `traits`."""
    rng = np.random.default_rng(seed)
    ph = ph.copy()
    pick = rng.random(len(ph)) < 0.2
    which = rng.integers(0, len(traits), len(ph))
    for j, tr in enumerate(traits):
        ph.loc[pick & (which == j), tr] = np.nan
    assert 0.1 < pick.mean() < 0.3
    return ph


def test_runmcmc_two_traits_random_effect_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = _phenotypes(small_data, ["a", "b"])
    ph = _with_missing(ph, ["a", "b"])
    outs = {}
    for name, engine in (("ref", MtmissOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", double_precision=True)
            model = api.build_model("a = intercept + age + herd + geno\nb = intercept + age + herd + geno")
            api.set_covariate(model, "age")
            api.set_random(model, "herd", np.array([[0.3, 0.1], [0.1, 0.4]]))
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True,
                                     output_folder=str(tmp_path / name), _engine=engine)
    _compare(outs, tmp_path, ["a", "b"], "a:herd_b:herd_variances")


def test_runmcmc_three_traits_one_categorical_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = _phenotypes(small_data, ["a", "b", "c"])
    ph["c"] = np.digitize(ph["c"], [np.median(ph["c"])]) + 1.0
    ph = _with_missing(ph, ["a", "b", "c"])
    outs = {}
    for name, engine in (("ref", MtmissOracleEngine64()), ("hip", None)):
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
    """A Float32 run on 2-bit packed storage with missing traits: it runs, the files are present, all values finite."""
    from jwas_jl_amd import api, streaming as S
    gdf, ph = _phenotypes(small_data, ["a", "b"])
    ph = _with_missing(ph, ["a", "b"])
    ph["ID"] = [str(i) for i in range(len(ph))]
    prefix = S.prepare_streaming_genotypes(small_data["raw"].astype(np.float64), tmp_path / "st", obs_ids=list(ph["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", storage="stream")
        model = api.build_model("a = intercept + age + herd + geno\nb = intercept + age + herd + geno")
        api.set_covariate(model, "age")
        api.set_random(model, "herd")
        out = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, output_folder=str(tmp_path / "r"))
    v = np.loadtxt(tmp_path / "r" / "MCMC_samples_a:herd_b:herd_variances.txt", delimiter=",", skiprows=1)
    assert v.shape == (30, 4) and np.all(np.isfinite(v))
    lp = out["location parameters"]
    assert len(lp) == 28 and np.all(np.isfinite(lp["Estimate"])) and np.all(np.isfinite(lp["SD"]))
    for key, col in (("a:herd_b:herd_variances", "Estimate"), ("EBV_a", "EBV"), ("EBV_b", "EBV"), ("marker effects geno", "Estimate"),
                     ("residual variance", "Estimate")):
        assert np.all(np.isfinite(out[key][col].to_numpy(dtype=np.float64))), key
