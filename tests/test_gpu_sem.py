"""Structural equation models on the device (csrc/sem.hpp) through the C ABI and runMCMC, against the numpy restatement of
tests/sem_reference.py on the same Philox counters.

The device and the restatement start every compared step from one common uploaded state (residual and lambda).  Both evaluate the
same formulas in double; they differ in the ORDER of the O(n) sums (the device's grid against numpy's dot product) and in the libm
behind Box-Muller.  With u = 2^-53 and |.| taken entry by entry:

    S_jk, C_ji     any two summation orders of the same n rounded products:  2 (n + 2) u sum |y_j y_k|,  2 (n + 2) u sum |y_j r_i|
    rhs, F         d rhs = (dC + dS |lambda_old| + (k + 2) u (|C| + |S| |lambda_old|)) / R_ii,   dF = dS / R_ii + u |F|
    mu             twice the first-order bound of a perturbed solve:  2 |inv(F)| (d rhs + dF |mu|)
    lambda         the same, plus 2^-46 sum_m |inv(L')|_qm for Box-Muller (the angle 2 pi u2 carries one rounding, which the cosine
                   passes on as an absolute error and the radius <= 8.5 multiplies, plus a few ulp of the library functions -- the
                   argument of tests/test_gpu_locpar.py)

THE RESIDUAL is checked against T(((double(r) + d_1 y_j1) + d_2 y_j2) + ...) with d = lambda_old - lambda_new from the DEVICE's own
coefficients: the same IEEE operations on the same doubles -- bit-equal in a Float32 context, within 4 u of the sum of the absolute
terms in a Float64 one.  Every test prints the figures it measured before it asserts."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

import sem_reference as SR
from conftest import make_dataset
from sem_reference import SemLocparOracleEngine64, SemOracleEngine, SemOracleEngine64

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4


def _structure(t, name):
    cs = np.zeros((t, t), dtype=np.int32)
    if name == "full":
        cs[np.tril_indices(t, -1)] = 1
    elif name == "edge":                 # a single edge: the last trait on the first
        cs[t - 1, 0] = 1
    elif name == "noparents":            # trait 1 has no parents, the last trait has all
        cs[t - 1, :t - 1] = 1
    elif name == "t4":                   # {(3,2), (4,1)} 1-based: row order and column order of the cells differ
        cs[2, 1] = 1
        cs[3, 0] = 1
    return cs


CASES = [(prec, 1003, t, s) for prec in (64, 32) for t, s in ((2, "full"), (3, "full"), (3, "edge"), (3, "noparents"), (4, "full"), (4, "t4"))] \
    + [(64, 20011, 3, "full"), (32, 20011, 3, "full"), (64, 20011, 4, "t4")] \
    + [(64, 525_389, 4, "full"), (32, 525_389, 3, "full")]     # n > 512 x 1024: k_sem_dots' capped grid takes a second trip


@functools.lru_cache(maxsize=None)
def _genotypes(n, precision):
    dtype = np.float64 if precision == 64 else np.float32
    if n > 100_000:                      # (the design plays no part in a structural-equation step: a small matrix, tiled)
        return np.asfortranarray(np.tile(_genotypes(1003, precision), (-(-n // 1003), 1))[:n].astype(dtype))
    return np.asfortranarray(make_dataset(n=n, p=64, ncausal=4, seed=5)["X"].astype(dtype))


@functools.lru_cache(maxsize=None)
def _data(n, t):
    """(y, r0, lambda0 pattern): correlated phenotypes with non-zero means, a residual that is not y."""
    rng = np.random.default_rng(1000 * t + n % 997)
    base = rng.standard_normal(n)
    y = np.stack([1.0 + 0.3 * k + 0.6 * base + rng.standard_normal(n) for k in range(t)])
    r0 = rng.standard_normal((t, n)) * 1.3 + 0.2
    lam0 = rng.uniform(-0.8, 0.8, (t, t))
    return y, r0, lam0


def _setup(precision, n, t, cs):
    import jwas_jl_amd as J
    X = _genotypes(n, precision)
    y, r0, lam0 = _data(n, t)
    hip = J.HipEngine(0, precision=precision)
    ref = SemOracleEngine64() if precision == 64 else SemOracleEngine("block")
    for e in (hip, ref):
        e.load_dense(X)
        e.setup_blocks(64, "f64")
        e.init_state("MTBayesC", t)
        for k in range(t):
            e.set_residual(r0[k].astype(X.dtype), k)
        e.sem_begin(y, cs)
    return hip, ref, y, r0.astype(X.dtype), lam0 * cs


def _abs_gram(y):
    return np.abs(y) @ np.abs(y).T


# ---- 1. the Gram matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t", [(1003, 2), (1003, 3), (1003, 4), (20011, 3), (20011, 4), (525_389, 4)])      # (the last: k_sem_gram's second trip)
def test_gram(n, t):
    hip, ref, y, r0, lam0 = _setup(64, n, t, _structure(t, "full"))
    try:
        S = hip.sem_get_gram()
        bound = 2 * (n + 2) * U * _abs_gram(y)
        err = np.abs(S - y @ y.T)
        print(f"sem gram n={n} t={t}: worst error / bound {(err / bound).max():.3f}")
        assert S.shape == (t, t) and np.array_equal(S, S.T) and np.all(err <= bound)
    finally:
        hip.close()


# ---- 2. and 3. one step from a common state: C, mu, lambda and the residual -------------------------------------------------------
@pytest.mark.parametrize("precision,n,t,structure", CASES)
def test_step_parity_and_apply(precision, n, t, structure):
    cs = _structure(t, structure)
    hip, ref, y, r0, lam0 = _setup(precision, n, t, cs)
    try:
        R_diag = np.array([1.3, 0.7, 2.1, 0.9])[:t]
        absS = _abs_gram(y)
        worst = {"C": 0.0, "mu": 0.0, "lambda": 0.0, "apply": 0.0}
        for it in (1, 2):                        # iteration 2 starts from the device's own lambda, uploaded to the stand-in
            if it == 1:
                for e in (hip, ref):
                    e.sem_set_lambda(lam0)
                before = r0.copy()
            else:
                before = np.stack([hip.get_residual(k) for k in range(t)])
                for k in range(t):
                    ref.set_residual(before[k], k)
                ref.sem_set_lambda(hip.sem_get_lambda())
            old = hip.sem_get_lambda()
            assert np.array_equal(old, ref.sem_get_lambda())
            details = []
            got = hip.sem_step(iteration=it, seed=29, R_diag=R_diag)
            want = ref.sem_step(iteration=it, seed=29, R_diag=R_diag, details=details)
            det = details[0]["traits"]
            assert sorted(det) == [i for i in range(t) if cs[i].any()]
            for i, d in det.items():
                P, k, Rii = d["P"], d["P"].size, d["R"]
                dC = 2 * (n + 2) * U * d["absC"]
                dS = 2 * (n + 2) * U * absS[np.ix_(P, P)]
                eC = np.abs(got["ypr"][i, P] - d["C"])
                worst["C"] = max(worst["C"], (eC / dC).max())
                assert np.all(eC <= dC), ("C", i, eC, dC)
                drhs = (dC + dS @ np.abs(d["old"]) + (k + 2) * U * (np.abs(d["C"]) + np.abs(d["S"]) @ np.abs(d["old"]))) / Rii
                dF = dS / Rii + U * np.abs(d["F"])
                Finv = np.abs(np.linalg.inv(d["F"]))
                bmu = 2 * Finv @ (drhs + dF @ np.abs(d["mu"]))
                emu = np.abs(got["mean"][i, P] - d["mu"])
                worst["mu"] = max(worst["mu"], (emu / bmu).max())
                assert np.all(emu <= bmu), ("mu", i, emu, bmu)
                blam = bmu + 2.0 ** -46 * np.abs(np.linalg.inv(d["L"].T)).sum(axis=1)
                elam = np.abs(got["lambda"][i, P] - want["lambda"][i, P])
                worst["lambda"] = max(worst["lambda"], (elam / blam).max())
                assert np.all(elam <= blam), ("lambda", i, elam, blam)
            # outside the structure nothing is written
            assert np.all(got["lambda"][cs == 0] == 0.0) and np.all(got["mean"][cs == 0] == 0.0) and np.all(got["ypr"][cs == 0] == 0.0)
            # the apply kernel, from the device's own d
            dmat = old - got["lambda"]
            expect = SR.sem_apply(before, y, cs, dmat)
            after = np.stack([hip.get_residual(k) for k in range(t)])
            for i in range(t):
                if not cs[i].any() or precision == 32:
                    assert np.array_equal(after[i], expect[i]), ("apply", i)
                else:
                    A = np.abs(before[i]) + np.abs(dmat[i]) @ np.abs(y)
                    ea = np.abs(after[i] - expect[i])
                    worst["apply"] = max(worst["apply"], (ea / (4 * U * A)).max())
                    assert np.all(ea <= 4 * U * A), ("apply", i)
        print(f"sem step {precision}-bit n={n} t={t} {structure}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    finally:
        hip.close()


# ---- 4. the indirect and overall accumulators -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,t", [(64, 3), (32, 3), (64, 4), (32, 2)])
def test_accumulate(precision, t):
    n = 1003
    hip, ref, y, r0, lam0 = _setup(precision, n, t, _structure(t, "full"))
    try:
        rng = np.random.default_rng(77 + t)
        p = hip.p
        mean = {kind: np.zeros((t, p)) for kind in ("indirect", "overall")}
        mean2 = {kind: np.zeros((t, p)) for kind in ("indirect", "overall")}
        freq = {kind: np.zeros((t, p)) for kind in ("indirect", "overall")}
        A1 = {kind: np.zeros((t, p)) for kind in ("indirect", "overall")}
        A2 = {kind: np.zeros((t, p)) for kind in ("indirect", "overall")}
        for s in (1, 2, 3):
            alpha = (rng.standard_normal((t, p)) * (rng.random((t, p)) < 0.3)).astype(hip.dtype)
            alpha[:, 5] = 0.0                                            # a marker that is never in the model
            for k in range(t):
                hip.set_state(k, alpha=alpha[k])
            K = np.tril(rng.uniform(-1.5, 1.5, (t, t)), -1)
            hip.sem_accumulate(K, s)
            a64 = alpha.astype(np.float64)
            ind, ov = SR.indirect_overall(K, a64)
            absind = np.abs(K) @ np.abs(a64)
            for kind, v, av in (("indirect", ind, absind), ("overall", ov, np.abs(a64) + absind)):
                mean[kind] += (v - mean[kind]) / s
                mean2[kind] += (v * v - mean2[kind]) / s
                freq[kind] += ((v != 0.0) - freq[kind]) / s
                A1[kind] += av
                A2[kind] += av * av
        for kind in ("indirect", "overall"):
            for k in range(t):
                m, m2, f = hip.sem_get_effects(kind, k)
                e1, e2 = np.abs(m - mean[kind][k]), np.abs(m2 - mean2[kind][k])
                b1, b2 = 4 * U * A1[kind][k], 4 * U * A2[kind][k]
                print(f"sem accumulate {precision}-bit t={t} {kind} trait {k}: max error {e1.max():.3e} / {e2.max():.3e}")
                assert np.all(e1 <= b1) and np.all(e2 <= b2) and np.array_equal(f, freq[kind][k])
            assert np.all(hip.sem_get_effects(kind, t - 1)[2][5] == 0.0)
        assert np.all(hip.sem_get_effects("indirect", 0)[0] == 0.0) and np.any(hip.sem_get_effects("indirect", t - 1)[0] != 0.0)
    finally:
        hip.close()


# ---- 5. same seed, same bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_same_seed_same_bits(precision):
    n, t = 20011, 3
    runs = []
    for _ in range(2):
        hip, ref, y, r0, lam0 = _setup(precision, n, t, _structure(t, "full"))
        try:
            lams = [hip.sem_step(iteration=it, seed=5, R_diag=[1.0, 0.8, 1.2]) for it in range(1, 6)]
            runs.append((np.stack([s["lambda"] for s in lams]), np.stack([s["ypr"] for s in lams]), np.stack([hip.get_residual(k) for k in range(t)]),
                         hip.sem_get_gram()))
        finally:
            hip.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert not np.array_equal(runs[0][0][0], runs[0][0][1])


# ---- 6. the exact conditional ---------------------------------------------------------------------------------------------------------
def test_exact_conditional_on_the_device():
    """The CPU test's case and seed (tests/test_sem_host.py): 4 000 steps, every mean within 5 sqrt(V_kk / N) of mu, every sample
    variance within 5 V_kk sqrt(2 / (N - 1)) of V_kk."""
    import jwas_jl_amd as J
    case = SR.conditional_case()
    hip = J.HipEngine(0, precision=64)
    try:
        rows = SR.conditional_check(SR.conditional_engine(hip, case), case)
        for i, j, zm, zv in rows:
            print(f"exact conditional on the device lambda[{i},{j}]: mean {zm:.2f} se, variance {zv:.2f} se")
        assert len(rows) == 3 and max(max(zm, zv) for _, _, zm, zv in rows) <= 5.0
    finally:
        hip.close()


# ---- 7. the error contract ------------------------------------------------------------------------------------------------------------
def test_error_contract():
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    n, t = 300, 3
    X = _genotypes(n, 32)
    y = np.random.default_rng(3).standard_normal((t, n))
    cs = _structure(t, "full")
    hip = J.HipEngine(0)
    try:
        def code(fn, *a, **kw):
            with pytest.raises(_lib.JwasHipError) as ei:
                fn(*a, **kw)
            return ei.value.code

        def without_session():
            hip._sem_t = t
            return [code(hip.sem_step, iteration=1, seed=1, R_diag=np.ones(t)), code(hip.sem_get_lambda), code(hip.sem_set_lambda, np.zeros((t, t))),
                    code(hip.sem_get_gram), code(hip.sem_accumulate, np.zeros((t, t)), 1), code(hip.sem_get_effects, "indirect", 0), code(hip.sem_end)]
        hip.n, hip.p = n, 64
        assert code(hip.sem_begin, y, cs) == ESTATE                           # no residual yet
        hip.load_dense(X)
        hip.setup_blocks(64, "f64")
        assert code(hip.sem_begin, y, cs) == ESTATE                           # before init_state
        hip.init_state("MTBayesC", t)
        assert without_session() == [ESTATE] * 7
        assert code(hip.sem_begin, y[:1], np.zeros((1, 1))) == EINVAL         # one trait
        assert code(hip.sem_begin, y[:2], _structure(2, "full")) == EINVAL    # ntraits differs from init_state's
        assert code(hip.sem_begin, y[:, :n - 1], cs) == EINVAL                # a wrong n
        for bad in (cs * 2, cs.T, cs + np.eye(t, dtype=np.int32), -cs):
            assert code(hip.sem_begin, y, bad) == EINVAL                      # not 0 / 1, not strictly lower
        ynan = y.copy(); ynan[1, 7] = np.nan
        yinf = y.copy(); yinf[2, n - 1] = np.inf
        assert code(hip.sem_begin, ynan, cs) == EINVAL and code(hip.sem_begin, yinf, cs) == EINVAL
        assert without_session() == [ESTATE] * 7                             # none of the failed calls opened a session
        hip.sem_begin(y, _structure(t, "edge"))
        for bad in (dict(iteration=0, R_diag=np.ones(t)), dict(iteration=1, R_diag=[1.0, 0.0, 1.0]), dict(iteration=1, R_diag=[1.0, 1.0, -2.0]),
                    dict(iteration=1, R_diag=[np.inf, 1.0, 1.0]), dict(iteration=1, R_diag=[1.0, np.nan, 1.0])):
            assert code(hip.sem_step, seed=1, **bad) == EINVAL
        Knan = np.zeros((t, t)); Knan[2, 0] = np.nan
        assert code(hip.sem_accumulate, Knan, 1) == EINVAL and code(hip.sem_accumulate, np.zeros((t, t)), 0.5) == EINVAL
        out_of_structure = np.zeros((t, t)); out_of_structure[1, 0] = 0.3
        assert code(hip.sem_set_lambda, out_of_structure) == EINVAL and code(hip.sem_set_lambda, Knan) == EINVAL
        buf = np.empty(64)
        raw = lambda kind, trait: hip._chk(hip._L.jwas_hip_sem_get_effects(hip._h, kind, trait, buf.ctypes.data, None, None))   # noqa: E731
        assert code(raw, 2, 0) == EINVAL and code(raw, 0, t) == EINVAL and code(raw, 0, -1) == EINVAL
        assert np.array_equal(hip.sem_get_lambda(), np.zeros((t, t)))        # nothing was launched
        assert np.array_equal(hip.get_residual(2), np.zeros(n, dtype=np.float32))
        hip.sem_begin(y, cs)                                                  # _begin on an open session replaces it
        hip.sem_step(iteration=1, seed=1, R_diag=np.ones(t))
        hip.init_state("MTBayesC", 2)
        assert code(hip.sem_step, iteration=2, seed=1, R_diag=np.ones(t)) == ESTATE       # init_state changed the traits
        assert code(hip.sem_get_lambda) == ESTATE
        hip.init_state("MTBayesC", t)
        hip.sem_step(iteration=2, seed=1, R_diag=np.ones(t))
        # a sharded context
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.sem_step, iteration=3, seed=1, R_diag=np.ones(t)) == EUNSUP
        hip.sem_end()
        assert code(hip.sem_begin, y, cs) == EUNSUP
        hip.comm_destroy()
        assert without_session() == [ESTATE] * 7
        hip.sem_begin(y, cs)
        hip.load_dense(X)                                                     # loading genotypes frees the session
        hip.setup_blocks(64, "f64")
        hip.init_state("MTBayesC", t)
        assert without_session() == [ESTATE] * 7
    finally:
        hip.close()


# ---- 8. and 9. runMCMC ----------------------------------------------------------------------------------------------------------------
EQ3 = "a = intercept + age + geno\nb = intercept + age + geno\nc = intercept + age + geno"
CS3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])


def test_runmcmc_three_traits_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = SR.sem_phenotypes(small_data, ["a", "b", "c"])
    outs = {}
    for name, engine in (("ref", SemLocparOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", double_precision=True)      # noqa: F841
            model = api.build_model(EQ3)
            api.set_covariate(model, "age")
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True, causal_structure=CS3,
                                     output_folder=str(tmp_path / name), _engine=engine)

    def diff(key, col):
        return float(np.abs(outs["hip"][key][col].to_numpy(dtype=np.float64) - outs["ref"][key][col].to_numpy(dtype=np.float64)).max())
    d_eff = diff("marker effects geno", "Estimate")
    d_ebv = max(diff(f"EBV_{tr}", "EBV") for tr in "abc")
    d_ind, d_ov = diff("indirect marker effects geno", "Estimate"), diff("overall marker effects geno", "Estimate")
    a, b = (np.loadtxt(tmp_path / nm / "MCMC_samples_residual_variance.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
    la, lb = (np.loadtxt(tmp_path / nm / "structure_coefficient_MCMC_samples.txt", delimiter=",") for nm in ("ref", "hip"))
    assert a.shape == b.shape == (30, 9) and la.shape == lb.shape == (30, 9)
    d_var, d_lam = float(np.abs(a - b).max()), float(np.abs(la - lb).max())
    print(f"runMCMC SEM: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, variance samples {d_var:.3e}, lambda samples {d_lam:.3e}, "
          f"indirect {d_ind:.3e}, overall {d_ov:.3e}")
    assert d_eff <= 1e-8 and d_ebv <= 1e-7 and d_var <= 1e-9 and d_lam <= 1e-8 and d_ind <= 1e-8 and d_ov <= 1e-8
    assert np.all(lb[:, [1, 2, 5]] != 0.0) and np.any(outs["hip"]["indirect marker effects geno"]["Estimate"] != 0.0)
    np.testing.assert_allclose(outs["hip"]["marker effects geno"]["Model_Frequency"].to_numpy(dtype=np.float64),
                               outs["ref"]["marker effects geno"]["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)


def test_runmcmc_float32_packed_storage_contract(tmp_path, small_data):
    """A Float32 run on 2-bit packed storage: it runs, the files are present, all values finite."""
    from jwas_jl_amd import api, streaming as S
    gdf, ph = SR.sem_phenotypes(small_data, ["a", "b", "c"])
    ph["ID"] = [str(i) for i in range(len(ph))]
    prefix = S.prepare_streaming_genotypes(small_data["raw"].astype(np.float64), tmp_path / "st", obs_ids=list(ph["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", storage="stream")      # noqa: F841
        model = api.build_model(EQ3)
        api.set_covariate(model, "age")
        out = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, causal_structure=CS3, output_folder=str(tmp_path / "r"))
    folder = tmp_path / "r"
    lam = np.loadtxt(folder / "structure_coefficient_MCMC_samples.txt", delimiter=",")
    assert lam.shape == (30, 9) and np.all(np.isfinite(lam)) and np.all(lam[:, [1, 2, 5]] != 0.0) and np.all(lam[:, [0, 3, 4, 6, 7, 8]] == 0.0)
    for kind in ("indirect", "overall"):
        for tr in "abc":
            assert os.path.exists(folder / f"MCMC_samples_{kind}_marker_effects_geno_{tr}.bin")
        tab = out[f"{kind} marker effects geno"]
        assert len(tab) == 3 * 640 and all(np.all(np.isfinite(tab[c])) for c in ("Estimate", "SD", "Model_Frequency"))
    for nm in ("direct", "indirect", "overall"):
        assert os.path.exists(folder / f"{nm}_marker_effects_geno.txt")
    sc = out["structure coefficients"]
    assert len(sc) == 3 and np.all(np.isfinite(sc["Estimate"])) and np.all(np.isfinite(sc["SD"]))
    assert all(np.all(np.isfinite(out[f"EBV_{tr}"]["EBV"])) for tr in "abc") and np.all(np.isfinite(out["marker effects geno"]["Estimate"]))
