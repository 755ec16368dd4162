"""GBLUP on the device (csrc/gblup.hpp) through the C ABI and runMCMC, against the numpy restatements of tests/gblup_reference.py on
the same Philox counters.

1. The relationship matrix, n = 301 and 129 (no multiple of a tile edge), p = c + 13 markers (one full fp32 chunk of c =
   HipEngine.GRM_CHUNK and a ragged tail), both precisions, against the double restatement from the same Z.  The bound is derived:
   (c + 2) 2^-24 (sum_k |z_ik z_jk| + 1e-5) / p in Float32 (a chunk is an fp32 fma chain of c roundings, the chunks meet in double, the
   + 1e-5 and the / p are two more), (p + 2) 2^-53 (...) / p in Float64.  K == K' bit for bit.
2. One step from an uploaded state, n = 301 (two 256-row slices, the second ragged; five column parts and waves, the last ragged),
   L and D from numpy's eigh of a 301 x 700 relationship matrix.  With u = 2^-53 and uT the unit roundoff of the element type:
       r+           the device's is not visible; numpy's T(r + L alpha) differs from it by at most dr = uT |r+| + 2 (n + 2) u sum_j |L_ij alpha_j|
                    (exactly 0 in an iteration that starts from alpha = 0, where r+ = r)
       s            numpy sums of the same products: 2 (n + 2) u sum_i |L_ij r+_i| + sum_i |L_ij| dr_i
       alpha        the restatement evaluated from the device's OWN s (gblup_reference.alpha_bound)
       r            T(r+ - L alpha) from the device's own alpha: dr + 2 (n + 2) u sum_j |L_ij alpha_j| + uT |r|
       statistics   numpy sums of the device's own state: 2 (K + 2) u sum |terms|
   Trait k of a diagonal T-trait step equals a one-trait step with first_trait = k, and two runs are equal, bit for bit.
3. The law of the draws: (alpha - mean) / sd over more than 20 000 (pseudo-marker, iteration) pairs against N(0, 1); in joint mode the
   whitened z of different traits uncorrelated.
4. The exact posterior of y = intercept + a + e through runMCMC (the CPU twin is tests/test_gblup_host.py).
5. genomic_relationship_matrix -> get_genotypes -> runMCMC: names, shapes, finite estimates; the device eigensolver against numpy's.
Every test prints what it measured before it asserts."""
import functools
import os

import numpy as np
import pytest

import draw_laws
import gblup_reference as GR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4
N, SEED = 301, 7


def _ur(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else U


@functools.lru_cache(maxsize=None)
def _genotypes(n, p, seed=3):
    """Centred 0/1/2 genotypes (float64) and the allele frequencies of the uncentred columns."""
    rng = np.random.default_rng(seed)
    freq = 0.1 + 0.8 * rng.random(p)
    X = rng.binomial(2, freq, size=(n, p)).astype(np.float64)
    X[0, X.std(axis=0) == 0] += 1.0
    pf = X.mean(axis=0) / 2
    return X - X.mean(axis=0), pf


@functools.lru_cache(maxsize=None)
def _eigen(dtype_name):
    """(K, L, D) of the 301 x 700 relationship matrix in the element type (numpy's eigh; D spans about 1e-5 .. 3)."""
    dt = np.dtype(dtype_name).type
    Xc, pf = _genotypes(N, 700)
    X = Xc.astype(dt)
    d = np.sqrt(dt(2.0) * pf.astype(dt) * (dt(1.0) - pf.astype(dt))).astype(dt)
    Z = X / d
    K = ((Z @ Z.T + np.eye(N, dtype=dt) * dt(1e-5)) / dt(700)).astype(dt)
    K = ((K + K.T) / dt(2)).astype(dt)
    D, L = np.linalg.eigh(K)
    return K, np.asfortranarray(L), np.abs(D.astype(np.float64))


def _hip(precision):
    import jwas_jl_amd as J
    return J.HipEngine(0, precision=precision)


# ---- 1. the relationship matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("n", [301, 129])
def test_relationship_matrix(n, precision):
    import jwas_jl_amd as J
    c = J.HipEngine.GRM_CHUNK
    p = c + 13
    dt = np.float64 if precision == 64 else np.float32
    Xc, pf = _genotypes(n, p, seed=n)
    X = np.asfortranarray(Xc.astype(dt))
    d = np.sqrt(dt(2.0) * pf.astype(dt) * (dt(1.0) - pf.astype(dt))).astype(dt)
    hip = _hip(precision)
    try:
        hip.load_dense(X)
        K = hip.grm(d)
    finally:
        hip.close()
    ref, absZZ = GR.grm_reference(X, d)
    bound = GR.grm_bound(absZZ, p, dt, c)
    err = np.abs(K.astype(np.float64) - ref)
    print(f"grm n={n} p={p} {np.dtype(dt).name}: worst error / bound {np.max(err / bound):.3f}; symmetric {np.array_equal(K, K.T)}")
    assert K.dtype == dt and K.shape == (n, n)
    assert np.array_equal(K, K.T)
    assert np.all(err <= bound)


def test_relationship_matrix_errors():
    from jwas_jl_amd import _lib
    Xc, pf = _genotypes(129, 40, seed=1)
    X = np.asfortranarray(Xc.astype(np.float32))
    d = np.sqrt(2.0 * pf * (1.0 - pf)).astype(np.float32)

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    hip = _hip(32)
    try:
        hip.n, hip.p = X.shape
        assert code(hip.grm, d) == ESTATE                                   # no genotypes
        hip.alloc_packed(*X.shape)
        assert code(hip.grm, d) == EUNSUP                                   # a packed context
        hip.load_dense(X)
        for bad in (0.0, -1.0, np.inf, np.nan):
            d2 = d.copy()
            d2[17] = bad
            assert code(hip.grm, d2) == EINVAL
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.grm, d) == EUNSUP                                   # shards
        hip.comm_destroy()
        hip.init_state("BayesC", 1)
        assert code(hip.gblup_begin, np.ones(40)) == EINVAL                 # p != n
        assert code(hip.gblup_step, iteration=1, seed=1, vare=1.0, G=1.0) == ESTATE
        assert code(hip.gblup_rhs) == ESTATE and code(hip.gblup_end) == ESTATE
    finally:
        hip.close()
    K, L, D = _eigen("float32")
    hip = _hip(32)
    try:
        hip.load_dense(L)
        assert code(hip.gblup_begin, D) == ESTATE                           # no state
        hip.init_state("BayesC", 1)
        for bad in (0.0, -1e-3, np.inf, np.nan):
            D2 = D.copy()
            D2[5] = bad
            assert code(hip.gblup_begin, D2) == EINVAL
        hip.set_weights(np.linspace(0.5, 2.0, N).astype(np.float32))
        assert code(hip.gblup_begin, D) == EUNSUP                           # residual weights
        hip.set_weights(None)
        hip.gblup_begin(D)
        assert code(hip.gblup_step, iteration=0, seed=1, vare=1.0, G=1.0) == EINVAL
        assert code(hip.gblup_step, iteration=1, seed=1, vare=-1.0, G=1.0) == EINVAL
        assert code(hip.gblup_step, iteration=1, seed=1, vare=1.0, G=1.0, first_trait=4) == EINVAL
        hip.gblup_end()
        assert code(hip.gblup_end) == ESTATE
    finally:
        hip.close()


# ---- 2. one step ------------------------------------------------------------------------------------------------------------------------
MODES = [(1, True)] + [(t, diag) for t in (2, 3, 4) for diag in (True, False)]
STEP_CASES = [(t, diag, prec) for (t, diag) in MODES for prec in (32, 64)]


def _variances(t):
    rng = np.random.default_rng(40 + t)
    A, B = rng.standard_normal((t, t)), rng.standard_normal((t, t))
    return A @ A.T / t + 0.5 * np.eye(t), B @ B.T / t + 0.3 * np.eye(t)      # vare, G


@functools.lru_cache(maxsize=None)
def _start(t):
    rng = np.random.default_rng(t)
    return rng.standard_normal((t, N)), 0.05 * rng.standard_normal((t, N))    # the residual, its perturbation between the two steps


def _run_steps(t, diag, precision, first_trait=0, traits=None, alpha0=None):
    """Two steps from the uploaded state.  Returns per iteration a dict of what the device holds before and after."""
    dt = np.float64 if precision == 64 else np.float32
    K, L, D = _eigen(np.dtype(dt).name)
    vare, G = _variances(t if traits is None else 4)
    r0, shift = _start(t if traits is None else 4)
    if traits is not None:
        vare, G = vare[np.ix_(traits, traits)], G[np.ix_(traits, traits)]
        r0, shift = r0[traits], shift[traits]
    hip = _hip(precision)
    out = []
    try:
        hip.load_dense(L)
        hip.init_state("BayesC" if t == 1 else "MTBayesC", t)
        hip.gblup_begin(D)
        for k in range(t):
            hip.set_residual(r0[k].astype(dt), k)
            if alpha0 is not None:
                hip.set_state(k, alpha=alpha0[k].astype(dt))
        for it in (1, 2):
            if it == 2:
                for k in range(t):
                    hip.set_residual((hip.get_residual(k).astype(np.float64) + shift[k]).astype(dt), k)
            before = {"r": np.stack([hip.get_residual(k) for k in range(t)]), "alpha": np.stack([hip.get_state(k)[0] for k in range(t)])}
            st = hip.gblup_step(iteration=it, seed=SEED, vare=vare, G=G, diagonal=diag, first_trait=first_trait)
            after = {"r": np.stack([hip.get_residual(k) for k in range(t)]), "alpha": np.stack([hip.get_state(k)[0] for k in range(t)]),
                     "beta": np.stack([hip.get_state(k)[1] for k in range(t)]), "s": hip.gblup_rhs(), "st": st}
            out.append((before, after))
    finally:
        hip.close()
    return out, (L, D, vare, G)


@pytest.mark.parametrize("t,diag,precision", STEP_CASES)
def test_one_step(t, diag, precision):
    dt = np.float64 if precision == 64 else np.float32
    ur = _ur(dt)
    steps, (L, D, vare, G) = _run_steps(t, diag, precision)
    L64, aL = L.astype(np.float64), np.abs(L.astype(np.float64))
    worst = {"s": 0.0, "alpha": 0.0, "r": 0.0, "stat": 0.0}
    for it, (b, a) in zip((1, 2), steps):
        r0, a0 = b["r"].astype(np.float64), b["alpha"].astype(np.float64)
        rplus = (r0 + a0 @ L64.T).astype(dt).astype(np.float64)
        dr = np.zeros_like(rplus) if not a0.any() else ur * np.abs(rplus) + 2 * (N + 2) * U * (np.abs(a0) @ aL.T)
        # the right-hand sides
        s_ref = (rplus @ L64).T
        s_bound = (2 * (N + 2) * U * (np.abs(rplus) @ aL) + dr @ aL).T
        es = np.abs(a["s"] - s_ref)
        worst["s"] = max(worst["s"], float(np.max(es / s_bound)))
        assert np.all(es <= s_bound), ("s", it)
        # every effect from the device's own s
        z = GR.draws(N, t, it, SEED)
        a_ref, a_bound, _ = GR.alpha_bound(a["s"], D, z, vare, G, diag, dt)
        ea = np.abs(a["alpha"].astype(np.float64).T - a_ref)
        worst["alpha"] = max(worst["alpha"], float(np.max(ea / a_bound)))
        assert np.all(ea <= a_bound), ("alpha", it, float(np.max(ea / a_bound)))
        assert np.array_equal(a["alpha"], a["beta"])
        # the residual from the device's own effects
        a1 = a["alpha"].astype(np.float64)
        r_ref = rplus - a1 @ L64.T
        r_bound = dr + 2 * (N + 2) * U * (np.abs(a1) @ aL.T) + ur * np.abs(r_ref)
        er = np.abs(a["r"].astype(np.float64) - r_ref)
        worst["r"] = max(worst["r"], float(np.max(er / r_bound)))
        assert np.all(er <= r_bound), ("r", it)
        # the statistics from the device's own state
        r1 = a["r"].astype(np.float64)
        for key, got, ref, absref, K_ in (("alpha_ss", a["st"]["alpha_ss"], (a1 / D) @ a1.T, (np.abs(a1) / D) @ np.abs(a1).T, N),
                                          ("resid_ss", a["st"]["resid_ss"], r1 @ r1.T, np.abs(r1) @ np.abs(r1).T, N),
                                          ("resid_sum", a["st"]["resid_sum"], r1.sum(axis=1), np.abs(r1).sum(axis=1), N)):
            bnd = 2 * (K_ + 2) * U * absref
            e = np.abs(np.asarray(got) - ref)
            worst["stat"] = max(worst["stat"], float(np.max(e / bnd)))
            assert np.all(e <= bnd), (key, it)
    print(f"step t={t} {'diagonal' if diag else 'joint'} {np.dtype(dt).name}: worst error / bound  s {worst['s']:.3f}  alpha {worst['alpha']:.3f}  "
          f"r {worst['r']:.3f}  statistics {worst['stat']:.3f}")


def _same(x, y):
    for (b1, a1), (b2, a2) in zip(x, y):
        for key in ("r", "alpha", "s"):
            if not np.array_equal(a1[key], a2[key]):
                return False
        for key in ("alpha_ss", "resid_ss", "resid_sum"):
            if not np.array_equal(a1["st"][key], a2["st"][key]):
                return False
    return True


@pytest.mark.parametrize("precision", [32, 64])
def test_two_runs_give_identical_bits(precision):
    for t, diag in ((1, True), (3, True), (4, False)):
        x, _ = _run_steps(t, diag, precision)
        y, _ = _run_steps(t, diag, precision)
        same = _same(x, y)
        print(f"two runs t={t} {'diagonal' if diag else 'joint'} {precision}: identical {same}")
        assert same


@pytest.mark.parametrize("precision", [32, 64])
def test_trait_of_a_diagonal_step_is_a_one_trait_step(precision):
    many, _ = _run_steps(4, True, precision)
    for k in range(4):
        one, _ = _run_steps(1, True, precision, first_trait=k, traits=[k])
        for it in range(2):
            am, ao = many[it][1], one[it][1]
            eq = [np.array_equal(am["alpha"][k], ao["alpha"][0]), np.array_equal(am["r"][k], ao["r"][0]), np.array_equal(am["s"][:, k], ao["s"][:, 0]),
                  am["st"]["alpha_ss"][k, k] == ao["st"]["alpha_ss"][0, 0], am["st"]["resid_ss"][k, k] == ao["st"]["resid_ss"][0, 0],
                  am["st"]["resid_sum"][k] == ao["st"]["resid_sum"][0]]
            print(f"trait {k} of 4 against a one-trait step, iteration {it + 1}, {precision}: {eq}")
            assert all(eq)


# ---- 3. the law of the draws --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,diag", [(1, True), (3, False)])
def test_draw_law(t, diag):
    niter = 70
    K, L, D = _eigen("float64")
    vare, G = _variances(t)
    r0, _ = _start(t)
    zs = []
    hip = _hip(64)
    try:
        hip.load_dense(L)
        hip.init_state("BayesC" if t == 1 else "MTBayesC", t)
        hip.gblup_begin(D)
        for k in range(t):
            hip.set_residual(r0[k], k)
        for it in range(1, niter + 1):
            hip.gblup_step(iteration=it, seed=SEED, vare=vare, G=G, diagonal=diag)
            s = hip.gblup_rhs()
            a = np.stack([hip.get_state(k)[0] for k in range(t)], axis=1)
            _, info = GR.sample_from_rhs(s, D, np.zeros((N, t)), vare, G, diag)
            if diag:
                zs.append((a - info["mean"]) / info["sd"])
            else:
                zs.append(np.stack([np.linalg.solve(info["C"][i], a[i] - info["mean"][i]) for i in range(N)]))
    finally:
        hip.close()
    z = np.concatenate(zs)
    Nz = len(z)
    ks = max(draw_laws.ks_stat(z[:, k], draw_laws.norm_cdf) for k in range(t))
    corr = draw_laws.max_offdiag_corr(z) if t > 1 else 0.0
    print(f"draw law t={t} {'diagonal' if diag else 'joint'}: N {Nz} per trait, KS {ks:.5f} (bound {draw_laws.ks_bound(Nz):.5f}), "
          f"largest correlation between traits {corr:.5f} (bound {draw_laws.corr_bound(Nz):.5f})")
    assert Nz >= 20_000
    assert ks <= draw_laws.ks_bound(Nz)
    assert corr <= draw_laws.corr_bound(Nz)


# ---- 4. the exact posterior through runMCMC -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,n,double_precision", [(1, 24, False), (2, 12, True)])
def test_exact_posterior(tmp_path, t, n, double_precision):
    from jwas_jl_amd import api
    case = GR.posterior_case(t, n)
    ebv, geno = GR.run_posterior_chain(api, case, None, str(tmp_path / "run"), double_precision=double_precision)
    Ea, Eaa = GR.mme_posterior(case["Y"], geno.genotypes.astype(np.float64), case["R"], case["G"])
    draw_laws.assert_effect_moments(ebv, Ea, Eaa, f"GBLUP on the device, {t} trait(s), n = {n}")


# ---- 5. whole calls -------------------------------------------------------------------------------------------------------------------------
def _whole_case(n=60, p=150, t=1, seed=2):
    import pandas as pd
    rng = np.random.default_rng(seed)
    X = rng.binomial(2, 0.2 + 0.6 * rng.random(p), size=(n, p)).astype(np.float64)
    ids = [f"id{i + 1}" for i in range(n)]
    gdf = pd.DataFrame(X, columns=[f"m{j + 1}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    b = rng.standard_normal((p, t)) * 0.2
    Y = 2.0 + (X - X.mean(axis=0)) @ b + rng.standard_normal((n, t))
    ph = pd.DataFrame({"ID": ids, **{f"y{k + 1}": Y[:, k] for k in range(t)}, "herd": [f"h{i % 4}" for i in range(n)]})
    return gdf, ph


@pytest.mark.parametrize("t,double_precision,locpar,random,outside,eigen", [(1, False, "host", False, False, "device"), (1, True, "device", True, False, "host"),
                                                                           (3, False, "device", False, True, "host"), (3, True, "host", False, False, "auto")])
def test_whole_call(tmp_path, t, double_precision, locpar, random, outside, eigen):
    from jwas_jl_amd import api
    gdf, ph = _whole_case(t=t)
    n = len(ph)
    Kdf = api.genomic_relationship_matrix(gdf, double_precision=double_precision)
    assert list(Kdf.columns[1:]) == list(gdf["ID"]) and Kdf.shape == (n, n + 1)
    Gv = 0.5 if t == 1 else 0.5 * np.eye(t) + 0.1
    geno = api.get_genotypes(Kdf, Gv, method="GBLUP", double_precision=double_precision)
    rhs = "intercept + herd + geno" if random else "intercept + geno"
    model = api.build_model("\n".join(f"y{k + 1} = {rhs}" for k in range(t)), genotypes={"geno": geno})
    if random:
        api.set_random(model, "herd")
    if outside:
        ph = ph.iloc[:45].reset_index(drop=True)
        api.outputEBV(model, list(gdf["ID"])[30:])
    folder = str(tmp_path / "run")
    try:
        out = api.runMCMC(model, ph, chain_length=60, burnin=10, seed=3, output_folder=folder, double_precision=double_precision,
                          location_parameters=locpar, gblup_eigen=eigen)
    except RuntimeError as ex:
        if eigen != "device" or "torch.linalg.eigh is not usable" not in str(ex):
            raise
        print(f"gblup_eigen=\"device\": {ex}")
        pytest.skip(f"torch.linalg.eigh itself raised: {ex}")
    files = sorted(os.listdir(folder))
    print(f"whole call t={t} double={double_precision} location={locpar} random={random} outside={outside} eigen={eigen}: {len(files)} files, tables {sorted(k for k in out if not k.startswith('_'))}")
    assert "MCMC_samples_genetic_variance(REML)_geno.txt" in files and "MCMC_samples_marker_effects_variances_geno.txt" not in files
    for k in range(t):
        ebv = out[f"EBV_y{k + 1}"]
        assert len(ebv) == (n - 30 if outside else len(ph)) and np.isfinite(ebv["EBV"].to_numpy(dtype=np.float64)).all()
        assert f"MCMC_samples_marker_effects_geno_y{k + 1}.txt" in files
    me = out["marker effects geno"]
    assert len(me) == t * len(ph) and np.isfinite(me["Estimate"].to_numpy(dtype=np.float64)).all()
    for key in ("marker effects variance geno", "residual variance", "genetic_variance", "heritability", "location parameters"):
        assert np.isfinite(out[key]["Estimate"].to_numpy(dtype=np.float64)).all(), key
    assert len(out["marker effects variance geno"]) == t * t


@pytest.mark.parametrize("double_precision", [False, True])
def test_device_eigensolver(double_precision):
    """||L'L - I|| and ||L D L' - K|| of the device solver no worse than 4 x numpy's on the same matrix in the same precision (two
    backward-stable solvers differ by a constant).  Skips only if torch.linalg.eigh itself cannot run, and says so."""
    from jwas_jl_amd import gblup
    dt = "float64" if double_precision else "float32"
    K, _, _ = _eigen(dt)

    def norms(D, L):
        L64, K64 = L.astype(np.float64), K.astype(np.float64)
        return np.linalg.norm(L64.T @ L64 - np.eye(N)), np.linalg.norm((L64 * D.astype(np.float64)) @ L64.T - K64)

    host = norms(*gblup.eigh_host(K))
    try:
        Dd, Ld = gblup.eigh_device(K, 0)
    except RuntimeError as ex:
        print(f"torch.linalg.eigh is not usable here: {ex}")
        pytest.skip(f"torch.linalg.eigh itself raised: {ex}")
    dev = norms(Dd, Ld)
    print(f"eigensolver {dt}: ||L'L - I|| device {dev[0]:.3e} host {host[0]:.3e} (ratio {dev[0] / host[0]:.2f}); "
          f"||L D L' - K|| device {dev[1]:.3e} host {host[1]:.3e} (ratio {dev[1] / host[1]:.2f})")
    assert Ld.dtype == K.dtype
    assert dev[0] <= 4 * host[0] and dev[1] <= 4 * host[1]
