"""TEST INFRASTRUCTURE: exact laws of the draws, in numpy / scipy and float64 only -- nothing here restates a kernel.  The
device tests (tests/test_gpu_draw_laws.py, tests/test_gpu_statistical.py) and their CPU twins on the oracle and the stand-ins
(tests/test_draw_laws_host.py) call the same functions with the same inputs and the same bounds.

Bounds.  ks_bound is the Dvoretzky-Kiefer-Wolfowitz-Massart inequality  P(D > eps) <= 2 exp(-2 N eps^2)  solved for eps at
P = alpha: it holds at every finite N, so a test fails by chance with probability <= alpha per statistic.  corr_bound is five
standard deviations of a sample correlation of independent variables (sd ~ 1 / sqrt(N))."""
import itertools
import math

import numpy as np
from scipy import special


def ks_bound(N, alpha=1e-6):
    return math.sqrt(math.log(2.0 / alpha) / 2.0) / math.sqrt(N)


def corr_bound(N):
    return 5.0 / math.sqrt(N)


def norm_cdf(x):
    return special.ndtr(x)


def chi2_cdf(nu):
    return lambda x: special.gammainc(0.5 * nu, 0.5 * np.asarray(x, dtype=np.float64))


def ks_stat(x, cdf):
    """Two-sided Kolmogorov-Smirnov statistic of the sample x against the continuous law with distribution function cdf."""
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    N = len(x)
    F = cdf(x)
    i = np.arange(1, N + 1)
    return float(max(np.max(i / N - F), np.max(F - (i - 1) / N)))


def max_offdiag_corr(cols):
    """Largest |sample correlation| between two different columns of cols (N x q)."""
    c = np.corrcoef(np.asarray(cols, dtype=np.float64), rowvar=False)
    c = np.atleast_2d(c)
    return float(np.max(np.abs(c - np.diag(np.diag(c))))) if c.shape[0] > 1 else 0.0


# ---- A. inverse-Wishart / scaled-inverse-chi2 draws ---------------------------------------------------------------------
IW_P, IW_ITERATIONS, IW_SEED, IW_MARKER0 = 20_000, tuple(range(1, 11)), 11, 1000


def iw_inputs(t, p=IW_P):
    """scale (t x t, float64) and beta (t x p, float32): every 7th marker zero, markers 3, 14, 25, ... twenty times as large."""
    rng = np.random.default_rng(100 * t)
    A = rng.standard_normal((t, t))
    scale = (A @ A.T / t + np.eye(t)) * 0.01
    beta = (0.05 * rng.standard_normal((t, p))).astype(np.float32)
    beta[:, ::7] = 0.0
    beta[:, 3::11] *= np.float32(20.0)
    return scale, beta


def iw_psi(scale, beta):
    """Psi_j = scale + b_j b_j' (p x t x t, float64)."""
    b = np.asarray(beta, dtype=np.float64).T
    return np.asarray(scale, dtype=np.float64)[None] + b[:, :, None] * b[:, None, :]


def bartlett_factors(G, Psi):
    """Whitening by Bartlett's theorem.  G ~ InverseWishart(df, Psi), Psi = C C'  =>  M = C^-1 G C^-T ~ IW(df, I), M^-1 ~
    Wishart(df, I) and its lower Cholesky factor L has independent entries, L_ii^2 ~ chi2(df - i) (i from 0), L_ik ~ N(0, 1) for
    k < i.  Returns (L, ok): L is N x t x t (rows of draws with ok = False are meaningless), ok marks the draws whose M^-1 is
    positive definite in float64."""
    G = np.asarray(G, dtype=np.float64)
    C = np.linalg.cholesky(Psi)
    Y = np.linalg.solve(C, G)                                           # C^-1 G
    M = np.linalg.solve(C, Y.transpose(0, 2, 1))                        # C^-1 (C^-1 G)' = C^-1 G C^-T (G symmetric)
    M = 0.5 * (M + M.transpose(0, 2, 1))
    t = G.shape[1]
    ok = np.isfinite(M).all(axis=(1, 2))
    M[~ok] = np.eye(t)
    ok &= np.linalg.eigvalsh(M)[:, 0] > 0                               # (M^-1 is definite exactly when M is)
    M[~ok] = np.eye(t)
    W = np.linalg.inv(M)
    W = 0.5 * (W + W.transpose(0, 2, 1))
    ok &= np.isfinite(W).all(axis=(1, 2))
    W[~ok] = np.eye(t)
    ok &= np.linalg.eigvalsh(W)[:, 0] > 0
    W[~ok] = np.eye(t)
    return np.linalg.cholesky(W), ok


def bartlett_check(G, Psi, df):
    """{"ks": worst KS D over the t (t + 1) / 2 entries of L, "corr": their worst pairwise correlation, "excluded": the share
    of draws left out because M^-1 was not positive definite, "N": draws used}."""
    L, ok = bartlett_factors(G, Psi)
    t = L.shape[1]
    L = L[ok]
    cols, worst = [], 0.0
    for i in range(t):
        for k in range(i + 1):
            if k == i:
                q = L[:, i, i] ** 2
                worst = max(worst, ks_stat(q, chi2_cdf(df - i)))
            else:
                q = L[:, i, k]
                worst = max(worst, ks_stat(q, norm_cdf))
            cols.append(q)
    return {"ks": worst, "corr": max_offdiag_corr(np.stack(cols, axis=1)), "excluded": 1.0 - float(ok.mean()), "N": int(ok.sum())}


def pivot_vectors(t, unit_only=False):
    vs = [np.eye(t)[k] for k in range(t)]
    if not unit_only:
        vs += [np.ones(t), np.array([1.0, -2.0, 3.0, -4.0])[:t]]
    return vs


def pivot_check(G, Psi, df, unit_only=False):
    """The inverse-free pivots (a' Psi a) / (a' G a) ~ chi2(df - t + 1): worst KS D over the vectors a."""
    G = np.asarray(G, dtype=np.float64)
    t = G.shape[1]
    worst = 0.0
    for a in pivot_vectors(t, unit_only):
        q = np.einsum("a,jab,b->j", a, Psi, a) / np.einsum("a,jab,b->j", a, G, a)
        worst = max(worst, ks_stat(q, chi2_cdf(df - t + 1)))
    return worst


def diagonal_check(G, Psi, df):
    """constraint = true: (scale_kk + b_k^2) / G_kk ~ chi2(df) for every trait k: worst KS D."""
    G = np.asarray(G, dtype=np.float64)
    t = G.shape[1]
    return max(ks_stat(Psi[:, k, k] / G[:, k, k], chi2_cdf(df)) for k in range(t))


def assert_iw_law(G, Psi, df, tag, *, bartlett=True, max_excluded=0.0, unit_only=False):
    """What both the device tests and their CPU twins assert of N = len(G) draws G_j ~ InverseWishart(df, Psi_j)."""
    N, t = len(G), G.shape[1]
    assert np.isfinite(G).all() and np.array_equal(G, G.transpose(0, 2, 1)), f"{tag}: a draw is not finite or not symmetric"
    kb = ks_bound(N)
    piv = pivot_check(G, Psi, df, unit_only)
    print(f"draw-law {tag} t{t} df={df}: pivots KS D {piv:.5f} (bound {kb:.5f}, N {N})")
    assert piv <= kb, (tag, "pivot", piv, kb)
    if bartlett:
        b = bartlett_check(G, Psi, df)
        print(f"draw-law {tag} t{t} df={df}: Bartlett KS D {b['ks']:.5f} (bound {ks_bound(b['N']):.5f}), correlation {b['corr']:.5f} "
              f"(bound {corr_bound(b['N']):.5f}), excluded share {b['excluded']:.2e} (allowed {max_excluded:.0e}), N {b['N']}")
        assert b["excluded"] <= max_excluded, (tag, "excluded", b["excluded"])
        assert b["ks"] <= ks_bound(b["N"]) and b["corr"] <= corr_bound(b["N"]), (tag, b)


def assert_diagonal_law(G, Psi, df, tag):
    N, t = len(G), G.shape[1]
    off = ~np.eye(t, dtype=bool)
    assert np.isfinite(G).all() and (G[:, off] == 0).all() and (G[:, ~off] > 0).all(), f"{tag}: off-diagonals must be exactly 0"
    d = diagonal_check(G, Psi, df)
    print(f"draw-law {tag} diagonal t{t} df={df}: KS D {d:.5f} (bound {ks_bound(N):.5f}, N {N})")
    assert d <= ks_bound(N), (tag, d)


def assert_imputation_law(R, codes, before, after, tag):
    t = R.shape[0]
    res = imputation_check(R, codes, before, after)
    assert len(res) == (1 << t) - 2
    worst_ks = max(v["ks"] / ks_bound(v["N"]) for v in res.values())
    worst_c = max(v["corr"] / corr_bound(v["N"]) for v in res.values())
    N = min(v["N"] for v in res.values())
    print(f"draw-law {tag} imputation t{t}: worst KS D {max(v['ks'] for v in res.values()):.5f} = {worst_ks:.2f} of its bound "
          f"{ks_bound(N):.5f}; worst correlation {max(v['corr'] for v in res.values()):.5f} = {worst_c:.2f} of its bound "
          f"{corr_bound(N):.5f}; N {N} per pattern, {len(res)} patterns")
    for code, v in res.items():
        assert v["ks"] <= ks_bound(v["N"]) and v["corr"] <= corr_bound(v["N"]), (tag, code, v)


# ---- B. imputation of missing traits ------------------------------------------------------------------------------------
MT_PER_PATTERN, MT_SEED, MT_ITERATION = 14_000, 77, 2


def mtmiss_inputs(t):
    """R (t x t), the shuffled codes (every code 1 .. 2^t - 1, MT_PER_PATTERN records each) and e (t x n, float64)."""
    rng = np.random.default_rng(9)
    A = rng.standard_normal((t, t))
    R = (A @ A.T / t + np.eye(t)) * 0.7
    R = 0.5 * (R + R.T)
    codes = np.repeat(np.arange(1, 1 << t), MT_PER_PATTERN).astype(np.int32)
    rng.shuffle(codes)
    e = 1.3 * rng.standard_normal((t, len(codes)))
    return R, codes, e


def imputation_check(R, codes, before, after):
    """Per incomplete pattern: e_m | e_o ~ N(R_mo R_oo^-1 e_o, R_mm - R_mo R_oo^-1 R_om), from R alone.  The whitened
    z = chol(S)^-1 (e_m - mean) must be N(0, I) and uncorrelated with e_o.  Returns {code: {"ks", "corr", "N"}}; asserts that
    observed cells and complete records are bit-unchanged."""
    t = R.shape[0]
    full = (1 << t) - 1
    out = {}
    for code in range(1, full + 1):
        rows = np.flatnonzero(codes == code)
        o = [k for k in range(t) if (code >> k) & 1]
        m = [k for k in range(t) if not (code >> k) & 1]
        assert np.array_equal(after[o][:, rows], before[o][:, rows]), f"code {code}: an observed cell changed"
        if code == full:
            continue
        eo = before[o][:, rows].astype(np.float64)
        em = after[m][:, rows].astype(np.float64)
        Roo, Rmo, Rmm = R[np.ix_(o, o)], R[np.ix_(m, o)], R[np.ix_(m, m)]
        Bc = Rmo @ np.linalg.inv(Roo)
        S = Rmm - Bc @ Rmo.T
        z = np.linalg.solve(np.linalg.cholesky(0.5 * (S + S.T)), em - Bc @ eo)
        ks = max(ks_stat(z[c], norm_cdf) for c in range(len(m)))
        cc = np.corrcoef(np.vstack([z, eo]))
        blk = np.abs(cc[:len(m)] - np.eye(len(m), len(m) + len(o)))
        out[code] = {"ks": ks, "corr": float(blk.max()), "N": len(rows)}
    return out


# ---- C. exact moments of the effects under the enumerated state posterior ------------------------------------------------
def _normalise(logp):
    mx = max(logp.values())
    tot = sum(math.exp(v - mx) for v in logp.values())
    return {s: math.exp(v - mx) / tot for s, v in logp.items()}


def exact_mixture_moments(X, y, vare, class_vars, class_probs):
    """y = X a + e, e ~ N(0, vare I), a_j | class k ~ N(0, class_vars[k]) (class_vars[0] = 0: a_j = 0), by enumeration of the
    K^p states s:  P(s | y) ~ prod_j class_probs[s_j] N(y; 0, vare I + X D_s X'),  a | s, y ~ N(m_s, V_s) on the markers in the
    model with V_s = (X_s' X_s / vare + D_s^-1)^-1, m_s = V_s X_s' y / vare.
    Returns (P, E[a], E[a a']): P maps state -> probability."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = X.shape
    logp, cond = {}, {}
    for s in itertools.product(range(len(class_vars)), repeat=p):
        d = np.array([class_vars[k] for k in s], dtype=np.float64)
        V = vare * np.eye(n) + (X * d) @ X.T
        logp[s] = -0.5 * (np.linalg.slogdet(V)[1] + y @ np.linalg.solve(V, y)) + sum(math.log(class_probs[k]) for k in s)
        act = np.flatnonzero(d > 0)
        m, C = np.zeros(p), np.zeros((p, p))
        if len(act):
            Xs = X[:, act]
            Vs = np.linalg.inv(Xs.T @ Xs / vare + np.diag(1.0 / d[act]))
            m[act] = Vs @ (Xs.T @ y) / vare
            C[np.ix_(act, act)] = Vs
        cond[s] = (m, C)
    P = _normalise(logp)
    Ea = sum(P[s] * cond[s][0] for s in P)
    Eaa = sum(P[s] * (cond[s][1] + np.outer(cond[s][0], cond[s][0])) for s in P)
    return P, Ea, Eaa


def exact_mixture_moments_mt(X, Y, R, G, prior):
    """The Kronecker form for t traits: vec(Y) (trait-major) ~ N(0, R (x) I + sum_j (D_j G_j D_j) (x) x_j x_j'), D_j = diag of
    marker j's joint state (bit k = trait k in the model).  G is t x t, or p x t x t (one per marker); prior is [2^t] or p x [2^t].
    The effects are ordered trait-major, a[k * p + j].  Returns (P, E[a], E[a a']); P maps (state_1 .. state_p) -> probability."""
    X, Y, R = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(R, dtype=np.float64)
    n, p = X.shape
    t = R.shape[0]
    G = np.asarray(G, dtype=np.float64)
    Gj = np.broadcast_to(G, (p, t, t))
    prior = np.broadcast_to(np.asarray(prior, dtype=np.float64), (p, 1 << t))
    yv = Y.reshape(-1)
    Z = np.kron(np.eye(t), X)                                           # column k * p + j
    Ri = np.kron(np.linalg.inv(R), np.eye(n))
    ZRZ, ZRy = Z.T @ Ri @ Z, Z.T @ Ri @ yv
    logp, cond = {}, {}
    for conf in itertools.product(range(1 << t), repeat=p):
        K = np.zeros((t * p, t * p))                                    # prior covariance of the effects under conf
        for j, st in enumerate(conf):
            D = np.diag([float((st >> k) & 1) for k in range(t)])
            idx = [k * p + j for k in range(t)]
            K[np.ix_(idx, idx)] = D @ Gj[j] @ D
        V = np.kron(R, np.eye(n)) + Z @ K @ Z.T
        logp[conf] = -0.5 * (np.linalg.slogdet(V)[1] + yv @ np.linalg.solve(V, yv)) + sum(math.log(prior[j, st]) for j, st in enumerate(conf))
        act = np.flatnonzero(np.diag(K) > 0)
        m, C = np.zeros(t * p), np.zeros((t * p, t * p))
        if len(act):
            Vs = np.linalg.inv(ZRZ[np.ix_(act, act)] + np.linalg.inv(K[np.ix_(act, act)]))
            m[act] = Vs @ ZRy[act]
            C[np.ix_(act, act)] = Vs
        cond[conf] = (m, C)
    P = _normalise(logp)
    Ea = sum(P[s] * cond[s][0] for s in P)
    Eaa = sum(P[s] * (cond[s][1] + np.outer(cond[s][0], cond[s][0])) for s in P)
    return P, Ea, Eaa


def moments_check(samples, Ea, Eaa, nbatch=50):
    """samples: niter x q draws of the effects after burn-in.  Standard errors from nbatch batch means.  Returns
    {"dev1": worst |mean - E a| / SE, "dev2": worst |mean(a a') - E a a'| / SE, "se_sd": worst SE(mean) / exact posterior sd}."""
    a = np.asarray(samples, dtype=np.float64)
    nb = (len(a) // nbatch) * nbatch
    a = a[:nb]
    q = a.shape[1]
    aa = (a[:, :, None] * a[:, None, :]).reshape(nb, q * q)

    def mean_se(x):
        bm = x.reshape(nbatch, nb // nbatch, -1).mean(axis=1)
        return x.mean(axis=0), bm.std(axis=0, ddof=1) / math.sqrt(nbatch)
    m1, se1 = mean_se(a)
    m2, se2 = mean_se(aa)
    sd = np.sqrt(np.diag(Eaa) - Ea ** 2)
    ex2 = Eaa.reshape(-1)
    live2 = (se2 > 0) | (ex2 != 0)                                      # (a pair that is zero in every state and every draw)
    dev2 = np.abs(m2 - ex2)[live2] / np.where(se2[live2] > 0, se2[live2], np.finfo(float).tiny)
    return {"dev1": float(np.max(np.abs(m1 - Ea) / se1)), "dev2": float(np.max(dev2)), "se_sd": float(np.max(se1 / sd))}


# ---- C. the exact-posterior chains: cases, runner and asserts shared by the device tests and their CPU twins --------------
CHAIN_SWEEPS, CHAIN_BURN = 30_000, 500


def st_chain_case(method):
    """Three correlated markers, fixed hyper-parameters (tests/test_gpu_statistical.py's case since its first version)."""
    rng = np.random.default_rng(12)
    n, p = 40, 3
    z = rng.standard_normal((n, 1))
    X = (0.6 * z + rng.standard_normal((n, p))).astype(np.float32)
    X -= X.mean(0)
    y = (0.9 * X[:, 0] + 0.5 * rng.standard_normal(n)).astype(np.float32)
    y -= y.mean()
    vare = 0.6
    if method == "BayesC":
        pi, varg = 0.6, 0.3
        return dict(method=method, X=X, y=y, vare=vare, class_vars=[0.0, varg], class_probs=[pi, 1 - pi], seed=77,
                    kw=dict(vare=np.float32(vare), var_effect=np.float32(varg), pi=pi), delta0=np.zeros(p, dtype=np.float32), shift=0)
    pis, sig = np.array([0.5, 0.2, 0.2, 0.1]), 0.5
    gam = np.array([0.0, 0.01, 0.1, 1.0])
    return dict(method=method, X=X, y=y, vare=vare, class_vars=list(gam * sig), class_probs=list(pis), seed=77,
                kw=dict(vare=np.float32(vare), var_effect=np.float32(sig), pi_classes=pis), delta0=np.ones(p, dtype=np.int32), shift=1)


def run_st_chain(e, case, dtype=np.float32):
    """CHAIN_SWEEPS sweeps on engine e (the device's or the oracle's protocol).  Returns ({state: count}, alpha samples after
    burn-in as (CHAIN_SWEEPS - CHAIN_BURN) x p float64)."""
    X, y = case["X"].astype(dtype), case["y"].astype(dtype)
    e.load_dense(np.asfortranarray(X)); e.setup_blocks(64, "f64"); e.init_state(case["method"])
    e.set_residual(y)
    e.set_state(delta=case["delta0"])
    kw = case["kw"] if dtype == np.float32 else {k: (float(v) if np.ndim(v) == 0 else v) for k, v in case["kw"].items()}
    counts, alphas = {}, np.empty((CHAIN_SWEEPS - CHAIN_BURN, X.shape[1]))
    for it in range(1, CHAIN_SWEEPS + 1):
        e.sweep(iteration=it, seed=case["seed"], **kw)
        if it > CHAIN_BURN:
            a, _, d = e.get_state()
            s = tuple(int(v) - case["shift"] for v in d)
            counts[s] = counts.get(s, 0) + 1
            alphas[it - CHAIN_BURN - 1] = a
    return counts, alphas


def mt_chain_case(kind):
    """Two correlated markers, two traits, 4 joint states each.  kind: "MTBayesC" / "MTBayesC_II" (samplers I and II, one G),
    "MegaBayesC" (constraint = true: diagonal R and G, one pi per trait), "MTBayesB" (one fixed G per marker, handed in)."""
    rng = np.random.default_rng(3)
    n, p, t = 30, 2, 2
    z = rng.standard_normal((n, 1))
    X = (0.5 * z + rng.standard_normal((n, p))).astype(np.float32)
    X -= X.mean(0)
    R = np.array([[0.7, 0.2], [0.2, 0.5]])
    G = np.array([[0.4, 0.15], [0.15, 0.3]])
    Y = np.stack([0.8 * X[:, 0] + 0.3 * rng.standard_normal(n), 0.5 * X[:, 0] - 0.4 * X[:, 1] + 0.3 * rng.standard_normal(n)]).astype(np.float32)
    Y -= Y.mean(axis=1, keepdims=True)
    prior = np.array([0.4, 0.2, 0.15, 0.25])                      # state index = delta_1 + 2 delta_2 (traits)
    case = dict(method=kind, X=X, Y=Y, R=R, G=G, prior=prior, seed=5)
    if kind == "MegaBayesC":
        pi = np.array([0.55, 0.35])                               # P(delta_k = 0)
        case.update(R=np.diag(np.diag(R)), G=np.diag(np.diag(G)),
                    prior=np.array([pi[0] * pi[1], (1 - pi[0]) * pi[1], pi[0] * (1 - pi[1]), (1 - pi[0]) * (1 - pi[1])]))
        case["kw"] = dict(vare=case["R"], var_effect=case["G"], pi=pi)
    elif kind == "MTBayesB":
        case["G"] = np.stack([G, np.array([[0.25, -0.1], [-0.1, 0.5]])])
        case["kw"] = dict(vare=R, var_effect=np.eye(t), var_effect_matrix=case["G"], log_prior_states=np.log(prior))
    else:
        case["kw"] = dict(vare=R, var_effect=G, log_prior_states=np.log(prior))
    return case


def run_mt_chain(e, case, dtype=np.float32):
    """As run_st_chain; the alpha samples are trait-major, a[k * p + j] (exact_mixture_moments_mt's order)."""
    X, Y = case["X"].astype(dtype), case["Y"].astype(dtype)
    t, p = Y.shape[0], X.shape[1]
    e.load_dense(np.asfortranarray(X)); e.setup_blocks(64, "f64"); e.init_state(case["method"], t)
    for k in range(t):
        e.set_residual(Y[k], k)
    kw = {k: (np.asarray(v, dtype=dtype) if k in ("vare", "var_effect", "var_effect_matrix") else v) for k, v in case["kw"].items()}
    counts, alphas = {}, np.empty((CHAIN_SWEEPS - CHAIN_BURN, t * p))
    for it in range(1, CHAIN_SWEEPS + 1):
        e.sweep(iteration=it, seed=case["seed"], **kw)
        if it > CHAIN_BURN:
            st = [e.get_state(k) for k in range(t)]
            s = tuple(sum(int(st[k][2][j] != 0) << k for k in range(t)) for j in range(p))
            counts[s] = counts.get(s, 0) + 1
            alphas[it - CHAIN_BURN - 1] = np.concatenate([st[k][0] for k in range(t)])
    return counts, alphas


def assert_effect_moments(alphas, Ea, Eaa, tag):
    """Every first and second moment of the effects within 5 SE (50 batch means) of the enumeration's, and every SE of a mean
    <= 0.02 of the exact posterior sd -- a stuck chain must not pass by having no spread."""
    m = moments_check(alphas, Ea, Eaa)
    print(f"exact-posterior effects {tag}: means within {m['dev1']:.2f} SE, second moments within {m['dev2']:.2f} SE (bound 5); "
          f"worst SE of a mean {m['se_sd']:.4f} of the posterior sd (bound 0.02); N {len(alphas)}")
    assert m["dev1"] <= 5.0 and m["dev2"] <= 5.0 and m["se_sd"] <= 0.02, (tag, m)


def assert_st_chain(engine, case, tag, dtype=np.float32, tol=0.02):
    """A chain of CHAIN_SWEEPS sweeps on `engine` must visit the states with the enumerated frequencies (Monte-Carlo error ~0.01)
    and its effects must have the enumeration's first and second moments."""
    exact, Ea, Eaa = exact_mixture_moments(case["X"], case["y"], case["vare"], case["class_vars"], case["class_probs"])
    counts, alphas = run_st_chain(engine, case, dtype)
    tot = len(alphas)
    worst = max(abs(counts.get(s, 0) / tot - pr) for s, pr in exact.items())
    print(f"exact-posterior states {tag}: worst frequency difference {worst:.4f} (bound {tol})")
    assert worst < tol, (worst, sorted(((pr, counts.get(s, 0) / tot, s) for s, pr in exact.items()), reverse=True)[:6])
    for j in range(case["X"].shape[1]):                             # marginal inclusion probability of every marker
        ex = sum(pr for s, pr in exact.items() if s[j] != 0)
        got = sum(c for s, c in counts.items() if s[j] != 0) / tot
        assert abs(ex - got) < tol, (j, ex, got)
    assert_effect_moments(alphas, Ea, Eaa, tag)


def assert_mt_chain(engine, case, tag, dtype=np.float32, tol=0.025):
    exact, Ea, Eaa = exact_mixture_moments_mt(case["X"], case["Y"], case["R"], case["G"], case["prior"])
    counts, alphas = run_mt_chain(engine, case, dtype)
    tot = len(alphas)
    worst = max(abs(counts.get(s, 0) / tot - pr) for s, pr in exact.items())
    print(f"exact-posterior states {tag}: worst frequency difference {worst:.4f} (bound {tol})")
    assert worst < tol, (worst, sorted(((pr, counts.get(s, 0) / tot, s) for s, pr in exact.items()), reverse=True)[:6])
    assert_effect_moments(alphas, Ea, Eaa, tag)
