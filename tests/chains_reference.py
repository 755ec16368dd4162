"""TEST INFRASTRUCTURE: a numpy Float64 restatement of the BayesR sweep of the device's session (k_mega_sample_r, csrc/mega.hpp) on the
same Philox counters, the potential scale reduction factor of k_mega_psrf, and the stand-in engine of tests/mega_reference.py extended
with mega_sweep_r / mega_accumulate_r / mega_psrf.  The package never imports this file.

K chains of one model are K traits of the session (chain k draws with trait_id = first_trait + k).  Per chain vare, sigma2, gamma[4]
(gamma_1 = 0) and pi[4]; one marker, markers in order (BayesR.jl:56-96, all in double):
    rhs = (x_j'r + xpx_j alpha_j) / vare;  c = 2..4: v_c = gamma_c sigma2, lhs_c = xpx_j / vare + 1 / v_c, bHat_c = rhs / lhs_c,
    lp_c = 0.5 (log(1 / lhs_c) - log v_c + bHat_c rhs) + log pi_c;  lp_1 = log pi_1;  probs_c = exp(lp_c - (mx + log sum exp(lp - mx)))
    the class: cp = probs_1, while cp <= u the next class is added;  class 1: alpha = 0, else alpha = bHat_c + z sqrt(1 / lhs_c)
    delta = the class (1..4), beta = alpha;  r += x_j (alpha_old - alpha_new)
u and z are mega_reference's (slots 10 and 11).  sweep_r_plain is that chain marker by marker, sweep_r_blocked the exact block form
the device runs.  The operations of the law are written in the device's order (the library is built without FMA contraction); the
O(n) sums are numpy's, so the tests that compare the device with this file carry a rounding bound.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mega_reference as MR  # noqa: E402
from mega_reference import MegaStandInEngine, SweepResult, apply_changes, draws, gram_block  # noqa: E402,F401

U = MR.U
MIN_MARGIN = MR.MIN_MARGIN
DEFAULT_GAMMA = np.array([0.0, 0.01, 0.1, 1.0])
R_STAT_KEYS = ("class_counts", "ssq", "nnz", "alpha_ss", "resid_ss", "resid_sum", "n_changed")


def _par_r(T, vare, var_effect, gamma, pi):
    vare, sig = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (vare, var_effect)]
    out = []
    for a in (gamma, pi):
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (4,):
            a = np.repeat(a[:, None], T, axis=1)
        out.append(a)
    assert vare.shape == (T,) and sig.shape == (T,) and out[0].shape == (4, T) and out[1].shape == (4, T)
    return vare, sig, out[0], out[1]


def check_r_params(vare, sig, gamma, pi):
    """What jwas_hip_mega_sweep_r refuses."""
    ok = np.all(np.isfinite(vare) & (vare > 0)) and np.all(np.isfinite(sig) & (sig > 0)) and np.all(gamma[0] == 0.0)
    ok = ok and np.all(np.isfinite(gamma[1:]) & (gamma[1:] > 0)) and np.all((pi >= 0) & (pi <= 1)) and np.all(np.abs(pi.sum(axis=0) - 1.0) <= 1e-8)
    if not ok:
        raise ValueError("positive finite variances, gamma_1 = 0, positive finite gamma_2..4 and class probabilities that sum to 1 are needed")


def marker_law_r(xpx, s, alpha, vare, sig, gamma, pi, u, z):
    """One marker of every chain at once (arrays over the chains; gamma, pi: 4 x T): (class 1..4, alpha_new, probs [4 x T], margin)
    -- margin: the distance of u from the nearest of the three CDF boundaries."""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        ie = 1.0 / vare
        rhs = (s + xpx * alpha) * ie
        vc = gamma[1:] * sig[None, :]                                   # 3 x T
        lhs = xpx * ie + 1.0 / vc
        inv_lhs = 1.0 / lhs
        bh = rhs * inv_lhs
        lp = np.vstack([np.log(pi[0])[None, :], 0.5 * ((np.log(inv_lhs) - np.log(vc)) + bh * rhs) + np.log(pi[1:])])
        mx = lp.max(axis=0)
        e = np.exp(lp - mx)
        se = ((e[0] + e[1]) + e[2]) + e[3]
        probs = np.exp(lp - (mx + np.log(se)))
    T = probs.shape[1]
    cls, cp = np.zeros(T, dtype=np.int64), probs[0].copy()
    bounds = np.empty((3, T))
    for c in range(3):                                                   # the walk `while cp <= u`, all chains at once
        bounds[c] = cp
        step = (cls == c) & (cp <= u)
        cls = np.where(step, c + 1, cls)
        cp = cp + probs[c + 1]                                           # (only the chains that stepped read it again)
    # the boundary k of a chain is read only if the chain reached class k: a chain that stopped earlier never compares with it
    reached = np.arange(3)[:, None] <= cls[None, :]
    margin = np.where(reached, np.abs(u[None, :] - bounds), np.inf).min(axis=0)
    k = np.maximum(cls - 1, 0)
    a_new = np.where(cls == 0, 0.0, bh[k, np.arange(T)] + z * np.sqrt(inv_lhs[k, np.arange(T)]))
    return (cls + 1).astype(np.float64), a_new, probs, margin


def _finish_r(R, alpha, delta, alpha0, gamma, margins):
    T = alpha.shape[0]
    g = np.take_along_axis(gamma, (delta.astype(np.int64) - 1).T, axis=0).T if T else np.zeros_like(alpha)      # gamma of every marker's class, T x p
    inm = delta > 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ssq = np.where(inm, alpha * alpha / g, 0.0).sum(axis=1)
    return SweepResult(class_counts=np.stack([(delta == c + 1.0).sum(axis=1).astype(np.float64) for c in range(4)]), ssq=ssq,
                       nnz=inm.sum(axis=1).astype(np.float64), alpha_ss=(alpha * alpha).sum(axis=1), resid_ss=(R * R).sum(axis=1),
                       resid_sum=R.sum(axis=1), n_changed=(alpha != alpha0).sum(axis=1).astype(np.float64), step_ms=0.0, margins=margins)


def sweep_r_plain(X, R, alpha, beta, delta, *, iteration, seed, vare, var_effect, gamma, pi, first_trait=0, min_margin=0.0):
    """The BayesR chain marker by marker; R, alpha, beta, delta (T x .) are updated in place."""
    X = np.asarray(X, dtype=np.float64)
    T, p = alpha.shape
    vare, sig, gamma, pi = _par_r(T, vare, var_effect, gamma, pi)
    u, z = draws(p, T, iteration, seed, first_trait)
    alpha0, margins = alpha.copy(), np.empty((T, p))
    xpx = (X * X).sum(axis=0)
    for j in range(p):
        d_new, a_new, _, margins[:, j] = marker_law_r(xpx[j], R @ X[:, j], alpha[:, j], vare, sig, gamma, pi, u[:, j], z[:, j])
        R += (alpha[:, j] - a_new)[:, None] * X[:, j][None, :]
        alpha[:, j], beta[:, j], delta[:, j] = a_new, a_new, d_new
    assert margins.min() >= min_margin, f"a decision uniform lies within {min_margin} of a CDF boundary ({margins.min()})"
    return _finish_r(R, alpha, delta, alpha0, gamma, margins)


def sweep_r_blocked(X, R, alpha, beta, delta, *, block_size, iteration, seed, vare, var_effect, gamma, pi, first_trait=0, min_margin=0.0, grams=None):
    """The exact block form (mega_reference.sweep_blocked under the 4-class law); grams[k]: gram_block of block k."""
    X = np.asarray(X, dtype=np.float64)
    T, p = alpha.shape
    vare, sig, gamma, pi = _par_r(T, vare, var_effect, gamma, pi)
    u, z = draws(p, T, iteration, seed, first_trait)
    alpha0, margins = alpha.copy(), np.empty((T, p))
    for k, j0 in enumerate(range(0, p, block_size)):
        b = min(block_size, p - j0)
        Xb = X[:, j0:j0 + b]
        G = grams[k] if grams is not None else Xb.T @ Xb
        s = R @ Xb
        D = np.zeros((T, b))
        for a in range(b):
            j = j0 + a
            d_new, a_new, _, margins[:, j] = marker_law_r(G[a, a], s[:, a], alpha[:, j], vare, sig, gamma, pi, u[:, j], z[:, j])
            d = alpha[:, j] - a_new
            s = s + d[:, None] * G[a][None, :]
            D[:, a] = d
            alpha[:, j], beta[:, j], delta[:, j] = a_new, a_new, d_new
        apply_changes(R, Xb, D)
    assert margins.min() >= min_margin, f"a decision uniform lies within {min_margin} of a CDF boundary ({margins.min()})"
    return _finish_r(R, alpha, delta, alpha0, gamma, margins)


def conditional_recheck_r(X, R0, alpha0, alpha1, delta1, *, iteration, seed, vare, var_effect, gamma, first_trait=0):
    """mega_reference.conditional_recheck under the 4-class law: every marker's effect recomputed from the OTHER side's own history
    and under its class.  In class c > 1 the effect is the BayesC draw with the effect variance v_c = gamma_c sigma2 -- the same
    scalar solve, so mega_reference.marker_bound applies with v = v_c (its derivation does not use where v came from; gamma_c sigma2
    is one product of the same two doubles on both sides).  In class 1 both sides hold exactly 0: the bound is 0 and the values
    must be equal.  Returns (alpha [T x p], bound [T x p])."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    T = R0.shape[0]
    vare, sig, gamma, _ = _par_r(T, vare, var_effect, gamma, np.full(4, 0.25))
    Xa = np.abs(X)
    G, Ga = np.tril(X.T @ X, -1), np.tril(Xa.T @ Xa, -1)
    xpx = (X * X).sum(axis=0)
    d = alpha0 - alpha1
    S = R0 @ X + d @ G.T
    Sa = np.abs(R0) @ Xa + np.abs(d) @ Ga.T + xpx[None, :] * np.abs(alpha0)
    out, bound = np.zeros((T, p)), np.zeros((T, p))
    for k in range(T):
        z = MR.mega_normal(np.arange(p), iteration, seed, first_trait + k)
        xw = S[k] + xpx * alpha0[k]
        ie = 1.0 / vare[k]
        dxw = 2 * (n + p + 3) * U * Sa[k]
        for j in range(p):
            c = int(delta1[k, j]) - 1
            if c == 0:
                continue
            vc = gamma[c, k] * sig[k]
            inv_lhs = 1.0 / (xpx[j] * ie + 1.0 / vc)
            out[k, j] = (xw[j] * ie) * inv_lhs + z[j] * np.sqrt(inv_lhs)
            bound[k, j] = MR.marker_bound(xpx[j], xw[j], dxw[j], n, vare[k], vc, 1.0, z[j])
    return out, bound


# ---- the potential scale reduction factor -------------------------------------------------------------------------------------------------
def psrf_from_moments(m, q, N):
    """k_mega_psrf in numpy: m, q [K x p] the running means and means of squares after N samples; NaN where W == 0."""
    K = m.shape[0]
    W = (N / (N - 1.0) * (q - m * m)).sum(axis=0) / K
    BN = ((m - m.sum(axis=0) / K) ** 2).sum(axis=0) / (K - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(W == 0.0, np.nan, np.sqrt(((N - 1.0) / N * W + BN) / W))


def psrf_bound(m, q, N):
    """A bound on |R_device - psrf_from_moments| per marker; both sides read the same doubles m_k, q_k and evaluate the same formula
    in double, in another order of the K-term sums at most.  u = 2^-53.
      q_k - m_k^2     the product m_k^2 and the difference round once each: <= u (m_k^2 + |q_k - m_k^2|) <= 2 u q_k' with
                      q_k' = max(q_k, m_k^2) -- an ABSOLUTE error: the difference itself may be far smaller (the cancellation)
      W               dW <= sum_k 2 u q_k' f / K + (K + 3) u |W|  (f = N / (N - 1); the scaling, the K-term sum and the division)
      B / N           every term is a square of a rounded difference: relative (K + 6) u of the sum (the mean, the difference,
                      the square, the sum, the division), dB <= (K + 6) u B/N + 4 u max|m| sqrt(B/N K) for the mean's own rounding
      V, V / W, sqrt  dV <= g dW + dB + 3 u V;  d(V / W) <= (dV + (V / W) dW) / (|W| - dW) + u V / W;  the square root halves the
                      relative error and adds u.
    The bound is doubled (first-order terms only); where |W| <= 2 dW the ratio is not determined and the bound is infinite."""
    K = m.shape[0]
    f, g = N / (N - 1.0), (N - 1.0) / N
    W = (f * (q - m * m)).sum(axis=0) / K
    BN = ((m - m.sum(axis=0) / K) ** 2).sum(axis=0) / (K - 1)
    V = g * W + BN
    dW = (2 * U * np.maximum(q, m * m) * f).sum(axis=0) / K + (K + 3) * U * np.abs(W)
    dB = (K + 6) * U * BN + 4 * U * np.abs(m).max(axis=0) * np.sqrt(BN * K)
    dV = g * dW + dB + 3 * U * np.abs(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = V / W
        dr = (dV + np.abs(ratio) * dW) / (np.abs(W) - dW) + U * np.abs(ratio)
        rhat = np.sqrt(ratio)
        out = 2 * (0.5 * dr / rhat + U * rhat)
    return np.where(np.abs(W) <= 2 * dW, np.inf, out)


def psrf_from_samples(x):
    """The same statistic from the saved samples themselves, x [K x N] (or [K x N x q]): the host's rows of PSRF.txt."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    m, q = x.mean(axis=1), (x * x).mean(axis=1)
    return psrf_from_moments(m.reshape(x.shape[0], -1), q.reshape(x.shape[0], -1), float(N))


# ---- the stand-in engine -----------------------------------------------------------------------------------------------------------------
class ChainsStandInEngine(MegaStandInEngine):
    """MegaStandInEngine with the methods of HipEngine that the chains driver adds."""

    def mega_sweep_r(self, *, iteration, seed, vare, var_effect, gamma, pi, min_margin=0.0):
        s = self._need()
        self.calls.append("mega_sweep_r")
        vare, sig, gamma, pi = _par_r(s.T, vare, var_effect, gamma, pi)
        if int(iteration) < 1:
            raise ValueError("iteration >= 1 is needed")
        check_r_params(vare, sig, gamma, pi)
        return sweep_r_blocked(self.X, s.R, s.alpha, s.beta, s.delta, block_size=s.bs, iteration=iteration, seed=seed, vare=vare, var_effect=sig,
                               gamma=gamma, pi=pi, first_trait=s.first, min_margin=min_margin, grams=s.grams)

    def mega_accumulate_r(self, nsamples):
        s = self._need()
        for acc, v in zip(s.acc, (s.alpha, s.alpha * s.alpha, (s.delta > 1.0).astype(np.float64))):
            acc += (v - acc) / nsamples

    def mega_psrf(self, nsamples):
        s = self._need()
        if s.T < 2 or not float(nsamples) >= 2.0:
            raise ValueError("at least 2 chains and 2 samples are needed")
        return psrf_from_moments(s.acc[0], s.acc[1], float(nsamples))


# ---- fixed inputs shared by tests/test_chains_host.py and tests/test_gpu_chains.py -------------------------------------------------------
PI_R_CYCLE = ((0.95, 0.03, 0.015, 0.005), (0.5, 0.2, 0.2, 0.1), (0.0, 0.5, 0.3, 0.2), (0.6, 0.0, 0.3, 0.1))
GAMMA_CYCLE = ((0.0, 0.01, 0.1, 1.0), (0.0, 0.001, 0.05, 2.0))


def make_case_r(n=301, p=100, seed=7):
    """mega_reference.make_case (genotypes, residuals, starting effects, vare for 64 chains) with the BayesR parameters of every chain:
    sigma2 = 20 v, pi from PI_R_CYCLE (one with an empty null class, one with an empty class 2), gamma from GAMMA_CYCLE."""
    cs = MR.make_case(n, p, seed)
    T = MR.MAX_TRAITS
    cs["sig"] = 20.0 * cs.v
    cs["pi_r"] = np.array([PI_R_CYCLE[k % 4] for k in range(T)]).T.copy()
    cs["gamma"] = np.array([GAMMA_CYCLE[(k // 4) % 2] for k in range(T)]).T.copy()
    return cs


def case_chains(cs, T, first=0):
    sl = slice(first, first + T)
    return SweepResult(n=cs.n, p=cs.p, X=cs.X, R=cs.R[sl].copy(), alpha=cs.alpha[sl].copy(), beta=cs.alpha[sl].copy(), delta=np.ones((T, cs.p)),
                       vare=cs.vare[sl].copy(), sig=cs.sig[sl].copy(), pi=cs.pi_r[:, sl].copy(), gamma=cs.gamma[:, sl].copy())


def reference_sweeps_r(cs, T, seed, block_size, iterations=(1, 2)):
    """The restatement's own consecutive sweeps of the first T chains from the case's state; asserts the margin of every decision.
    Returns one SweepResult per iteration with the state after it (and R0, alpha0: the state before it)."""
    c = case_chains(cs, T)
    out = []
    for it in iterations:
        R0, a0 = c.R.copy(), c.alpha.copy()
        r = sweep_r_blocked(c.X, c.R, c.alpha, c.beta, c.delta, block_size=block_size, iteration=it, seed=seed, vare=c.vare, var_effect=c.sig,
                            gamma=c.gamma, pi=c.pi, min_margin=MIN_MARGIN)
        r.update(R=c.R.copy(), alpha=c.alpha.copy(), delta=c.delta.copy(), R0=R0, alpha0=a0)
        out.append(r)
    return out


# ---- the exact-conditional case: one marker, three chains --------------------------------------------------------------------------------
CONDITIONAL_STEPS = 4000
CONDITIONAL_SEED = 29
MIN_EXPECTED = 200


def conditional_case_r():
    """mega_reference.conditional_case for BayesR: n = 83, one marker, three chains.  x'r + xpx alpha does not depend on the marker's
    current effect, so with fixed hyper-parameters every sweep draws (class, effect) from the same closed-form posterior,
    independently from step to step.  pi and gamma are chosen so that every class of every chain has an expected count of at
    least MIN_EXPECTED in CONDITIONAL_STEPS draws (conditional_posterior_r; the tests check it)."""
    base = MR.conditional_case()
    return SweepResult(n=base.n, T=base.T, X=base.X, e=base.e, vare=base.vare, sig=np.array([0.05, 0.04, 0.06]),
                       gamma=np.array([[0.0, 0.0, 0.0], [0.05, 0.1, 0.08], [0.3, 0.4, 0.35], [1.0, 1.0, 1.0]]),
                       pi=np.array([[0.25, 0.4, 0.3], [0.25, 0.2, 0.3], [0.25, 0.2, 0.2], [0.25, 0.2, 0.2]]))


def conditional_posterior_r(case):
    """Per chain (probs [4 x T], mean [3 x T], variance [3 x T] of the effect in the classes 2..4), in closed form."""
    xpx = float((case.X[:, 0] ** 2).sum())
    s = case.e @ case.X[:, 0]
    vc = case.gamma[1:] * case.sig[None, :]
    lhs = xpx / case.vare[None, :] + 1.0 / vc
    rhs = s / case.vare
    mu = rhs[None, :] / lhs
    lp = np.vstack([np.log(case.pi[0])[None, :], 0.5 * (-np.log(lhs) - np.log(vc) + mu * rhs[None, :]) + np.log(case.pi[1:])])
    pr = np.exp(lp - lp.max(axis=0))
    return pr / pr.sum(axis=0), mu, 1.0 / lhs


def conditional_engine_r(engine, case):
    engine.load_dense(case.X.astype(engine.dtype))
    engine.mega_begin(case.T, 64, 0)
    engine.mega_set_residual(case.e)                                     # alpha = 0: r = e
    return engine


def conditional_check_r(engine, case, seed=CONDITIONAL_SEED, steps=CONDITIONAL_STEPS):
    """Run `steps` BayesR sweeps; returns rows (chain, class, expected count, z of the class frequency, z of the mean and of the variance
    of the effect in the class -- 0 for class 1, whose effect must be exactly 0).  Every z must be <= 5."""
    probs, mu, var = conditional_posterior_r(case)
    T = case.T
    classes, effects = np.empty((steps, T)), np.empty((steps, T))
    for it in range(1, steps + 1):
        engine.mega_sweep_r(iteration=it, seed=seed, vare=case.vare, var_effect=case.sig, gamma=case.gamma, pi=case.pi)
        a, _, d = engine.mega_get_state()
        classes[it - 1], effects[it - 1] = d[:, 0], a[:, 0]
    rows = []
    for k in range(T):
        for c in range(4):
            sel = classes[:, k] == c + 1.0
            nc, pc = int(sel.sum()), probs[c, k]
            zf = abs(nc / steps - pc) / np.sqrt(pc * (1 - pc) / steps)
            if c == 0:
                assert np.all(effects[sel, k] == 0.0)
                rows.append((k, 1, pc * steps, zf, 0.0, 0.0))
                continue
            a = effects[sel, k]
            rows.append((k, c + 1, pc * steps, zf, abs(a.mean() - mu[c - 1, k]) / np.sqrt(var[c - 1, k] / nc),
                         abs(a.var(ddof=1) - var[c - 1, k]) / (var[c - 1, k] * np.sqrt(2.0 / (nc - 1)))))
    return rows
