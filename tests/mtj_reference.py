"""TEST INFRASTRUCTURE: a numpy Float64 restatement of the device's joint multi-trait sweep (csrc/mtjoint.hpp) on the same Philox counters,
and a stand-in engine with the mtj_* methods of HipEngine.  The package never imports this file.

Gibbs sampler I (_MTBayesABC_samplerI!, markers/BayesianAlphabet/MTBayesABC.jl:75-126).  n individuals, t traits, R the t x n residual,
Rinv = inv(vare), Ginv = inv(G) (t x t), log_pi over the 2^t joint states (state = sum_k delta_k << k, -inf: probability 0).  Marker j with
s_k = x_j'r_k at the marker's entry, xx = x_j'x_j and its current (alpha, beta, delta):  w_k = s_k + xx alpha_k (not refreshed below); then
for k = 0 .. t-1 in order, with beta and delta of the other traits as they stand:
    Ginv11 = Ginv[k,k],  C11 = Ginv11 + Rinv[k,k] xx,  invLhs0 = 1 / Ginv11,  invLhs1 = 1 / C11
    q0 = sum_{l != k} Ginv[k,l] beta_l,  gHat0 = (-q0) invLhs0
    wr = sum_l w_l Rinv[l,k],  q1 = sum_{l != k} (delta_l ? Ginv[k,l] + xx Rinv[k,l] : Ginv[k,l]) beta_l,  gHat1 = (wr - q1) invLhs1
    logDelta0 = -0.5 (log Ginv11 - gHat0^2 Ginv11) + log_pi[d0],  logDelta1 = -0.5 (log C11 - gHat1^2 C11) + log_pi[d1]
    probDelta1 = 1 / (1 + exp(logDelta0 - logDelta1))   (log_pi[d1] = -inf: 0)
    u_k < probDelta1: delta_k = 1, beta_k = alpha_k = gHat1 + z_k sqrt(invLhs1);  else delta_k = 0, alpha_k = 0, beta_k = gHat0 + z_k sqrt(invLhs0)
then r_k += x_j (alpha_k,old - alpha_k,new) for every k.  Every sum above runs over l ascending, one product after the other: the
device's order, so the chain of one marker is the same IEEE operations on both sides; what differs is the order of the O(n) sums
behind s and xx and the libm behind log, exp and Box-Muller.
u_k = u52 of words (1, 0) of philox(marker, iteration, 0x05000000 | k, 14); z_k Box-Muller of philox(marker, iteration, 0x05000000 | k, 15).
sweep_plain is that chain marker by marker; sweep_blocked is the exact block form the device runs (mega_reference.sweep_blocked's)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from liability_reference import philox4x32_10  # noqa: E402
from mega_reference import BlockStandInEngine, SweepResult, apply_changes, gram_block  # noqa: E402,F401

MTJ_TAG, SLOT_U, SLOT_Z = 0x05000000, 14, 15
MIN_TRAITS, MAX_TRAITS, MAX_BLOCK = 5, 8, 256
TWO_PI = 6.283185307179586476925286766559
U = 2.0 ** -53
MIN_MARGIN = 1e-9


def _u52(lo, hi):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def _words(index, iteration, trait, slot, seed):
    seed = int(seed)
    return philox4x32_10(np.asarray(index, dtype=np.uint64), np.uint64(iteration), np.uint64(MTJ_TAG | int(trait)), np.uint64(slot),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def draws(p, t, iteration, seed):
    """(u [t, p], z [t, p]) of one sweep."""
    j = np.arange(p)
    u, z = np.empty((t, p)), np.empty((t, p))
    for k in range(t):
        w0, w1, _, _ = _words(j, iteration, k, SLOT_U, seed)
        u[k] = _u52(w0, w1)
        w0, w1, w2, w3 = _words(j, iteration, k, SLOT_Z, seed)
        z[k] = np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(TWO_PI * _u52(w2, w3))
    return u, z


def inv_small(A):
    """Gauss-Jordan with partial pivoting in the operation order of csrc/ctx.hpp's inv_small."""
    A = np.asarray(A, dtype=np.float64)
    t = A.shape[0]
    M = np.hstack([A.copy(), np.eye(t)])
    for c in range(t):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        assert M[piv, c] != 0.0
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for i in range(t):
            if i != c and M[i, c] != 0.0:
                M[i] = M[i] - M[i, c] * M[c]
    return M[:, t:].copy()


def log_table(pi):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(pi, dtype=np.float64))


def state_of(delta_col):
    return int(sum(1 << k for k in range(len(delta_col)) if delta_col[k] != 0.0))


def marker_chain(xx, s, alpha, beta, state, Rinv, Ginv, log_pi, u, z, force=None, dw=None, dxx=0.0):
    """The t-step chain of one marker.  Returns (alpha_new [t], beta_new [t], state_new, prob [t]) and, when dw (a bound on the error of every
    w_k) is given, also err [t]: a bound on the error of beta_new of a second evaluation that takes the same decisions.
    force: a state whose bits replace the decisions (the recheck of another side's chain).
    THE BOUND, u = 2^-53, first order and doubled at the end for the higher-order terms.  A sum of m products in the same order on both
    sides from inputs that differ: sum |coefficient| |input error| + (m + 2) u sum |product|.  xx differs by dxx (two summation orders
    of n squares), so C11 by dC = |Rinv[k,k]| dxx + 2 u C11 and a coefficient Ginv[k,l] + xx Rinv[k,l] by |Rinv[k,l]| dxx + 2 u |.|.
      gHat1 = (wr - q1) / C11:  (d wr + d q1) / C11 + |gHat1| (dC / C11 + 4 u);   gHat0 = -q0 / Ginv11:  d q0 / Ginv11 + 4 u |gHat0|
      z sqrt(1 / C11): |z| sd (dC / C11 + 4 u) + 2^-46 sd for Box-Muller (mega_reference.marker_bound's argument);  + 2 u |beta|
    and the error of beta_k enters q0 and q1 of the later traits of the marker through their coefficients."""
    t = len(s)
    w = [s[k] + xx * alpha[k] for k in range(t)]
    bn = [float(b) for b in beta]
    an = [0.0] * t
    prob = [0.0] * t
    err = [0.0] * t                      # of bn: the traits not yet visited carry the same doubles on both sides
    dn = int(state)
    for k in range(t):
        G11 = Ginv[k, k]
        C11 = G11 + Rinv[k, k] * xx
        invC, invG = 1.0 / C11, 1.0 / G11
        q0 = q1 = wr = 0.0
        dq0 = dq1 = dwr = a0 = a1 = aw = 0.0
        for l in range(t):
            pw = w[l] * Rinv[l, k]
            wr = wr + pw
            if dw is not None:
                dwr += abs(Rinv[l, k]) * dw[l]
                aw += abs(pw)
            if l != k:
                g = Ginv[k, l]
                inc_l = (dn >> l) & 1
                c = g + xx * Rinv[k, l] if inc_l else g
                q0 = q0 + g * bn[l]
                q1 = q1 + c * bn[l]
                if dw is not None:
                    dq0 += abs(g) * err[l]
                    dq1 += abs(c) * err[l] + ((abs(Rinv[k, l]) * dxx + 2 * U * abs(c)) * abs(bn[l]) if inc_l else 0.0)
                    a0 += abs(g * bn[l])
                    a1 += abs(c * bn[l])
        gHat0 = (-q0) * invG
        gHat1 = (wr - q1) * invC
        d0, d1 = dn & ~(1 << k), dn | (1 << k)
        with np.errstate(over="ignore", invalid="ignore"):
            ld0 = -0.5 * (np.log(G11) - gHat0 * gHat0 * G11) + log_pi[d0]
            ld1 = -0.5 * (np.log(C11) - gHat1 * gHat1 * C11) + log_pi[d1]
            prob[k] = 0.0 if log_pi[d1] == -np.inf else float(1.0 / (1.0 + np.exp(ld0 - ld1)))
        inc = bool((force >> k) & 1) if force is not None else bool(u[k] < prob[k])
        if inc:
            sd = np.sqrt(invC)
            bn[k] = gHat1 + z[k] * sd
            an[k] = bn[k]
            dn = d1
            if dw is not None:
                dC = abs(Rinv[k, k]) * dxx + 2 * U * C11
                dg = (dwr + (t + 2) * U * aw + dq1 + (t + 2) * U * a1) * invC + abs(gHat1) * (dC * invC + 4 * U)
                err[k] = 2 * (dg + abs(z[k]) * sd * (dC * invC + 4 * U) + 2.0 ** -46 * sd + 2 * U * abs(bn[k]))
        else:
            sd = np.sqrt(invG)
            bn[k] = gHat0 + z[k] * sd
            an[k] = 0.0
            dn = d0
            if dw is not None:
                dg = (dq0 + (t + 2) * U * a0) * invG + 4 * U * abs(gHat0)
                err[k] = 2 * (dg + abs(z[k]) * sd * 4 * U + 2.0 ** -46 * sd + 2 * U * abs(bn[k]))
    out = (np.array(an), np.array(bn), dn, np.array(prob))
    return out + (np.array(err),) if dw is not None else out


def _finish(R, alpha, beta, delta, alpha0, margins, probs):
    t, p = alpha.shape
    states = np.array([state_of(delta[:, j]) for j in range(p)])
    return SweepResult(state_counts=np.bincount(states, minlength=1 << t).astype(np.float64), beta_ss=beta @ beta.T, alpha_ss=(alpha * alpha).sum(axis=1),
                       resid_cp=R @ R.T, resid_sum=R.sum(axis=1), n_changed=float((alpha != alpha0).any(axis=0).sum()), step_ms=0.0,
                       margins=margins, probs=probs, states=states)


def sweep_plain(X, R, alpha, beta, delta, *, iteration, seed, Rinv, Ginv, log_pi, min_margin=0.0):
    """The chain marker by marker; R, alpha, beta, delta (t x .) are updated in place."""
    X = np.asarray(X, dtype=np.float64)
    t, p = alpha.shape
    u, z = draws(p, t, iteration, seed)
    alpha0, margins, probs = alpha.copy(), np.empty((t, p)), np.empty((t, p))
    xpx = (X * X).sum(axis=0)
    for j in range(p):
        an, bn, dn, prob = marker_chain(xpx[j], R @ X[:, j], alpha[:, j], beta[:, j], state_of(delta[:, j]), Rinv, Ginv, log_pi, u[:, j], z[:, j])
        R += (alpha[:, j] - an)[:, None] * X[:, j][None, :]
        alpha[:, j], beta[:, j], delta[:, j] = an, bn, [(dn >> k) & 1 for k in range(t)]
        margins[:, j], probs[:, j] = np.abs(u[:, j] - prob), prob
    assert margins.min() >= min_margin, f"a decision uniform lies within {min_margin} of probDelta1 ({margins.min()})"
    return _finish(R, alpha, beta, delta, alpha0, margins, probs)


def sweep_blocked(X, R, alpha, beta, delta, *, block_size, iteration, seed, Rinv, Ginv, log_pi, min_margin=0.0, grams=None):
    """The exact block form; grams[k]: gram_block of block k (formed here when None)."""
    X = np.asarray(X, dtype=np.float64)
    t, p = alpha.shape
    u, z = draws(p, t, iteration, seed)
    alpha0, margins, probs = alpha.copy(), np.empty((t, p)), np.empty((t, p))
    for k, j0 in enumerate(range(0, p, block_size)):
        b = min(block_size, p - j0)
        Xb = X[:, j0:j0 + b]
        G = grams[k] if grams is not None else Xb.T @ Xb
        s = R @ Xb                                                       # t x b
        D = np.zeros((t, b))
        for a in range(b):
            j = j0 + a
            an, bn, dn, prob = marker_chain(G[a, a], s[:, a], alpha[:, j], beta[:, j], state_of(delta[:, j]), Rinv, Ginv, log_pi, u[:, j], z[:, j])
            d = alpha[:, j] - an
            s = s + d[:, None] * G[a][None, :]
            D[:, a] = d
            alpha[:, j], beta[:, j], delta[:, j] = an, bn, [(dn >> q) & 1 for q in range(t)]
            margins[:, j], probs[:, j] = np.abs(u[:, j] - prob), prob
        apply_changes(R, Xb, D)
    assert margins.min() >= min_margin, f"a decision uniform lies within {min_margin} of probDelta1 ({margins.min()})"
    return _finish(R, alpha, beta, delta, alpha0, margins, probs)


def _history(X, R0, alpha0, alpha1):
    """What conditional_recheck and propagated_bound share: with d_i = alpha0_i - alpha1_i the changes made to the markers before j, the
    chain's s_j = x_j'r0 + sum_{i<j} G_ji d_i whatever the blocks, and abs_s_j the sum of the absolute terms (xx |alpha0_j| included)."""
    X = np.asarray(X, dtype=np.float64)
    Xa = np.abs(X)
    G, Ga = np.tril(X.T @ X, -1), np.tril(Xa.T @ Xa, -1)                 # [j, i], i < j
    xpx = (X * X).sum(axis=0)
    d = alpha0 - alpha1
    S = R0 @ X + d @ G.T
    Sa = np.abs(R0) @ Xa + np.abs(d) @ Ga.T + xpx[None, :] * np.abs(alpha0)
    return X, Ga, xpx, S, Sa


def marker_bound(n, p, xx, abs_s, alpha0, carried=0.0):
    """(dw [t], dxx) of one marker: w_k = s_k + xx alpha_k from sums of at most N = n + p + 1 products in two orders, 2 (N + 2) u abs_s_k, plus
    what earlier markers' differences carry into s_k, plus the two orders of xx (2 (n + 2) u xx) times |alpha_k|."""
    dxx = 2 * (n + 2) * U * xx
    return 2 * (n + p + 3) * U * abs_s + carried + dxx * np.abs(alpha0), dxx


def conditional_recheck(X, R0, alpha0, beta0, delta0, alpha1, delta1, *, iteration, seed, Rinv, Ginv, log_pi):
    """Every marker's chain recomputed from the OTHER side's own history and under ITS indicators delta1: (beta [t x p], bound [t x p]).  The
    inputs of marker j are the same doubles on both sides, so only the order of the sums behind s and xx differs (marker_bound), carried
    through the t-step conditional by marker_chain."""
    X, Ga, xpx, S, Sa = _history(X, R0, alpha0, alpha1)
    n, p = X.shape
    t = R0.shape[0]
    u, z = draws(p, t, iteration, seed)
    beta, bound = np.empty((t, p)), np.empty((t, p))
    for j in range(p):
        dw, dxx = marker_bound(n, p, xpx[j], Sa[:, j], alpha0[:, j])
        _, bn, _, _, err = marker_chain(xpx[j], S[:, j], alpha0[:, j], beta0[:, j], state_of(delta0[:, j]), Rinv, Ginv, log_pi, u[:, j], z[:, j],
                                        force=state_of(delta1[:, j]), dw=dw, dxx=dxx)
        beta[:, j], bound[:, j] = bn, err
    return beta, bound


def propagated_bound(X, R0, alpha0, beta0, delta0, res, *, iteration, seed, Rinv, Ginv, log_pi):
    """Bounds on what a device that runs the chain of `res` (a sweep of this file from R0, alpha0, beta0, delta0) in another summation order
    and block size may differ by when both choose the same indicators: err_beta [t x p].  An earlier marker's difference reaches marker j
    through the Gram (inside a block) or through the residual (across blocks): to first order both are Gabs_ji err_d_i, with err_d_i =
    delta_i err_beta_i.  Meaningful under a tight prior only."""
    X, Ga, xpx, S, Sa = _history(X, R0, alpha0, res.alpha)
    n, p = X.shape
    t = R0.shape[0]
    u, z = draws(p, t, iteration, seed)
    err, err_d = np.zeros((t, p)), np.zeros((t, p))
    for j in range(p):
        dw, dxx = marker_bound(n, p, xpx[j], Sa[:, j], alpha0[:, j], carried=err_d[:, :j] @ Ga[j, :j])
        e = marker_chain(xpx[j], S[:, j], alpha0[:, j], beta0[:, j], state_of(delta0[:, j]), Rinv, Ginv, log_pi, u[:, j], z[:, j],
                         force=state_of(res.delta[:, j]), dw=dw, dxx=dxx)[4]
        err[:, j], err_d[:, j] = e, e * res.delta[:, j]
    return err


class MtjStandInEngine(BlockStandInEngine):
    """The mtj_* methods of HipEngine (and the little else the joint driver calls) on the restatement above."""
    KIND = "mtj"
    mtj_set_residual, mtj_get_residual = BlockStandInEngine._set_residual, BlockStandInEngine._get_residual
    mtj_set_state, mtj_get_state = BlockStandInEngine._set_state, BlockStandInEngine._get_state
    mtj_accumulate, mtj_posterior = BlockStandInEngine._accumulate, BlockStandInEngine._posterior
    mtj_mul_alpha, mtj_gram, mtj_end = BlockStandInEngine._mul_alpha, BlockStandInEngine._gram, BlockStandInEngine._finish

    def mtj_begin(self, ntraits, block_size=64):
        if self.p == 0:
            raise ValueError("no genotype matrix loaded")
        if not MIN_TRAITS <= int(ntraits) <= MAX_TRAITS or not 0 <= int(block_size) <= MAX_BLOCK:
            raise ValueError("the number of traits must be in [5,8] and the block size in [1,256]")
        self._open(int(ntraits), int(block_size) or 64)

    def mtj_sweep(self, *, iteration, seed, rinv, ginv, log_pi, min_margin=0.0):
        s = self._need()
        self.calls.append("mtj_sweep")
        rinv, ginv, lp = np.asarray(rinv, dtype=np.float64), np.asarray(ginv, dtype=np.float64), np.asarray(log_pi, dtype=np.float64).reshape(-1)
        if int(iteration) < 1 or rinv.shape != (s.T, s.T) or ginv.shape != (s.T, s.T) or lp.size != 1 << s.T or np.any(np.isnan(lp)) or np.any(lp > 0):
            raise ValueError("iteration >= 1, T x T inverses and 2^T log probabilities are needed")
        for M in (rinv, ginv):
            if not np.all(np.isfinite(M)) or np.any(np.linalg.eigvalsh((M + M.T) / 2) <= 0):
                raise ValueError("rinv and ginv must be finite and positive definite")
        return sweep_blocked(self.X, s.R, s.alpha, s.beta, s.delta, block_size=s.bs, iteration=iteration, seed=seed, Rinv=rinv, Ginv=ginv, log_pi=lp,
                             min_margin=min_margin, grams=s.grams)


# ---- fixed inputs shared by tests/test_mtj_host.py and tests/test_gpu_mtj.py ----------------------------------------------------------------
CASE_SEED = 5                            # the Philox seed of the GPU tests: find_seed(make_case()) returns it (asserted in test_mtj_host.py)


def _spd(rng, t, scale, corr):
    """A t x t covariance with variances around `scale` and correlations up to about `corr`; its leading blocks are covariances too."""
    L = np.eye(t) + corr * np.tril(rng.uniform(-1, 1, (t, t)), -1)
    sd = np.sqrt(scale * rng.uniform(0.6, 1.4, t))
    C = L @ L.T
    C = C / np.sqrt(np.outer(np.diag(C), np.diag(C)))
    return C * np.outer(sd, sd)


def make_case(n=301, p=100, seed=7):
    """Genotypes as mega_reference.make_case (centred counts rounded to Float32) and, for 8 traits at once, a residual, a starting state,
    full covariances vare and G and, per number of traits t in 5 .. 8, a Pi table with every joint state possible (half the mass on the
    all-zero state).  A t-trait test takes rows 0 .. t-1 and the leading t x t blocks."""
    rng = np.random.default_rng(seed)
    T = MAX_TRAITS
    freq = rng.uniform(0.1, 0.9, p)
    X = (rng.binomial(2, freq, size=(n, p)) - 2.0 * freq).astype(np.float32).astype(np.float64)
    R = rng.standard_normal((T, n))
    delta = (rng.random((T, p)) < 0.4).astype(np.float64)
    beta = 0.05 * rng.standard_normal((T, p))
    alpha = delta * beta
    vare = _spd(rng, T, 1.0, 0.5)
    G = _spd(rng, T, 0.005, 0.5)
    pi = {}
    for t in range(MIN_TRAITS, MAX_TRAITS + 1):
        tab = rng.dirichlet(np.ones(1 << t))
        tab[0] += 1.0
        pi[t] = tab / tab.sum()
    return SweepResult(n=n, p=p, X=X, R=R, alpha=alpha, beta=beta, delta=delta, vare=vare, G=G, pi=pi)


def case_traits(cs, t, pi=None, gscale=1.0):
    """The first t traits of a case: its state, Rinv, Ginv (Gauss-Jordan) and log pi."""
    pi = cs.pi[t] if pi is None else np.asarray(pi, dtype=np.float64)
    return SweepResult(n=cs.n, p=cs.p, t=t, X=cs.X, R=cs.R[:t].copy(), alpha=cs.alpha[:t].copy(), beta=cs.beta[:t].copy(), delta=cs.delta[:t].copy(),
                       Rinv=inv_small(cs.vare[:t, :t]), Ginv=inv_small(cs.G[:t, :t] * gscale), pi=pi, log_pi=log_table(pi))


def reference_sweep(c, iteration, seed, block_size, min_margin=MIN_MARGIN):
    """The restatement's own sweep from the state of c (a case_traits); asserts the margin of every decision uniform."""
    R, a, b, d = c.R.copy(), c.alpha.copy(), c.beta.copy(), c.delta.copy()
    r = sweep_blocked(c.X, R, a, b, d, block_size=block_size, iteration=iteration, seed=seed, Rinv=c.Rinv, Ginv=c.Ginv, log_pi=c.log_pi,
                      min_margin=min_margin)
    r.update(R=R, alpha=a, beta=b, delta=d)
    return r


def find_seed(cs, first=CASE_SEED, tries=50):
    """The first Philox seed from `first` on with which EVERY decision of iterations 1 and 2 (t = 5 and 8, blocks of 40, from the case's
    state) keeps |u - probDelta1| >= MIN_MARGIN in the restatement."""
    for seed in range(first, first + tries):
        ok = True
        for t in (MIN_TRAITS, MAX_TRAITS):
            c = case_traits(cs, t)
            for it in (1, 2):
                ok = ok and reference_sweep(c, it, seed, 40, min_margin=0.0).margins.min() >= MIN_MARGIN
        if ok:
            return seed
    raise AssertionError("no seed keeps every decision away from its threshold")


GPU_BLOCK, GPU_BLOCK_SIZES, GPU_TIGHT = 40, (1, 40, 100, 256), 0.01      # tests/test_gpu_mtj.py: its blocks, and G / 100 as the tight prior


def duplicate_case(cs, t, j1=3, j2=17):
    """A sparse Pi (0.95 on the all-zero state) and two duplicated causal columns j1 < j2 of one 64-lane sub-block: the residual carries a
    strong signal along x_j1 in every trait and the state starts empty, so marker j1 enters the model and its commit takes the signal
    away from marker j2.  Returns (case, (j1, j2))."""
    rng = np.random.default_rng(31)
    X = cs.X.copy()
    X[:, j2] = X[:, j1]
    pi = np.full(1 << t, 0.05 / ((1 << t) - 1))
    pi[0] = 0.95
    c = case_traits(cs, t, pi=pi)
    c.update(X=X, R=0.5 * rng.standard_normal((t, cs.n)) + np.linspace(0.6, 1.0, t)[:, None] * X[:, j1][None, :], alpha=np.zeros((t, cs.p)),
             beta=np.zeros((t, cs.p)), delta=np.zeros((t, cs.p)))
    return c, (j1, j2)


def speculative_state(c, j, iteration, seed):
    """The joint state marker j would take from the residual at block entry, with no commit of an earlier marker of its block: what a lane
    of the device's speculative walk evaluates first."""
    u, z = draws(c.p, c.t, iteration, seed)
    x = c.X[:, j]
    return marker_chain(float(x @ x), c.R @ x, c.alpha[:, j], c.beta[:, j], state_of(c.delta[:, j]), c.Rinv, c.Ginv, c.log_pi, u[:, j], z[:, j])[2]


def rrblup_case(cs, t):
    """All mass on the all-ones state (RR-BLUP), every marker in it from the start, as a session begins (sampler I moves one trait at a
    time: it cannot reach the only possible state from another one): every marker commits.  Returns (case, None)."""
    pi = np.zeros(1 << t)
    pi[-1] = 1.0
    c = case_traits(cs, t, pi=pi)
    c.delta[...] = 1.0
    c.alpha[...] = c.beta
    return c, None


def zero_state_case(cs, t):
    """A Pi with probability 0 on every state that has trait 0 in the model and trait 1 out of it, and on the all-ones state; the starting
    state holds no marker in such a state.  Returns (case, the states of probability 0)."""
    zero = np.array([s for s in range(1 << t) if ((s & 1) and not (s & 2)) or s == (1 << t) - 1])
    pi = cs.pi[t].copy()
    pi[zero] = 0.0
    c = case_traits(cs, t, pi=pi / pi.sum())
    c.delta[1] = np.where(c.delta[0] == 1.0, 1.0, c.delta[1])
    c.delta[t - 1] = np.where(c.delta[:t - 1].all(axis=0), 0.0, c.delta[t - 1])
    c.alpha[...] = c.delta * c.beta
    assert not np.isin([state_of(c.delta[:, j]) for j in range(c.p)], zero).any()
    return c, zero


# ---- the exact one-marker law: enumeration of the 2^t joint states ---------------------------------------------------------------------------
CONDITIONAL_STEPS = 3000
CONDITIONAL_SEED = 23


def conditional_case(t=5):
    """n = 83 individuals, ONE marker, t traits with correlated residuals and effects and a Pi table with every state possible.  With the
    variances held fixed, the t-step scan of the marker is a Gibbs sampler whose stationary law is the joint posterior of (delta, beta)
    given the record y = r + x alpha (which the sweep leaves unchanged); successive sweeps are a Markov chain on it."""
    rng = np.random.default_rng(83)
    n = 83
    x = np.round((rng.binomial(2, 0.4, size=(n, 1)) - 0.8) * 4) / 4     # (exact in Float32)
    vare = _spd(rng, t, 1.0, 0.4)
    G = _spd(rng, t, 0.02, 0.4)
    e = np.linalg.cholesky(vare) @ rng.standard_normal((t, n)) + rng.uniform(-0.15, 0.15, t)[:, None] * x[:, 0][None, :]
    tab = rng.dirichlet(np.full(1 << t, 4.0))
    return SweepResult(n=n, t=t, X=x, e=e, vare=vare, G=G, pi=tab, Rinv=inv_small(vare), Ginv=inv_small(G), log_pi=log_table(tab))


def conditional_posterior(case):
    """By enumeration.  With w = X'y, xx = x'x and, for a state S (the traits in the model), D = diag(delta): integrating the prior
    beta ~ N(0, G) against exp(-0.5 (y - x D beta)' Rinv (...)) gives for every state
        precision P_S = Ginv + xx D Rinv D,  mean m_S = P_S^-1 D Rinv w,  log weight = log pi_S - 0.5 log det P_S + 0.5 m_S' P_S m_S
    (the common factor det G^-1/2 dropped).  Returns (prob [2^t], mean [2^t, t], cov [2^t, t, t]) of beta | state."""
    t = case.t
    xx = float((case.X[:, 0] ** 2).sum())
    w = case.e @ case.X[:, 0]
    Rinv, Ginv = np.linalg.inv(case.vare), np.linalg.inv(case.G)
    lw, means, covs = np.empty(1 << t), np.empty((1 << t, t)), np.empty((1 << t, t, t))
    for s in range(1 << t):
        D = np.diag([float((s >> k) & 1) for k in range(t)])
        P = Ginv + xx * D @ Rinv @ D
        C = np.linalg.inv(P)
        m = C @ (D @ Rinv @ w)
        lw[s] = case.log_pi[s] - 0.5 * np.linalg.slogdet(P)[1] + 0.5 * m @ P @ m
        means[s], covs[s] = m, C
    pr = np.exp(lw - lw.max())
    return pr / pr.sum(), means, covs


def conditional_engine(engine, case):
    engine.load_dense(case.X.astype(engine.dtype))
    engine.mtj_begin(case.t, 64)
    engine.mtj_set_residual(case.e)                                      # alpha = 0: r = y
    return engine


def conditional_check(engine, case, seed=CONDITIONAL_SEED, steps=CONDITIONAL_STEPS, burn=20, thin=3):
    """Run `steps` sweeps and keep every `thin`-th after `burn` (the scan of one marker mixes within a sweep or two; thinning leaves nearly
    independent draws).  Returns (rows_trait, rows_state): per trait (k, z of the marginal inclusion frequency, z of the mean of beta_k,
    z of the variance of beta_k) against the enumerated mixture, and per state with an expected count >= 25 (s, z of its frequency, the
    largest z over the traits of the mean and of the variance of beta | state).  Every figure must be <= 5."""
    prob, means, covs = conditional_posterior(case)
    t = case.t
    states, betas = [], []
    for it in range(1, steps + 1):
        engine.mtj_sweep(iteration=it, seed=seed, rinv=case.Rinv, ginv=case.Ginv, log_pi=case.log_pi)
        if it > burn and (it - burn) % thin == 0:
            _, b, d = engine.mtj_get_state()
            states.append(state_of(d[:, 0]))
            betas.append(b[:, 0].copy())
    states, betas = np.array(states), np.array(betas)
    m = len(states)
    rows_trait, rows_state = [], []
    for k in range(t):
        pk = prob[[s for s in range(1 << t) if (s >> k) & 1]].sum()
        zf = abs(((states >> k) & 1).mean() - pk) / np.sqrt(pk * (1 - pk) / m)
        mu = float(prob @ means[:, k])
        var = float(prob @ (covs[:, k, k] + means[:, k] ** 2)) - mu * mu
        m4 = float(prob @ (3 * covs[:, k, k] ** 2 + 6 * covs[:, k, k] * (means[:, k] - mu) ** 2 + (means[:, k] - mu) ** 4))      # central, of the mixture
        zm = abs(betas[:, k].mean() - mu) / np.sqrt(var / m)
        zv = abs(betas[:, k].var(ddof=1) - var) / np.sqrt((m4 - var * var) / m)
        rows_trait.append((k, zf, zm, zv))
    for s in range(1 << t):
        if prob[s] * m >= 25:
            sel = betas[states == s]
            ns = len(sel)
            zf = abs(ns / m - prob[s]) / np.sqrt(prob[s] * (1 - prob[s]) / m)
            if ns < 10:
                rows_state.append((s, zf, np.inf, np.inf))
                continue
            v = np.diag(covs[s])
            zm = float((np.abs(sel.mean(axis=0) - means[s]) / np.sqrt(v / ns)).max())
            zv = float((np.abs(sel.var(axis=0, ddof=1) - v) / (v * np.sqrt(2.0 / (ns - 1)))).max())
            rows_state.append((s, zf, zm, zv))
    return rows_trait, rows_state
