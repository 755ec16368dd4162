"""TEST INFRASTRUCTURE: a numpy Float64 restatement of the device's random-regression sweep (csrc/rrm.hpp) on the same Philox counters,
and a stand-in engine with the rrm_* methods of HipEngine.  The package never imports this file.

n individuals with genotype rows x_i., T time points, Phi (T x c) with rows phi_t, obs (T x n booleans), W the T x n residual (0 at
every cell without a record), vare a scalar, G c x c, pi over the 2^c states (bit q of the state index = coefficient q).
    O_i  = sum_t m_it phi_t phi_t'         M_j = sum_i x_ij^2 O_i         G_jk = sum_i x_ij x_ik O_i
One marker, markers in order:
    s_j  = sum_i x_ij sum_t m_it phi_t W_it,   xw = s_j + M_j alpha_j
    every state: lhs = D M_j D / vare + inv(G), rhs = D xw / vare, mu = inv(lhs) rhs, logDelta = -0.5 (log det lhs - rhs'mu) + log pi
    state by the CDF walk of softmax(logDelta) with ONE uniform (the last state when rounding leaves u above the total)
    beta = mu + chol(inv(lhs)) z with one shared z,   alpha_new = D beta,   W_it += m_it x_ij phi_t'(alpha_j - alpha_new)
u = u52 of words (1, 0) of philox(marker, iteration, 0x02000000, 8); z_q Box-Muller of philox(marker, iteration, 0x02000000, 9 + 16 q).
sweep_plain is that chain marker by marker; sweep_blocked is the exact block form the device runs (s_k of a block from the residual at
block entry, s_k += G_kj d on every change, the residual brought up to date at block exit).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from liability_reference import philox4x32_10  # noqa: E402

RRM_TAG, RRM_SLOT_U, RRM_SLOT_Z = 0x02000000, 8, 9
MIN_COEFF, MAX_COEFF, MAX_TIMES, MAX_BLOCK = 2, 4, 64, 256
TWO_PI = 6.283185307179586476925286766559


def _u52(lo, hi):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def rrm_uniform(markers, iteration, seed):
    seed = int(seed)
    w0, w1, _, _ = philox4x32_10(np.asarray(markers, dtype=np.uint64), np.uint64(iteration), np.uint64(RRM_TAG), np.uint64(RRM_SLOT_U),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return _u52(w0, w1)


def rrm_normal(markers, iteration, seed, q):
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(np.asarray(markers, dtype=np.uint64), np.uint64(iteration), np.uint64(RRM_TAG), np.uint64(RRM_SLOT_Z + 16 * int(q)),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(TWO_PI * _u52(w2, w3))


def draws(p, c, iteration, seed):
    """(u [p], z [p, c]) of one sweep."""
    j = np.arange(p)
    return rrm_uniform(j, iteration, seed), np.stack([rrm_normal(j, iteration, seed, q) for q in range(c)], axis=1)


def inv_small(A):
    """The library's c x c inverse: Gauss-Jordan with partial pivoting, operation for operation (csrc/ctx.hpp)."""
    A = np.asarray(A, dtype=np.float64)
    t = A.shape[0]
    M = np.hstack([A.copy(), np.eye(t)])
    for c in range(t):
        piv = c
        for i in range(c + 1, t):
            if abs(M[i, c]) > abs(M[piv, c]):
                piv = i
        if M[piv, c] == 0.0:
            raise np.linalg.LinAlgError("singular")
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for i in range(t):
            if i != c and M[i, c] != 0.0:
                M[i] = M[i] - M[i, c] * M[c]
    return M[:, t:].copy()


def occupancy(Phi, obs):
    """O (n x c x c): O_i = sum_t m_it phi_t phi_t'."""
    return np.einsum("ti,ta,tb->iab", np.asarray(obs, dtype=np.float64), Phi, Phi)


def m_array(X, O):
    """M (p x c x c) -- get_mPhiPhiarray, RRM.jl:43-57."""
    X = np.asarray(X, dtype=np.float64)
    return np.einsum("ij,iab->jab", X * X, O)


def gram_block(X, O, j0, b):
    """G (b x b x c x c) of the markers j0 .. j0 + b - 1."""
    Xb = np.asarray(X[:, j0:j0 + b], dtype=np.float64)
    return np.einsum("ij,ik,iab->jkab", Xb, Xb, O)


def marker_states(Mj, Ginv, ie, xw, log_pi):
    """Per state: (logDelta, mu, inv(lhs))."""
    c = len(xw)
    out = []
    for s in range(1 << c):
        D = np.array([(s >> q) & 1 for q in range(c)], dtype=np.float64)
        lhs = (D[:, None] * Mj * D[None, :]) * ie + Ginv
        rhs = (D * xw) * ie
        L = np.linalg.cholesky(lhs)
        Li = np.linalg.inv(L)
        inv = Li.T @ Li
        mu = inv @ rhs
        out.append((-0.5 * (2.0 * np.log(np.diag(L)).sum() - rhs @ mu) + log_pi[s], mu, inv))
    return out


def state_probabilities(Mj, Ginv, ie, xw, log_pi):
    st = marker_states(Mj, Ginv, ie, xw, log_pi)
    ld = np.array([v[0] for v in st])
    e = np.exp(ld - ld.max())
    return e / e.sum(), st


def sample_marker(Mj, Ginv, ie, s, alpha_j, log_pi, u, z):
    """One marker: (state, beta, alpha_new, margin) -- margin: the distance of u from the nearest boundary of the state CDF."""
    c = len(s)
    xw = s + Mj @ alpha_j
    prob, st = state_probabilities(Mj, Ginv, ie, xw, log_pi)
    cdf = np.cumsum(prob)
    which = (1 << c) - 1
    for k in range(1 << c):
        if u < cdf[k]:
            which = k
            break
    margin = float(np.min(np.abs(cdf[:-1] - u)))
    _, mu, inv = st[which]
    beta = mu + np.linalg.cholesky(inv) @ z
    D = np.array([(which >> q) & 1 for q in range(c)], dtype=np.float64)
    return which, beta, D * beta, margin


U = 2.0 ** -53


def marker_bound(Mj, Mabs, Ginv, ie, xw, dxw, which, z, n):
    """A bound on |beta_device - beta_restatement| of one marker whose right-hand side differs by at most dxw (entry by entry), both
    sides choosing the state `which`.  u = 2^-53, c coefficients.
      M_j           two summation orders of the same n products: 2 (n + 2) u Mabs, Mabs = sum_i x_ij^2 sum_t m_it |phi_t| |phi_t|'
      lhs, rhs      d lhs = D dM D / vare + 2 u |lhs| + 4 c (c + 1) u ||lhs||_2 -- the last term is the backward error of the Cholesky
                    factorisations behind inv(lhs) (|dA| <= gamma_(c+1) |R'||R|, || |R'||R| ||_2 <= c ||A||_2; Higham, Accuracy and
                    Stability, Thm 10.3), taken for the factor, its inverse, the product and the second factor;  d rhs = D dxw / vare + 2 u |rhs|
      mu            twice the first-order bound of a perturbed solve: 2 |inv| (d rhs + d lhs |mu|)
      K z           K = chol(inv(lhs)): inv moves by E, |E| <= 2 |inv| d lhs |inv|, its factor by at most ||K||_2 ||inv(K)||_2^2 ||E||_F
                    (first order, norm-wise; doubled), plus 2^-46 sum_m |K|_qm for Box-Muller (the argument of tests/test_gpu_sem.py)
      beta          the sum, plus 2 u |beta|."""
    c = len(xw)
    D = np.array([(which >> q) & 1 for q in range(c)], dtype=np.float64)
    lhs = (D[:, None] * Mj * D[None, :]) * ie + Ginv
    rhs = (D * xw) * ie
    inv = np.linalg.inv(lhs)
    mu = inv @ rhs
    K = np.linalg.cholesky((inv + inv.T) / 2)
    n2 = np.linalg.norm(lhs, 2)
    dlhs = (D[:, None] * (2 * (n + 2) * U * Mabs) * D[None, :]) * ie + 2 * U * np.abs(lhs) + 4 * c * (c + 1) * U * n2
    drhs = D * dxw * ie + 2 * U * np.abs(rhs)
    ainv = np.abs(inv)
    dmu = 2 * ainv @ (drhs + dlhs @ np.abs(mu))
    E = 2 * ainv @ dlhs @ ainv
    Kn, Kin = np.linalg.norm(K, 2), np.linalg.norm(np.linalg.inv(K), 2)
    dkz = 2 * Kn * Kin ** 2 * np.linalg.norm(E, "fro") * np.linalg.norm(z) + 2.0 ** -46 * np.abs(K).sum(axis=1)
    beta = mu + K @ z
    return dmu + dkz + 2 * U * np.abs(beta)


def phi_times(Phi, d):
    """g_t = phi_t'd, q ascending from the first product (the order of the device's table)."""
    g = Phi[:, 0] * d[0]
    for q in range(1, Phi.shape[1]):
        g = g + Phi[:, q] * d[q]
    return g


def apply_change(W, obs, x, g):
    """W_it = W_it + x_i g_t where the individual has a record (in place)."""
    W[...] = np.where(obs, W + x[None, :] * g[:, None], W)


def v_of(W, obs, Phi):
    """v (n x c): v_i = sum_t m_it phi_t W_it."""
    return np.where(obs, W, 0.0).T @ Phi


class SweepResult(dict):
    __getattr__ = dict.__getitem__


def _finish(W, alpha, beta, delta, states, changed, margins, abs_s):
    c = alpha.shape[0]
    counts = np.bincount(states, minlength=1 << c).astype(np.float64)
    return SweepResult(state_counts=counts, beta_ss=beta @ beta.T, alpha_ss=float((alpha * alpha).sum()), resid_ss=float((W * W).sum()),
                       n_changed=float(changed), step_ms=0.0, states=states, margins=np.array(margins), abs_s=abs_s)


def sweep_plain(X, Phi, obs, M, W, alpha, beta, delta, *, iteration, seed, vare, G, log_pi, min_margin=0.0):
    """The chain marker by marker (RRM.jl:101-158); W, alpha, beta, delta (c x p) are updated in place."""
    X = np.asarray(X, dtype=np.float64)
    p, c = X.shape[1], Phi.shape[1]
    Ginv, ie = inv_small(G), 1.0 / float(vare)
    u, z = draws(p, c, iteration, seed)
    states, margins, changed = np.zeros(p, dtype=np.int64), [], 0
    for j in range(p):
        s = X[:, j] @ v_of(W, obs, Phi)
        which, b_new, a_new, mg = sample_marker(M[j], Ginv, ie, s, alpha[:, j].copy(), log_pi, u[j], z[j])
        d = alpha[:, j] - a_new
        if np.any(d != 0.0):
            apply_change(W, obs, X[:, j], phi_times(Phi, d))
            changed += 1
        alpha[:, j], beta[:, j], delta[:, j] = a_new, b_new, [(which >> q) & 1 for q in range(c)]
        states[j] = which
        margins.append(mg)
    assert min(margins) >= min_margin, f"a uniform lies within {min_margin} of a state boundary ({min(margins)})"
    return _finish(W, alpha, beta, delta, states, changed, margins, None)


def sweep_blocked(X, Phi, obs, M, grams, W, alpha, beta, delta, *, block_size, iteration, seed, vare, G, log_pi, min_margin=0.0, bounds=False):
    """The exact block form; grams[k]: gram_block of block k.
    bounds=True: the result also carries err_beta (c x p) and err_W (T x n), bounds on what a device that runs the same chain in
    another summation order may differ by when both start from this state and choose the same states.  Per marker k the right-hand
    side differs by  d s_k = sum_{j changed before k} Gabs_kj err_d_j  (an earlier marker's difference reaches k through the Gram
    correction inside a block and through the residual across blocks: to first order both are G_kj err_d_j, Gabs_kj = |G_kj|)
    + 2 (N + 2) u abs_s_k, N = n T + c (b + 2) products, abs_s_k the sum of the absolute values of every term that enters s_k and
    M_k alpha_k; marker_bound carries it to beta; err_d_j = D err_beta_j."""
    X = np.asarray(X, dtype=np.float64)
    n, p, c = X.shape[0], X.shape[1], Phi.shape[1]
    Ginv, ie = inv_small(G), 1.0 / float(vare)
    u, z = draws(p, c, iteration, seed)
    states, margins, changed = np.zeros(p, dtype=np.int64), [], 0
    abs_s = np.zeros((p, c))
    if bounds:
        Xa, Oabs, O_ = np.abs(X), occupancy(np.abs(Phi), obs), occupancy(Phi, obs)
        Mabs = m_array(Xa, Oabs)
        err_d, err_beta = np.zeros((p, c)), np.zeros((c, p))
    for k, j0 in enumerate(range(0, p, block_size)):
        b = min(block_size, p - j0)
        Xb = X[:, j0:j0 + b]
        s = Xb.T @ v_of(W, obs, Phi)                                   # b x c
        sa = np.abs(Xb).T @ (np.where(obs, np.abs(W), 0.0).T @ np.abs(Phi))
        Gk = grams[k]
        events = []
        for a in range(b):
            j = j0 + a
            which, b_new, a_new, mg = sample_marker(M[j], Ginv, ie, s[a], alpha[:, j].copy(), log_pi, u[j], z[j])
            abs_s[j] = sa[a] + np.abs(M[j]) @ np.abs(alpha[:, j])
            d = alpha[:, j] - a_new
            if bounds:
                Gabs_j = np.abs(np.einsum("i,ik,iab->kab", X[:, j], X[:, :j], O_))      # |x_j'(...) x_k|: the first-order reach of marker k's difference
                abs_j = sa[a] + Mabs[j] @ np.abs(alpha[:, j])
                dxw = np.einsum("kab,kb->a", Gabs_j, err_d[:j]) + 2 * (n * Phi.shape[0] + c * (b + 2) + 2) * U * abs_j
                err_beta[:, j] = marker_bound(M[j], Mabs[j], Ginv, ie, s[a] + M[j] @ alpha[:, j], dxw, which, z[j], n)
                if np.any(d != 0.0):
                    err_d[j] = err_beta[:, j] * [(which >> q) & 1 for q in range(c)]
            if np.any(d != 0.0):
                s = s + np.einsum("kab,b->ka", Gk[:, a], d)
                sa = sa + np.einsum("kab,b->ka", np.einsum("i,ik,iab->kab", np.abs(X[:, j]), np.abs(Xb), occupancy(np.abs(Phi), obs)) if bounds else np.abs(Gk[:, a]), np.abs(d))
                events.append((j, d))
                changed += 1
            alpha[:, j], beta[:, j], delta[:, j] = a_new, b_new, [(which >> q) & 1 for q in range(c)]
            states[j] = which
            margins.append(mg)
        for j, d in events:
            apply_change(W, obs, X[:, j], phi_times(Phi, d))
    assert min(margins) >= min_margin, f"a uniform lies within {min_margin} of a state boundary ({min(margins)})"
    out = _finish(W, alpha, beta, delta, states, changed, margins, abs_s)
    if bounds:
        out["err_beta"], out["err_d"] = err_beta, err_d
        out["err_W"] = np.where(obs, (np.abs(Phi) @ (Xa @ err_d).T), 0.0) + 4 * U * np.abs(W)
    return out


def conditional_recheck(X, Phi, obs, W0, alpha0, alpha1, states, *, iteration, seed, vare, G):
    """Every marker's update recomputed from the OTHER side's own history: with d_j = alpha0_j - alpha1_j the changes a device made
    to the markers before k, the chain's right-hand side of marker k is  s_k = x_k'v(W0) + sum_{j<k} G_kj d_j  whatever the blocks
    (inside a block the correction is G_kj d_j, across blocks the residual carries x_j phi'd_j and x_k'(...) gives the same term).
    Returns (beta [c x p], bound [c x p]): the restatement's beta of marker k in state states[k] from that s_k, and the bound on a
    device's difference from it.  The inputs of marker k are then the same doubles on both sides, so only the order of the sums in
    s_k, M_k and G_kj differs: d xw <= 2 (N + 2) u abs_s_k with N = n T + (c + 2) p products at most (the residual of a row carries
    one rounded product per changed marker) and abs_s_k = sum_i |x_ik| sum_t m_it |phi_t| |W0_it| + sum_{j<k} Gabs_kj |d_j| + Mabs_k |alpha0_k|,
    Gabs and Mabs the sums of the absolute products; marker_bound carries it through the c x c solve."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    T, c = Phi.shape
    Ginv, ie = inv_small(G), 1.0 / float(vare)
    _, z = draws(p, c, iteration, seed)
    O, Xa, Oabs = occupancy(Phi, obs), np.abs(X), occupancy(np.abs(Phi), obs)
    M, Mabs = m_array(X, O), m_array(Xa, Oabs)
    s0 = X.T @ v_of(W0, obs, Phi)
    sa0 = Xa.T @ (np.where(obs, np.abs(W0), 0.0).T @ np.abs(Phi))
    d = alpha0 - alpha1
    beta, bound = np.zeros((c, p)), np.zeros((c, p))
    for k in range(p):
        Gk = np.einsum("i,ij,iab->jab", X[:, k], X[:, :k], O)
        Gak = np.einsum("i,ij,iab->jab", Xa[:, k], Xa[:, :k], Oabs)
        s = s0[k] + np.einsum("jab,bj->a", Gk, d[:, :k])
        abs_s = sa0[k] + np.einsum("jab,bj->a", Gak, np.abs(d[:, :k])) + Mabs[k] @ np.abs(alpha0[:, k])
        xw = s + M[k] @ alpha0[:, k]
        dxw = 2 * (n * T + (c + 2) * p + 2) * U * abs_s
        which = int(states[k])
        _, mu, inv = marker_states(M[k], Ginv, ie, xw, np.zeros(1 << c))[which]
        beta[:, k] = mu + np.linalg.cholesky(inv) @ z[k]
        bound[:, k] = marker_bound(M[k], Mabs[k], Ginv, ie, xw, dxw, which, z[k], n)
    return beta, bound


def legendre_phi(times, ncoeff=3):
    """Closed-form normalised Legendre columns on [-1, 1] (RRM.jl:24-39), for ncoeff <= 5."""
    t = np.sort(np.unique(np.asarray(times, dtype=np.float64)))
    q = 2.0 * (t - t.min()) / (t.max() - t.min()) - 1.0
    P = [np.ones_like(q), q, 0.5 * (3 * q ** 2 - 1), 0.5 * (5 * q ** 3 - 3 * q), 0.125 * (35 * q ** 4 - 30 * q ** 2 + 3)]
    return np.stack([np.sqrt((2 * k + 1) / 2.0) * P[k] for k in range(ncoeff)], axis=1)


class RrmStandInEngine:
    """The rrm_* methods of HipEngine (and the little else the RRM driver calls) on the restatement above."""

    def __init__(self, precision=64):
        self.precision = int(precision)
        self.dtype = np.float64 if precision == 64 else np.float32
        self.n = self.p = 0
        self._rrm = None

    def close(self):
        pass

    def load_dense(self, X):
        X = np.asarray(X)
        if X.dtype != self.dtype:
            raise TypeError(f"this engine stores {np.dtype(self.dtype).name} genotypes")
        self.X = X.astype(np.float64)
        self.n, self.p = X.shape
        self._rrm = None

    @staticmethod
    def rrm_estimate_bytes(n, p, ntimes, ncoeff, block_size=64):
        ld, cells, bs = (n + 255) // 256 * 256, ncoeff * (ncoeff + 1) // 2, block_size or 64
        nblocks = (p + bs - 1) // bs
        return 8 * (ld + ntimes * ncoeff + cells * ld + ntimes * ld + p * cells + nblocks * bs * bs * cells + 6 * ncoeff * p + (ld // 256) * bs * ncoeff +
                    34 + ld // 256 + ld) + (8 + 4 * 256 + 8 * 4 * 256 + 8 * 256 * 64)

    def _need(self):
        if self._rrm is None:
            raise ValueError("rrm_begin has not been called")
        return self._rrm

    def rrm_begin(self, Phi, observed, block_size=64):
        Phi = np.ascontiguousarray(Phi, dtype=np.float64)
        obs = np.asarray(observed).astype(bool)
        if self.p == 0:
            raise ValueError("no genotype matrix loaded")
        T, c = Phi.shape
        if not MIN_COEFF <= c <= MAX_COEFF:
            raise ValueError(f"the number of regression coefficients must be in [{MIN_COEFF},{MAX_COEFF}]")
        if not 1 <= T <= MAX_TIMES:
            raise ValueError(f"the number of time points must be in [1,{MAX_TIMES}]")
        if obs.shape != (T, self.n):
            raise ValueError("observed must be T x n")
        if not np.all(np.isfinite(Phi)) or not 0 <= int(block_size) <= MAX_BLOCK:
            raise ValueError("Phi must be finite and the block size in [1,256]")
        bs = int(block_size) or 64
        O = occupancy(Phi, obs)
        s = SweepResult(Phi=Phi, obs=obs, bs=bs, T=T, c=c, O=O, M=m_array(self.X, O),
                        grams=[gram_block(self.X, O, j0, min(bs, self.p - j0)) for j0 in range(0, self.p, bs)],
                        W=np.zeros((T, self.n)), alpha=np.zeros((c, self.p)), beta=np.zeros((c, self.p)), delta=np.ones((c, self.p)),
                        acc=[np.zeros((c, self.p)) for _ in range(3)])
        self._rrm = s

    def rrm_set_residual(self, W):
        s = self._need()
        W = np.asarray(W, dtype=np.float64)
        if W.shape != (s.T, self.n):
            raise ValueError("the residual must be T x n")
        s.W[...] = np.where(s.obs, W, 0.0)

    def rrm_get_residual(self):
        return self._need().W.copy()

    def rrm_set_state(self, alpha=None, beta=None, delta=None):
        s = self._need()
        for name, a in (("alpha", alpha), ("beta", beta), ("delta", delta)):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.shape != (s.c, self.p) or not np.all(np.isfinite(a)):
                    raise ValueError("state arrays must be finite and c x p")
                s[name][...] = a

    def rrm_get_state(self):
        s = self._need()
        return s.alpha.copy(), s.beta.copy(), s.delta.copy()

    def rrm_sweep(self, *, iteration, seed, vare, G, log_pi, min_margin=0.0):
        s = self._need()
        G = np.asarray(G, dtype=np.float64)
        if int(iteration) < 1 or not (np.isfinite(vare) and vare > 0) or G.shape != (s.c, s.c) or not np.all(np.isfinite(G)):
            raise ValueError("iteration >= 1, vare > 0 and a finite c x c G are needed")
        np.linalg.cholesky(G)
        return sweep_blocked(self.X, s.Phi, s.obs, s.M, s.grams, s.W, s.alpha, s.beta, s.delta, block_size=s.bs, iteration=iteration, seed=seed,
                             vare=vare, G=G, log_pi=np.asarray(log_pi, dtype=np.float64), min_margin=min_margin)

    def rrm_accumulate(self, nsamples):
        s = self._need()
        for acc, v in zip(s.acc, (s.alpha, s.alpha * s.alpha, s.delta)):
            acc += (v - acc) / nsamples

    def rrm_posterior(self, q):
        return tuple(a[q].copy() for a in self._need().acc)

    def rrm_mul_alpha(self, q):
        return self.X @ self._need().alpha[q]

    def rrm_m(self):
        return self._need().M.copy()

    def rrm_gram(self, block):
        return self._need().grams[block].copy()

    def rrm_end(self):
        self._need()
        self._rrm = None


# ---- fixed inputs shared by tests/test_rrm_host.py and tests/test_gpu_rrm.py ----------------------------------------------------------
def make_case(n, p, T, c, missing, seed, single_record=0):
    """Genotypes (centred 0/1/2 counts, exactly representable in Float32), Phi, the record pattern and a starting state.
    missing: the fraction of cells without a record; single_record: that many individuals keep one record only.  Every individual
    keeps at least one record."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.1, 0.9, p)
    X = (rng.binomial(2, freq, size=(n, p)) - 1.0).astype(np.float64)
    Phi = legendre_phi(np.arange(T), c) if T > 1 and c <= 5 else rng.standard_normal((T, c))
    obs = rng.random((T, n)) >= missing
    for i in range(single_record):
        obs[:, i] = False
        obs[rng.integers(T), i] = True
    for i in np.flatnonzero(~obs.any(axis=0)):
        obs[rng.integers(T), i] = True
    W = np.where(obs, rng.standard_normal((T, n)), 0.0)
    delta = (rng.random((c, p)) < 0.6).astype(np.float64)
    beta = 0.05 * rng.standard_normal((c, p))
    alpha = delta * beta
    A = rng.standard_normal((c, c))
    G = 0.01 * (A @ A.T + c * np.eye(c))
    G = (G + G.T) / 2
    pi = rng.dirichlet(np.full(1 << c, 2.0))
    return SweepResult(n=n, p=p, T=T, c=c, X=X, Phi=Phi, obs=obs, W=W, alpha=alpha, beta=beta, delta=delta, G=G, vare=0.9, log_pi=np.log(pi))


# ---- the exact-conditional case: one marker, c = 2 -----------------------------------------------------------------------------------
CONDITIONAL_STEPS = 4000
CONDITIONAL_SEED = 23


def conditional_case():
    """n = 83 individuals, T = 3, one marker, two coefficients.  xw = s + M alpha does not depend on the marker's current
    coefficients (adding x phi'alpha back to the residual gives the record minus everything else), so with the variances held
    fixed every sweep draws (state, beta) from the same closed-form posterior, independently from step to step (the Philox counter
    changes with the iteration) -- the argument of the reference's test_multitrait_mcmc.jl:557-642."""
    rng = np.random.default_rng(83)
    n, T, c = 83, 3, 2
    x = (rng.binomial(2, 0.4, size=(n, 1)) - 0.8).astype(np.float64)
    x = np.round(x * 4) / 4                                            # (exact in Float32)
    Phi = legendre_phi(np.arange(T), c)
    obs = rng.random((T, n)) >= 0.2
    obs[0, ~obs.any(axis=0)] = True
    e = np.where(obs, 0.9 * rng.standard_normal((T, n)) + 0.12 * x[:, 0][None, :] * (Phi @ np.array([1.0, -0.8]))[:, None], 0.0)
    return SweepResult(n=n, T=T, c=c, X=x, Phi=Phi, obs=obs, e=e, vare=0.81, G=np.array([[0.02, 0.004], [0.004, 0.015]]),
                       log_pi=np.log(np.array([0.3, 0.2, 0.2, 0.3])))


def conditional_posterior(case):
    """(state probabilities, [(mu, V)] per state) of the closed-form posterior."""
    O = occupancy(case.Phi, case.obs)
    M = m_array(case.X, O)[0]
    s = case.X[:, 0] @ v_of(case.e, case.obs, case.Phi)                # alpha = 0: xw = s
    prob, st = state_probabilities(M, inv_small(case.G), 1.0 / case.vare, s, case.log_pi)
    return prob, [(mu, V) for _, mu, V in st]


def conditional_engine(engine, case):
    engine.load_dense(case.X.astype(engine.dtype))
    engine.rrm_begin(case.Phi, case.obs, 64)
    engine.rrm_set_residual(case.e)                                    # alpha = 0: W = e
    return engine


def conditional_check(engine, case, seed=CONDITIONAL_SEED, steps=CONDITIONAL_STEPS):
    """Run `steps` sweeps; returns (rows_state, rows_coef): rows_state = [(state, |freq - P| / sqrt(P (1 - P) / N))], rows_coef =
    [(state, q, |mean - mu_q| / sqrt(V_qq / N_s), |var - V_qq| / (V_qq sqrt(2 / (N_s - 1))))].  Every figure must be <= 5."""
    prob, mom = conditional_posterior(case)
    c = case.c
    states, betas = np.empty(steps, dtype=np.int64), np.empty((steps, c))
    for it in range(1, steps + 1):
        engine.rrm_sweep(iteration=it, seed=seed, vare=case.vare, G=case.G, log_pi=case.log_pi)
        _, b, d = engine.rrm_get_state()
        states[it - 1] = sum(int(d[q, 0]) << q for q in range(c))
        betas[it - 1] = b[:, 0]
    rows_state, rows_coef = [], []
    for s in range(1 << c):
        sel = states == s
        ns = int(sel.sum())
        rows_state.append((s, abs(ns / steps - prob[s]) / np.sqrt(prob[s] * (1 - prob[s]) / steps)))
        mu, V = mom[s]
        for q in range(c):
            xq = betas[sel, q]
            rows_coef.append((s, q, abs(xq.mean() - mu[q]) / np.sqrt(V[q, q] / ns), abs(xq.var(ddof=1) - V[q, q]) / (V[q, q] * np.sqrt(2.0 / (ns - 1)))))
    return rows_state, rows_coef
