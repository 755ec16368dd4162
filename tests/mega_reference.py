"""TEST INFRASTRUCTURE: a numpy Float64 restatement of the device's mega-trait sweep (csrc/mega.hpp) on the same Philox counters, and
a stand-in engine with the mega_* methods of HipEngine.  The package never imports this file.

n individuals with genotype rows x_i., T traits, R the T x n residual, per trait vare_k, the effect variance v_k and pi_k.
One marker of one trait, markers in order (bayesabc_update_marker!, BayesABC.jl:24-58):
    rhs = (x_j'r + xpx_j alpha_j) / vare,  lhs = xpx_j / vare + 1 / v,  gHat = rhs / lhs
    logDelta1 = -0.5 (log lhs + log v - gHat rhs) + log(1 - pi),  logDelta0 = log pi,  probDelta1 = 1 / (1 + exp(logDelta0 - logDelta1))
    u < probDelta1: delta = 1, beta = alpha = gHat + z sqrt(1 / lhs);  else delta = 0, alpha = 0, beta = z sqrt(v);  r += x_j (alpha_old - alpha_new)
u = u52 of words (1, 0) of philox(marker, iteration, 0x01000000 | trait_id, 10); z Box-Muller of philox(marker, iteration, 0x01000000 |
trait_id, 11); the normal of a missing cell: philox(record, iteration, 0x01000000 | trait_id, 12); trait_id = first_trait + k.
sweep_plain is that chain marker by marker; sweep_blocked is the exact block form the device runs (s_j of a block from the residual at
block entry, s_i += G_ij d on every change, the residual brought up to date at block exit: per trait the changed markers ascending,
r = r + x_j d_j one marker after the other -- the device's order, so a residual recomputed this way from the device's own changes
compares bit for bit).  Every other sum here is numpy's; where the device is compared with this file the tests carry a rounding bound,
and where bits are compared (independence of T, same seed) both sides are the device.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from liability_reference import philox4x32_10  # noqa: E402

MEGA_TAG, SLOT_U, SLOT_Z, SLOT_MISS = 0x01000000, 10, 11, 12
MAX_TRAITS, MAX_BLOCK, TRAIT_TILE = 64, 256, 8
TWO_PI = 6.283185307179586476925286766559
U = 2.0 ** -53
MIN_MARGIN = 1e-9


def _u52(lo, hi):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def _words(index, iteration, trait_id, slot, seed):
    seed = int(seed)
    return philox4x32_10(np.asarray(index, dtype=np.uint64), np.uint64(iteration), np.uint64(MEGA_TAG | int(trait_id)), np.uint64(slot),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def mega_uniform(markers, iteration, seed, trait_id):
    w0, w1, _, _ = _words(markers, iteration, trait_id, SLOT_U, seed)
    return _u52(w0, w1)


def _normal(index, iteration, seed, trait_id, slot):
    w0, w1, w2, w3 = _words(index, iteration, trait_id, slot, seed)
    return np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(TWO_PI * _u52(w2, w3))


def mega_normal(markers, iteration, seed, trait_id):
    return _normal(markers, iteration, seed, trait_id, SLOT_Z)


def missing_normal(records, iteration, seed, trait_id):
    return _normal(records, iteration, seed, trait_id, SLOT_MISS)


def draws(p, T, iteration, seed, first_trait=0):
    """(u [T, p], z [T, p]) of one sweep."""
    j = np.arange(p)
    return (np.stack([mega_uniform(j, iteration, seed, first_trait + k) for k in range(T)]),
            np.stack([mega_normal(j, iteration, seed, first_trait + k) for k in range(T)]))


def gram_block(X, j0, b):
    Xb = np.asarray(X[:, j0:j0 + b], dtype=np.float64)
    return Xb.T @ Xb


def marker_law(xpx, s, alpha, vare, v, pi, u, z):
    """One marker of every trait at once (arrays over the traits): (delta, beta, alpha_new, probDelta1)."""
    with np.errstate(divide="ignore", over="ignore"):
        ie, iv = 1.0 / vare, 1.0 / v
        rhs = (s + xpx * alpha) * ie
        lhs = xpx * ie + iv
        inv_lhs = 1.0 / lhs
        g_hat = rhs * inv_lhs
        ld1 = -0.5 * (np.log(lhs) + np.log(v) - g_hat * rhs) + np.log(1.0 - pi)
        prob = 1.0 / (1.0 + np.exp(np.log(pi) - ld1))
    inc = u < prob
    beta = np.where(inc, g_hat + z * np.sqrt(inv_lhs), z * np.sqrt(v))
    return inc.astype(np.float64), beta, np.where(inc, beta, 0.0), prob


class SweepResult(dict):
    __getattr__ = dict.__getitem__


def _finish(R, alpha, beta, delta, alpha0, margins):
    return SweepResult(sum_delta=delta.sum(axis=1), beta_ss=(beta * beta).sum(axis=1), alpha_ss=(alpha * alpha).sum(axis=1),
                       resid_ss=(R * R).sum(axis=1), resid_sum=R.sum(axis=1), n_changed=(alpha != alpha0).sum(axis=1).astype(np.float64),
                       step_ms=0.0, margins=margins)


def _par(T, vare, var_effect, pi):
    out = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (vare, var_effect, pi)]
    assert all(a.shape == (T,) for a in out)
    return out


def sweep_plain(X, R, alpha, beta, delta, *, iteration, seed, vare, var_effect, pi, first_trait=0, min_margin=0.0):
    """The chain marker by marker (BayesABC.jl:60-116 per trait); R, alpha, beta, delta (T x .) are updated in place."""
    X = np.asarray(X, dtype=np.float64)
    T, p = alpha.shape
    vare, v, pi = _par(T, vare, var_effect, pi)
    u, z = draws(p, T, iteration, seed, first_trait)
    alpha0, margins = alpha.copy(), np.empty((T, p))
    xpx = (X * X).sum(axis=0)
    for j in range(p):
        d_new, b_new, a_new, prob = marker_law(xpx[j], R @ X[:, j], alpha[:, j], vare, v, pi, u[:, j], z[:, j])
        R += (alpha[:, j] - a_new)[:, None] * X[:, j][None, :]
        alpha[:, j], beta[:, j], delta[:, j] = a_new, b_new, d_new
        margins[:, j] = np.abs(u[:, j] - prob)
    assert margins.min() >= min_margin, f"a decision uniform lies within {min_margin} of probDelta1 ({margins.min()})"
    return _finish(R, alpha, beta, delta, alpha0, margins)


def apply_changes(R, X, d):
    """The device's residual update of a block: per trait the changed markers ascending, r = r + x_j d_j one after the other
    (d: T x b changes of the block's markers, X: their columns).  In place."""
    for a in range(d.shape[1]):
        ch = d[:, a] != 0.0
        if ch.any():
            R[ch] = R[ch] + X[:, a][None, :] * d[ch, a][:, None]


def sweep_blocked(X, R, alpha, beta, delta, *, block_size, iteration, seed, vare, var_effect, pi, first_trait=0, min_margin=0.0, grams=None):
    """The exact block form; grams[k]: gram_block of block k (formed here when None)."""
    X = np.asarray(X, dtype=np.float64)
    T, p = alpha.shape
    vare, v, pi = _par(T, vare, var_effect, pi)
    u, z = draws(p, T, iteration, seed, first_trait)
    alpha0, margins = alpha.copy(), np.empty((T, p))
    for k, j0 in enumerate(range(0, p, block_size)):
        b = min(block_size, p - j0)
        Xb = X[:, j0:j0 + b]
        G = grams[k] if grams is not None else Xb.T @ Xb
        s = R @ Xb                                                       # T x b
        D = np.zeros((T, b))
        for a in range(b):
            j = j0 + a
            d_new, b_new, a_new, prob = marker_law(G[a, a], s[:, a], alpha[:, j], vare, v, pi, u[:, j], z[:, j])
            d = alpha[:, j] - a_new
            s = s + d[:, None] * G[a][None, :]
            D[:, a] = d
            alpha[:, j], beta[:, j], delta[:, j] = a_new, b_new, d_new
            margins[:, j] = np.abs(u[:, j] - prob)
        apply_changes(R, Xb, D)
    assert margins.min() >= min_margin, f"a decision uniform lies within {min_margin} of probDelta1 ({margins.min()})"
    return _finish(R, alpha, beta, delta, alpha0, margins)


def impute(R, missing, *, iteration, seed, vare, first_trait=0):
    """Every missing cell of R (T x n) redrawn: z sqrt(vare_k).  In place; observed cells are not touched."""
    T, n = R.shape
    vare = np.asarray(vare, dtype=np.float64).reshape(-1)
    for k in range(T):
        i = np.flatnonzero(missing[k])
        if i.size:
            R[k, i] = missing_normal(i, iteration, seed, first_trait + k) * np.sqrt(vare[k])


def marker_bound(xpx, xw, dxw, n, vare, v, delta, z):
    """A bound on |beta_device - beta_restatement| of one marker whose x'r + xpx alpha differs by at most dxw, both sides with the
    indicator delta.  u = 2^-53.
      xpx        two summation orders of the same n positive products: dx = 2 (n + 2) u xpx
      rhs, lhs   d rhs = dxw / vare + 2 u |rhs|,  d lhs = dx / vare + 2 u lhs
      gHat       twice the first-order bound of the perturbed scalar solve: 2 (d rhs + d lhs |gHat|) / lhs
      z sqrt(1 / lhs)  |z| sqrt(1 / lhs) (d lhs / lhs + 4 u) (the square root halves the relative error; doubled), plus 2^-46 sqrt(1 / lhs)
                 for Box-Muller (the argument of tests/test_gpu_sem.py: the angle 2 pi u2 carries one rounding, the cosine passes it on
                 as an absolute error, the radius <= 8.5 multiplies, plus a few ulp of the library functions)
      beta       the sum, plus 2 u |beta|;  delta = 0: beta = z sqrt(v), the Box-Muller term 2^-46 sqrt(v) plus 4 u |beta|."""
    if delta == 0.0:
        return 2.0 ** -46 * np.sqrt(v) + 4 * U * abs(z) * np.sqrt(v)
    ie = 1.0 / vare
    rhs, lhs = xw * ie, xpx * ie + 1.0 / v
    g_hat, sd = rhs / lhs, np.sqrt(1.0 / lhs)
    dx = 2 * (n + 2) * U * xpx
    drhs, dlhs = dxw * ie + 2 * U * abs(rhs), dx * ie + 2 * U * lhs
    dg = 2 * (drhs + dlhs * abs(g_hat)) / lhs
    dz = abs(z) * sd * (dlhs / lhs + 4 * U) + 2.0 ** -46 * sd
    return dg + dz + 2 * U * abs(g_hat + z * sd)


def conditional_recheck(X, R0, alpha0, alpha1, delta1, *, iteration, seed, vare, var_effect, first_trait=0):
    """Every marker's update recomputed from the OTHER side's own history: with d_i = alpha0_i - alpha1_i the changes a device made
    to the markers before j, the chain's right-hand side of marker j is  s_j = x_j'r0 + sum_{i<j} G_ji d_i  whatever the blocks
    (inside a block the correction is G_ji d_i, across blocks the residual carries x_i d_i and x_j'(...) gives the same term).
    Returns (beta [T x p], bound [T x p]): the restatement's beta of marker j under the device's indicator from that s_j, and the
    bound on a device's difference from it.  The inputs of marker j are the same doubles on both sides, so only the order of the
    sums differs: d xw <= 2 (N + 2) u abs_s_j with N = n + p + 1 products at most and abs_s_j = sum_i |x_ij| |r0_i| + sum_{i<j}
    Gabs_ji |d_i| + xpx_j |alpha0_j| (Gabs the sums of the absolute products); marker_bound carries it through the scalar solve."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    T = R0.shape[0]
    vare, v = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (vare, var_effect)]
    Xa = np.abs(X)
    G, Ga = np.tril(X.T @ X, -1), np.tril(Xa.T @ Xa, -1)                 # [j, i], i < j
    xpx = (X * X).sum(axis=0)
    d = alpha0 - alpha1
    S = R0 @ X + d @ G.T                                                 # T x p
    Sa = np.abs(R0) @ Xa + np.abs(d) @ Ga.T + xpx[None, :] * np.abs(alpha0)
    beta, bound = np.empty((T, p)), np.empty((T, p))
    for k in range(T):
        z = mega_normal(np.arange(p), iteration, seed, first_trait + k)
        xw = S[k] + xpx * alpha0[k]
        ie = 1.0 / vare[k]
        lhs = xpx * ie + 1.0 / v[k]
        beta[k] = np.where(delta1[k] != 0.0, (xw * ie) / lhs + z * np.sqrt(1.0 / lhs), z * np.sqrt(v[k]))
        dxw = 2 * (n + p + 3) * U * Sa[k]
        bound[k] = [marker_bound(xpx[j], xw[j], dxw[j], n, vare[k], v[k], delta1[k, j], z[j]) for j in range(p)]
    return beta, bound


def propagated_bound(X, R0, alpha0, res, *, iteration, seed, vare, var_effect, first_trait=0):
    """Bounds on what a device that runs the chain of `res` (a sweep of this file from R0, alpha0) in another summation order and
    block size may differ by when both choose the same indicators: err_beta [T x p].  Per marker j the right-hand side differs by
    d xw_j = sum_{i<j} Gabs_ji err_d_i (an earlier marker's difference reaches j through the Gram correction inside a block and
    through the residual across blocks: to first order both are G_ji err_d_i) + 2 (N + 2) u abs_s_j as in conditional_recheck;
    marker_bound carries it to beta; err_d_j = delta_j err_beta_j (an effect that leaves the model moves by exactly alpha0_j).
    Meaningful under a tight prior only, where a marker is moved by an earlier one's difference by less than that difference."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    T = R0.shape[0]
    vare, v = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (vare, var_effect)]
    Xa = np.abs(X)
    G, Ga = np.tril(X.T @ X, -1), np.tril(Xa.T @ Xa, -1)
    xpx = (X * X).sum(axis=0)
    d = alpha0 - res.alpha
    S = R0 @ X + d @ G.T
    Sa = np.abs(R0) @ Xa + np.abs(d) @ Ga.T + xpx[None, :] * np.abs(alpha0)
    err = np.zeros((T, p))
    for k in range(T):
        z = mega_normal(np.arange(p), iteration, seed, first_trait + k)
        err_d = np.zeros(p)
        for j in range(p):
            dxw = Ga[j, :j] @ err_d[:j] + 2 * (n + p + 3) * U * Sa[k, j]
            err[k, j] = marker_bound(xpx[j], S[k, j] + xpx[j] * alpha0[k, j], dxw, n, vare[k], v[k], res.delta[k, j], z[j])
            err_d[j] = err[k, j] * res.delta[k, j]
    return err


class BlockStandInEngine:
    """What the stand-ins of the two block sessions share (MegaStandInEngine, MtjStandInEngine): the loaders and the transfer of the
    residual, the state, the running means, X alpha and the Grams.  KIND ("mega", "mtj"): the session lives in self._<KIND>, a
    subclass names the methods <KIND>_* and adds its _begin and its sweep."""
    KIND = None

    def __init__(self, precision=64):
        self.precision = int(precision)
        self.dtype = np.float64 if precision == 64 else np.float32
        self.n = self.p = 0
        setattr(self, "_" + self.KIND, None)
        self.X = self.Xout = None
        self.calls = []

    def close(self):
        pass

    def load_dense(self, X):
        X = np.asarray(X)
        if X.dtype != self.dtype:
            raise TypeError(f"this engine stores {np.dtype(self.dtype).name} genotypes")
        self.X = X.astype(np.float64)
        self.n, self.p = X.shape
        setattr(self, "_" + self.KIND, None)
        self.calls.append("load_dense")

    def load_output_dense(self, X_out):
        X_out = np.asarray(X_out)
        if X_out.dtype != self.dtype:
            raise TypeError(f"this engine stores {np.dtype(self.dtype).name} genotypes")
        self.Xout = X_out.astype(np.float64)
        self.n_out = X_out.shape[0]

    def _need(self):
        s = getattr(self, "_" + self.KIND)
        if s is None:
            raise ValueError(f"{self.KIND}_begin has not been called")
        return s

    def _open(self, T, bs, **more):
        """The session of T traits in blocks of bs markers: residuals, alpha and beta 0, delta 1, the block Grams."""
        setattr(self, "_" + self.KIND, SweepResult(
            T=T, bs=bs, R=np.zeros((T, self.n)), alpha=np.zeros((T, self.p)), beta=np.zeros((T, self.p)), delta=np.ones((T, self.p)),
            acc=[np.zeros((T, self.p)) for _ in range(3)], grams=[gram_block(self.X, j0, min(bs, self.p - j0)) for j0 in range(0, self.p, bs)], **more))
        self.calls.append(self.KIND + "_begin")

    def _set_residual(self, R, trait=None):
        s = self._need()
        R = np.asarray(R, dtype=np.float64)
        if trait is None:
            if R.shape != (s.T, self.n) or not np.all(np.isfinite(R)):
                raise ValueError("the residual must be finite and T x n")
            s.R[...] = R
        else:
            s.R[int(trait)] = R

    def _get_residual(self, trait=None):
        s = self._need()
        return s.R.copy() if trait is None else s.R[int(trait)].copy()

    def _set_state(self, alpha=None, beta=None, delta=None):
        s = self._need()
        for name, a in (("alpha", alpha), ("beta", beta), ("delta", delta)):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.shape != (s.T, self.p) or not np.all(np.isfinite(a)):
                    raise ValueError("state arrays must be finite and T x p")
                s[name][...] = a

    def _get_state(self, trait=None):
        s = self._need()
        if trait is None:
            return s.alpha.copy(), s.beta.copy(), s.delta.copy()
        return s.alpha[int(trait)].copy(), s.beta[int(trait)].copy(), s.delta[int(trait)].copy()

    def _accumulate(self, nsamples):
        s = self._need()
        for acc, v in zip(s.acc, (s.alpha, s.alpha * s.alpha, s.delta)):
            acc += (v - acc) / nsamples

    def _posterior(self, trait):
        return tuple(a[int(trait)].copy() for a in self._need().acc)

    def _mul_alpha(self, trait, output_rows=False):
        return (self.Xout if output_rows else self.X) @ self._need().alpha[int(trait)]

    def _gram(self, block):
        G = self._need().grams[block]
        return G.copy(), np.diag(G).copy()

    def _finish(self):
        self._need()
        setattr(self, "_" + self.KIND, None)
        self.calls.append(self.KIND + "_end")


class MegaStandInEngine(BlockStandInEngine):
    """The mega_* methods of HipEngine (and the little else the mega-trait driver calls) on the restatement above."""
    KIND = "mega"
    mega_set_residual, mega_get_residual = BlockStandInEngine._set_residual, BlockStandInEngine._get_residual
    mega_set_state, mega_get_state = BlockStandInEngine._set_state, BlockStandInEngine._get_state
    mega_accumulate, mega_posterior = BlockStandInEngine._accumulate, BlockStandInEngine._posterior
    mega_mul_alpha, mega_gram, mega_end = BlockStandInEngine._mul_alpha, BlockStandInEngine._gram, BlockStandInEngine._finish

    @staticmethod
    def mega_estimate_bytes(n, p, ntraits, block_size=64):
        ld, bs = (n + 255) // 256 * 256, block_size or 64
        nsl, nblocks = ld // 256, (p + bs - 1) // bs
        return 8 * (ntraits * ld + p + nblocks * bs * bs + 6 * ntraits * p + nsl * ntraits * bs + 4 * ntraits + ntraits * (4 + 2 * nsl) + ld) + \
            4 * ntraits * (ld // 32) + (4 * 64 + 4 * 64 * 256 + 8 * 64 * 256)

    def mega_begin(self, ntraits, block_size=64, first_trait=0):
        if self.p == 0:
            raise ValueError("no genotype matrix loaded")
        if not 1 <= int(ntraits) <= MAX_TRAITS or not 0 <= int(block_size) <= MAX_BLOCK or int(first_trait) < 0:
            raise ValueError("the number of traits must be in [1,64] and the block size in [1,256]")
        self._open(int(ntraits), int(block_size) or 64, first=int(first_trait), missing=None)

    def mega_set_missing(self, missing):
        s = self._need()
        if missing is None:
            s["missing"] = None
            return
        m = np.asarray(missing).astype(bool)
        if m.shape != (s.T, self.n):
            raise ValueError("the missing pattern must be T x n")
        s["missing"] = m.copy()

    def mega_impute(self, *, iteration, seed, vare):
        s = self._need()
        self.calls.append("mega_impute")
        if s.missing is not None:
            impute(s.R, s.missing, iteration=iteration, seed=seed, vare=vare, first_trait=s.first)

    def mega_sweep(self, *, iteration, seed, vare, var_effect, pi, min_margin=0.0):
        s = self._need()
        self.calls.append("mega_sweep")
        vare, v, pi = _par(s.T, vare, var_effect, pi)
        if int(iteration) < 1 or not np.all(np.isfinite(vare) & (vare > 0)) or not np.all(np.isfinite(v) & (v > 0)) or not np.all((pi >= 0) & (pi <= 1)):
            raise ValueError("iteration >= 1, positive finite variances and pi in [0,1] are needed")
        return sweep_blocked(self.X, s.R, s.alpha, s.beta, s.delta, block_size=s.bs, iteration=iteration, seed=seed, vare=vare, var_effect=v, pi=pi,
                             first_trait=s.first, min_margin=min_margin, grams=s.grams)


# ---- fixed inputs shared by tests/test_megatrait_host.py and tests/test_gpu_megatrait.py ------------------------------------------------
PI_CYCLE = (0.0, 0.5, 0.95)


def make_case(n=301, p=100, seed=7):
    """Genotypes (0/1/2 counts centred by twice the allele frequency and rounded to Float32, so that both storage types hold the same
    values and products of two of them do not fit a double's sums exactly) and, for all 64 traits at once, a residual, a starting
    state, the variances, pi (0, 0.5, 0.95 in turn) and a pattern of ~20 % missing cells (trait 0 fully observed, the first 30
    records with a single observed trait).  Trait k of a T-trait test is row k whatever T: the rows do not depend on T."""
    rng = np.random.default_rng(seed)
    T = MAX_TRAITS
    freq = rng.uniform(0.1, 0.9, p)
    X = (rng.binomial(2, freq, size=(n, p)) - 2.0 * freq).astype(np.float32).astype(np.float64)      # (24-bit values: the sums do round)
    R = rng.standard_normal((T, n))
    delta = (rng.random((T, p)) < 0.4).astype(np.float64)
    beta = 0.05 * rng.standard_normal((T, p))
    alpha = delta * beta
    vare = rng.uniform(0.6, 1.4, T)
    v = rng.uniform(0.002, 0.01, T)
    pi = np.array([PI_CYCLE[k % 3] for k in range(T)])
    missing = rng.random((T, n)) < 0.2
    missing[0] = False
    for i in range(30):
        missing[:, i] = True
        missing[rng.integers(T) if i % 2 else 0, i] = False
    missing[0] = False
    return SweepResult(n=n, p=p, X=X, R=R, alpha=alpha, beta=beta, delta=delta, vare=vare, v=v, pi=pi, missing=missing)


def case_traits(cs, T, first=0):
    """The traits first .. first + T - 1 of a case."""
    sl = slice(first, first + T)
    return SweepResult(n=cs.n, p=cs.p, X=cs.X, R=cs.R[sl].copy(), alpha=cs.alpha[sl].copy(), beta=cs.beta[sl].copy(), delta=cs.delta[sl].copy(),
                       vare=cs.vare[sl].copy(), v=cs.v[sl].copy(), pi=cs.pi[sl].copy(), missing=cs.missing[sl].copy())


def reference_sweep(cs, T, iteration, seed, block_size, vscale=1.0):
    """The restatement's own sweep of the first T traits from the case's state; asserts the margin of every decision uniform."""
    c = case_traits(cs, T)
    r = sweep_blocked(c.X, c.R, c.alpha, c.beta, c.delta, block_size=block_size, iteration=iteration, seed=seed, vare=c.vare, var_effect=c.v * vscale,
                      pi=c.pi, min_margin=MIN_MARGIN)
    r.update(R=c.R, alpha=c.alpha, beta=c.beta, delta=c.delta)
    return r


# ---- the exact-conditional case: one marker, three traits -------------------------------------------------------------------------------
CONDITIONAL_STEPS = 4000
CONDITIONAL_SEED = 23


def conditional_case():
    """n = 83 individuals, one marker, three traits with pi = 0.3, 0.5, 0.7.  x'r + xpx alpha does not depend on the marker's current
    effect (adding x alpha back to the residual gives the record minus everything else), so with the variances held fixed every
    sweep draws (delta, beta) from the same closed-form posterior, independently from step to step (the Philox counter changes
    with the iteration)."""
    rng = np.random.default_rng(83)
    n, T = 83, 3
    x = np.round((rng.binomial(2, 0.4, size=(n, 1)) - 0.8) * 4) / 4     # (exact in Float32)
    vare = np.array([0.81, 1.1, 0.6])
    v = np.array([0.02, 0.015, 0.03])
    e = np.sqrt(vare)[:, None] * rng.standard_normal((T, n)) + np.array([0.12, -0.1, 0.15])[:, None] * x[:, 0][None, :]
    return SweepResult(n=n, T=T, X=x, e=e, vare=vare, v=v, pi=np.array([0.3, 0.5, 0.7]))


def conditional_posterior(case):
    """Per trait (probDelta1, gHat, 1 / lhs)."""
    xpx = float((case.X[:, 0] ** 2).sum())
    s = case.e @ case.X[:, 0]
    _, _, _, prob = marker_law(xpx, s, np.zeros(case.T), case.vare, case.v, case.pi, np.zeros(case.T), np.zeros(case.T))
    lhs = xpx / case.vare + 1.0 / case.v
    return prob, (s / case.vare) / lhs, 1.0 / lhs


def conditional_engine(engine, case):
    engine.load_dense(case.X.astype(engine.dtype))
    engine.mega_begin(case.T, 64, 0)
    engine.mega_set_residual(case.e)                                     # alpha = 0: r = e
    return engine


def conditional_check(engine, case, seed=CONDITIONAL_SEED, steps=CONDITIONAL_STEPS):
    """Run `steps` sweeps; returns rows (trait, z of the frequency, z of mean and variance of beta | delta = 1, z of mean and variance of
    beta | delta = 0).  Every figure must be <= 5."""
    prob, mu, var1 = conditional_posterior(case)
    T = case.T
    deltas, betas = np.empty((steps, T)), np.empty((steps, T))
    for it in range(1, steps + 1):
        engine.mega_sweep(iteration=it, seed=seed, vare=case.vare, var_effect=case.v, pi=case.pi)
        _, b, d = engine.mega_get_state()
        deltas[it - 1], betas[it - 1] = d[:, 0], b[:, 0]
    rows = []
    for k in range(T):
        inc = deltas[:, k] == 1.0
        n1, n0 = int(inc.sum()), int((~inc).sum())
        zf = abs(n1 / steps - prob[k]) / np.sqrt(prob[k] * (1 - prob[k]) / steps)
        b1, b0 = betas[inc, k], betas[~inc, k]
        rows.append((k, zf, abs(b1.mean() - mu[k]) / np.sqrt(var1[k] / n1), abs(b1.var(ddof=1) - var1[k]) / (var1[k] * np.sqrt(2.0 / (n1 - 1))),
                     abs(b0.mean()) / np.sqrt(case.v[k] / n0), abs(b0.var(ddof=1) - case.v[k]) / (case.v[k] * np.sqrt(2.0 / (n0 - 1)))))
    return rows
