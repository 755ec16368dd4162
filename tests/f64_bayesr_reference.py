"""Float64 restatement of BayesR! (BayesR.jl:56-96) in the sequential block form the Float64 device context runs
(csrc/f64_path.hpp: k64_update_partial / k64_sample<kBayesR> / k64_finish): per block the right-hand sides X_b'R^-1 r, then
`nreps` passes over the block's markers in order (nreps = 0: the block's own size, BayesABC.jl:153), every change of an effect
corrects the block's right-hand sides through the block Gram X_b'R^-1 X_b, then the residual takes the block's changes.
independent=True (BayesABC_block_independent!, BayesABC.jl:190-255): every block's right-hand sides from the residual at the
start of the sweep, the residual reconciled afterwards block by block, in marker order (k64_finish).  Any partition, residual
weights, a 4-vector or a p x 4 matrix of class priors, a marker offset.  TEST INFRASTRUCTURE, plain numpy / Python floats.

With one pass per block this is the literal per-marker chain (oracle.bayesr_sweep64, the C restatement) up to the association
of the sums; tests/test_f64_bayesr_host.py pins it to that chain before anything on the device is judged by it.  Draws: the
exported counter RNG (oracle.uniform / oracle.normal) on the slots of orc64_bayesr_sweep and of R64 in csrc/f64_path.hpp:
counter (marker0 + j, iteration, repetition, slot 0), one uniform and one normal per marker and repetition.  The scalar
algebra follows orc64_bayesr_sweep operation for operation."""
import math

import numpy as np

import oracle as O
from oracle_engine import OracleEngine64, BAYESR


def _log(x):
    return math.log(x) if x > 0.0 else (-math.inf if x == 0.0 else math.nan)


def marker_constants(d, ie, sigma_sq, pj, gamma):
    """What BayesR! computes for a marker that does not depend on its right-hand side (the same operations, :64-72, :88-91):
    d * ie, log pi per class, and per nonzero class invLhs, log(invLhs) - log(varEffect), sqrt(invLhs)."""
    lpi = [_log(v) for v in pj]
    inv_lhs, logs, sd = [0.0] * 4, [0.0] * 4, [0.0] * 4
    for k in range(1, 4):
        varEffect = gamma[k] * sigma_sq
        invVarEffect = 1.0 / varEffect
        lhs = d * ie + invVarEffect
        inv_lhs[k] = 1.0 / lhs
        logs[k] = math.log(inv_lhs[k]) - math.log(varEffect)
        sd[k] = math.sqrt(inv_lhs[k])
    return lpi, inv_lhs, logs, sd


def bayesr_update(x_r, d, a_old, ie, consts, u, z):
    """BayesR! for one marker (BayesR.jl:56-96), T = Float64: x_r = x'R^-1 r with the marker's own effect still in r,
    d = x'R^-1 x, consts = marker_constants(...).  Returns (new effect, new class 1..4)."""
    lpi, inv_lhs, logs, sd = consts
    rhs = (x_r + d * a_old) * ie                                                     # :60
    lp = [lpi[0], 0.0, 0.0, 0.0]                                                     # :64
    for k in range(1, 4):                                                            # :65-72
        betaHat = inv_lhs[k] * rhs
        lp[k] = 0.5 * (logs[k] + betaHat * rhs) + lpi[k]
    mx = lp[0]
    for k in range(1, 4):
        if lp[k] > mx:
            mx = lp[k]
    se = 0.0
    for k in range(4):
        se += math.exp(lp[k] - mx)
    log_norm = mx + math.log(se)                                                     # bayesr_logsumexp :1-4
    probs = [math.exp(lp[k] - log_norm) for k in range(4)]                           # :75-77
    cls = 0                                                                          # rand(Categorical(probs)) :79
    cp = probs[0]
    while cp <= u and cls < 3:
        cls += 1
        cp += probs[cls]
    if cls == 0:                                                                     # :82-86
        return 0.0, 1
    return inv_lhs[cls] * rhs + z * sd[cls], cls + 1                                 # :88-94


def block_grams(X, starts, w=None):
    """X_b'R^-1 X_b of every block of the partition `starts` (0-based block starts)."""
    n, p = X.shape
    ww = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    bounds = list(starts) + [p]
    out = []
    for bi in range(len(starts)):
        Xb = X[:, int(bounds[bi]):int(bounds[bi + 1])]
        out.append(Xb.T @ (ww[:, None] * Xb))
    return out


def bayesr_block_sweep(X, xpx, r, alpha, delta, vare, sigma_sq, pi, seed, it, starts, nreps=1, independent=False, w=None,
                       gamma=O.GAMMA, marker0=0, grams=None):
    """One sweep, in place.  X n x p; r (n), alpha (p) float64; delta (p) int32 classes 1..4; pi: 4 class priors or p x 4;
    starts: block starts (0-based); grams: block_grams(X, starts, w) when the caller keeps them."""
    n, p = X.shape
    ie = 1.0 / float(vare)
    sigma_sq = float(sigma_sq)
    pm = np.asarray(pi, dtype=np.float64)
    gam = [float(g) for g in np.asarray(gamma, dtype=np.float64)]
    ww = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    bounds = list(starts) + [p]
    if grams is None:
        grams = block_grams(X, starts, w)
    seed, it = int(seed), int(it)
    snap = r * ww                                                                    # (independent: the snapshot, weighted once)
    changes = []
    for bi in range(len(starts)):
        j0, j1 = int(bounds[bi]), int(bounds[bi + 1])
        b = j1 - j0
        Xb = X[:, j0:j1]
        Gram = grams[bi]
        rhs = (snap if independent else r * ww) @ Xb                                 # X_b'R^-1 r (block_rhs!)
        a_start = alpha[j0:j1].copy()
        dj = [float(v) for v in xpx[j0:j1]]
        consts = [marker_constants(dj[c], ie, sigma_sq, (pm[j0 + c] if pm.ndim == 2 else pm).tolist(), gam) for c in range(b)]
        for rep in range(nreps if nreps > 0 else b):
            for c in range(b):
                j = j0 + c
                a_old = float(alpha[j])
                u = O.uniform(seed, marker0 + j, it, rep, 0)
                z = O.normal(seed, marker0 + j, it, rep, 0)
                a_new, cls = bayesr_update(float(rhs[c]), dj[c], a_old, ie, consts[c], u, z)
                alpha[j] = a_new
                delta[j] = cls
                coef = a_old - a_new
                if coef != 0.0:
                    rhs += coef * Gram[c]                                            # BayesABC.jl:169,172
        dlt = a_start - alpha[j0:j1]
        nz = np.flatnonzero(dlt)
        if independent:
            changes.append((Xb, nz, dlt))
        elif len(nz):
            r += Xb[:, nz] @ dlt[nz]                                                 # :181-185
    for Xb, nz, dlt in changes:                                                      # :251-253, (block, marker) order
        if len(nz):
            r += Xb[:, nz] @ dlt[nz]


class BayesROracleEngine64(OracleEngine64):
    """OracleEngine64 whose BayesR sweep is the block restatement above (repetitions, weights, explicit partitions,
    independent blocks); every other method runs on the parent (the C oracle)."""

    def _drop_grams(self):
        self._r_grams = None

    def load_dense(self, X):
        super().load_dense(X)
        self._drop_grams()

    def setup_blocks(self, block_size=128, gram_mode="f64"):
        super().setup_blocks(block_size, gram_mode)
        self._drop_grams()

    def setup_blocks_explicit(self, starts, gram_mode="f64"):
        super().setup_blocks_explicit(starts, gram_mode)
        self._drop_grams()

    def set_weights(self, rinv):
        super().set_weights(rinv)
        self._drop_grams()

    def sweep(self, *, iteration, seed, vare, var_effect, pi_classes=None, gamma=O.GAMMA, pi_matrix=None, nreps=1,
              marker_offset=0, independent_blocks=False, **kw):
        if self.method != BAYESR:
            return super().sweep(iteration=iteration, seed=seed, vare=vare, var_effect=var_effect, pi_classes=pi_classes, gamma=gamma,
                                 pi_matrix=pi_matrix, nreps=nreps, marker_offset=marker_offset, independent_blocks=independent_blocks, **kw)
        w = getattr(self, "_w", None)
        starts = self.block_starts()
        if getattr(self, "_r_grams", None) is None:
            self._r_grams = block_grams(self.X, starts, w)
        a_before = self.alpha.copy()
        bayesr_block_sweep(self.X, self._xpx, self.r[0], self.alpha[0], self.delta[0], float(np.asarray(vare).reshape(-1)[0]),
                           float(np.asarray(var_effect).reshape(-1)[0]), pi_matrix if pi_matrix is not None else pi_classes,
                           seed, iteration, starts, nreps=nreps, independent=bool(independent_blocks), w=w, gamma=gamma,
                           marker0=marker_offset, grams=self._r_grams)
        ww = np.ones(self.n) if w is None else w
        d = self.delta[0]
        nz = d > 1
        return {"alpha_ss": self.alpha @ self.alpha.T, "beta_ss": self.beta @ self.beta.T, "resid_ss": (self.r * ww) @ self.r.T,
                "resid_sum": (self.r * ww).sum(axis=1), "n_events": float(np.any(a_before != self.alpha, axis=0).sum()), "sweep_ms": 0.0,
                "class_counts": np.array([(d == k + 1).sum() for k in range(4)], dtype=np.float64),
                "bayesr_ssq": float((self.alpha[0][nz] ** 2 / np.asarray(gamma)[d[nz] - 1]).sum()), "bayesr_nnz": float(nz.sum()),
                "sum_delta": np.zeros(1), "state_counts": np.zeros(2)}
