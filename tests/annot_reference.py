"""TEST INFRASTRUCTURE: a numpy restatement of the device's annotation-prior update (csrc/annot.hpp) on the same Philox counters
and in the same order of every sum, and stand-in engines that add the annot methods of HipEngine to the oracle engines.

Step s of a model (BayesC: 1 step; BayesR and the 2-trait tree: 3), with its coefficients c_0 .. c_K-1 and the design matrix D
(column 0 ones):
    (a) mu_i = c_0 + sum_{k >= 1} D_ik c_k                      k ascending, multiply then add
    (b) i in A_s: u = u52(philox(i, iteration, 0x08000000 | s, 5)), e_i = truncated_std_normal(lo, hi, u) with
        (lo, hi) = (-mu_i, +Inf) if z_i else (-Inf, -mu_i); liability_i = mu_i + e_i forced onto its side of 0
    (c) k = 0 .. K - 1: S_k = sum_A D_ik e_i, d_k = sum_A D_ik^2 (d_0 = n_A), inv_k = 1 / (d_k + 1 / var_s) (inv_0 = 1 / n_A),
        c_k' = inv_k (S_k + d_k c_k) + z_k sqrt(inv_k), e_i += D_ik (c_k - c_k') on A_s;
        z_k = sqrt(-2 ln u1) cos(2 pi u2) from philox(k, iteration, 0x08000000 | s, 6)
    (d) n_A = 0: nothing is drawn, the coefficients stay
    (e) mu from the new coefficients, P_s = clip(Phi(mu), eps, 1 - eps), Phi(x) = erfc(-x / sqrt 2) / 2, eps = 2^-52
Sums: pieces of 1024 consecutive markers; within a piece 256 partial sums (thread j: markers j, j + 256, j + 512, j + 768 in that
order) meet in a tree 128 .. 1; the piece sums are added the same way (thread j: pieces j, j + 256, ...; the same tree).  Given
the same e the sums are the device's bit for bit; e itself differs by the libm of erfc / erfcinv (here ndtr / ndtri), log and cos,
which tests/test_gpu_annot.py bounds.
"""
import os
import sys

import numpy as np
from scipy.special import erfc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine, OracleEngine64  # noqa: E402
from f64_mt_reference import RestatementEngine64  # noqa: E402
from liability_reference import philox4x32_10, truncated_std_normal  # noqa: E402

PIECE = 1024
TAG = 0x08000000
EPS = 2.0 ** -52
KINDS = {"BayesC": 0, "BayesR": 1, "tree": 2}
BAYESC, BAYESR, MTBAYESC1, MTBAYESC2, MEGABAYESC, MEGABAYESB = 0, 2, 3, 4, 5, 8


def _u52(lo, hi):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def annot_uniform(markers, iteration, step, seed):
    seed = int(seed)
    w0, w1, _, _ = philox4x32_10(np.asarray(markers, dtype=np.uint64), np.uint64(iteration), np.uint64(TAG | int(step)), np.uint64(5),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return _u52(w0, w1)


def annot_normal(k, iteration, step, seed):
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(np.asarray([k], dtype=np.uint64), np.uint64(iteration), np.uint64(TAG | int(step)), np.uint64(6),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return float((np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(6.283185307179586476925286766559 * _u52(w2, w3)))[0])


def _tree(a):
    """a: (..., 256) -> (...,): the device's tree 128 .. 1."""
    a = a.copy()
    w = 128
    while w >= 1:
        a[..., :w] = a[..., :w] + a[..., w:2 * w]
        w >>= 1
    return a[..., 0]


def _strided(v):
    """v (m,) -> the 256 partial sums of threads that add entries j, j + 256, ... in that order."""
    rows = max(1, -(-len(v) // 256))
    pad = np.zeros(rows * 256)
    pad[:len(v)] = v
    a = pad.reshape(rows, 256)
    acc = a[0].copy()
    for r in range(1, rows):
        acc = acc + a[r]
    return acc


def ordered_sum(v):
    """sum of the per-marker values v (zeros outside the active set) in the device's order."""
    p = len(v)
    npieces = -(-p // PIECE)
    pad = np.zeros(npieces * PIECE)
    pad[:p] = v
    a = pad.reshape(npieces, PIECE // 256, 256)
    acc = a[:, 0].copy()
    for q in range(1, PIECE // 256):
        acc = acc + a[:, q]
    return float(_tree(_strided(_tree(acc))))


def mu_of(D, coef):
    mu = np.full(D.shape[0], coef[0], dtype=np.float64)
    for k in range(1, D.shape[1]):
        mu = mu + D[:, k] * coef[k]
    return mu


def response(kind, s, d1, d2=None):
    """(active, z) of step s."""
    if kind == 0:
        return np.ones(d1.shape, dtype=bool), d1 != 0
    if kind == 1:
        cl = np.asarray(d1).astype(np.int64)
        return (np.ones(cl.shape, dtype=bool) if s == 0 else cl > s), cl > s + 1
    a, b = d1 != 0, d2 != 0
    if s == 0:
        return np.ones(a.shape, dtype=bool), a | b
    if s == 1:
        return a | b, a & b
    return a ^ b, a & ~b


def probit_step(D, coef, liab, act, z, var, *, iteration, step, seed, all_active, dsq, detail=None):
    """(a)-(d) of one step.  coef (K,) and liab (p,) are updated in place."""
    p, K = D.shape
    mu = mu_of(D, coef)
    nA = int(act.sum())
    if detail is not None:
        detail.update(mu_in=mu, n_active=nA, e0=np.zeros(p), S=[], d=[], inv=[], old=coef.copy(), A=[])
    if nA == 0:
        return nA
    idx = np.flatnonzero(act)
    za = z[idx]
    u = annot_uniform(idx, iteration, step, seed)
    ea = truncated_std_normal(np.where(za, -mu[idx], -np.inf), np.where(za, np.inf, -mu[idx]), u)
    la = mu[idx] + ea
    liab[idx] = np.where(za, np.fmax(la, 0.0), np.fmin(la, 0.0))
    e = np.zeros(p)
    e[idx] = ea
    if detail is not None:
        detail["e0"] = e.copy()
    dc = 0.0
    for k in range(K):
        x = np.ones(p) if k == 0 else D[:, k]
        if k > 0:
            xp = np.ones(p) if k == 1 else D[:, k - 1]
            e[idx] = e[idx] + xp[idx] * dc
        S = ordered_sum(np.where(act, x * e, 0.0))
        d = float(nA) if k == 0 else (dsq[k] if all_active else ordered_sum(np.where(act, x * x, 0.0)))
        inv = 1.0 / nA if k == 0 else 1.0 / (d + 1.0 / var)
        zk = annot_normal(k, iteration, step, seed)
        new = inv * (S + d * coef[k]) + zk * np.sqrt(inv)
        if detail is not None:
            detail["S"].append(S); detail["d"].append(d); detail["inv"].append(inv)
            detail["A"].append(float(np.abs(x * e)[act].sum()))
        dc = coef[k] - new
        coef[k] = new
    return nA


def phi(mu):
    return 0.5 * erfc(-mu * 0.70710678118654752440)


def table_of(kind, D, coef):
    """coef (nsteps, K) -> (mu (nsteps, p), table, probabilities (p,) | (p, 4))."""
    mu = np.stack([mu_of(D, c) for c in coef])
    if kind == 0:
        pi = np.clip(1.0 - phi(mu[0]), EPS, 1.0 - EPS)
        return mu, pi, pi
    p1, p2, p3 = [np.clip(phi(m), EPS, 1.0 - EPS) for m in mu]
    if kind == 1:
        rows = np.stack([1.0 - p1, p1 * (1.0 - p2), (p1 * p2) * (1.0 - p3), (p1 * p2) * p3], axis=1)
        return mu, rows, rows
    rows = np.stack([1.0 - p1, (p1 * (1.0 - p2)) * p3, (p1 * (1.0 - p2)) * (1.0 - p3), p1 * p2], axis=1)
    return mu, np.log(rows), rows


def column_means(rows):
    rows = rows.reshape(len(rows), -1)
    return np.array([ordered_sum(rows[:, c]) / len(rows) for c in range(rows.shape[1])])


class _AnnotMixin:
    """The annot methods of HipEngine (and sweep(resident_priors=True)) on an engine that keeps its indicators in self.delta."""

    @staticmethod
    def annot_estimate_bytes(p, ncols, kind):
        ns, tab = (1, p) if kind == "BayesC" else (3, 4 * p)
        return 8 * (max(ncols - 1, 1) * p + 2 * ns * p + p + 3 * tab)

    def annot_begin(self, kind, design_matrix, coefficients, variance, start_prior):
        if getattr(self, "_an", None) is not None:
            raise RuntimeError("an annotation session is already open")
        if self.method is None:
            raise RuntimeError("init_state first")
        code = KINDS[kind]
        if self.method in (MEGABAYESC, MEGABAYESB):
            raise NotImplementedError("annotation priors are not available with constraint = true")
        fits = {0: self.method == BAYESC and self.ntraits == 1, 1: self.method == BAYESR and self.ntraits == 1,
                2: self.method in (MTBAYESC1, MTBAYESC2) and self.ntraits == 2}[code]
        if not fits:
            raise ValueError("the annotation kind does not match the engine's method")
        D = np.array(design_matrix, dtype=np.float64)
        if D.shape[0] != self.p or not np.all(D[:, 0] == 1.0) or not np.all(np.isfinite(D)):
            raise ValueError("design_matrix must be p x ncols with a first column of ones")
        ns = 1 if code == 0 else 3
        K = D.shape[1]
        table = np.array(start_prior, dtype=np.float64).reshape((self.p,) if ns == 1 else (self.p, 4))
        self._an = {"kind": code, "ns": ns, "D": D, "coef": np.array(coefficients, dtype=np.float64).reshape(K, ns).T.copy(),
                    "liab": np.zeros((ns, self.p)), "mu": np.zeros((ns, self.p)), "table": table,
                    "mean": np.zeros(table.shape), "mean2": np.zeros(table.shape),
                    "dsq": np.array([0.0] + [ordered_sum(D[:, k] * D[:, k]) for k in range(1, K)])}

    def annot_step(self, *, iteration, seed, variance, details=None):
        an = self._an
        if int(iteration) < 1:
            raise ValueError("iteration must be >= 1")
        var = np.broadcast_to(np.asarray(variance, dtype=np.float64), (an["ns"],))
        if an["D"].shape[1] > 1 and not np.all(np.isfinite(var) & (var > 0)):
            raise ValueError("variance must be positive and finite")
        d1 = self.delta[0]
        d2 = self.delta[1] if an["kind"] == 2 else None
        nA = []
        for s in range(an["ns"]):
            act, z = response(an["kind"], s, d1, d2)
            det = {} if details is not None else None
            nA.append(probit_step(an["D"], an["coef"][s], an["liab"][s], act, z, float(var[s]), iteration=iteration, step=s, seed=seed,
                                  all_active=s == 0, dsq=an["dsq"], detail=det))
            if details is not None:
                det.update(act=act, z=z)
                details.append(det)
        an["mu"], an["table"], rows = table_of(an["kind"], an["D"], an["coef"])
        cf = an["coef"]
        return {"coefficients": cf[0].copy() if an["ns"] == 1 else np.ascontiguousarray(cf.T), "n_active": np.array(nA),
                "means": column_means(rows), "step_ms": 0.0}

    def annot_accumulate(self, nsamples):
        an = self._an
        v = np.exp(an["table"]) if an["kind"] == 2 else an["table"]
        an["mean"] = an["mean"] + (v - an["mean"]) / nsamples
        an["mean2"] = an["mean2"] + (v * v - an["mean2"]) / nsamples

    def annot_prior(self):
        return self._an["table"].copy()

    def annot_means(self):
        return self._an["mean"].copy(), self._an["mean2"].copy()

    def _annot_steps(self, a):
        return a[0].copy() if self._an["ns"] == 1 else np.ascontiguousarray(a.T)

    def annot_liability(self):
        return self._annot_steps(self._an["liab"])

    def annot_mu(self):
        return self._annot_steps(self._an["mu"])

    def annot_end(self):
        self._an = None

    def init_state(self, method, ntraits=1):
        self._an = None
        return super().init_state(method, ntraits)

    def sweep(self, *, resident_priors=False, **kw):
        if resident_priors:
            an = self._an
            if any(kw.get(k) is not None for k in ("pi_vec", "pi_matrix")) or np.ndim(kw.get("log_prior_states")) == 2:
                raise ValueError("resident_priors=True takes no per-marker prior")
            key = {0: "pi_vec", 1: "pi_matrix", 2: "log_prior_states"}[an["kind"]]
            kw[key] = an["table"]
        return super().sweep(**kw)


class AnnotOracleEngine(_AnnotMixin, OracleEngine):
    pass


class AnnotOracleEngine64(_AnnotMixin, RestatementEngine64):
    pass


# ---- the exact-posterior case shared by tests/test_annot_host.py and tests/test_gpu_annot.py -------------------------------------
POSTERIOR_STEPS, POSTERIOR_BATCHES = 3000, 30
POSTERIOR_SEED = 11
POSTERIOR_VARIANCE = 1.0


def posterior_case():
    """p = 400 markers, 2 annotations, a fixed delta whose inclusion follows the first annotation: with the shrinkage variance fixed
    the step alone is the Albert-Chib sampler of a probit regression."""
    rng = np.random.default_rng(400)
    p = 400
    A = np.column_stack([(rng.random(p) < 0.4).astype(np.float64), rng.standard_normal(p)])
    D = np.hstack([np.ones((p, 1)), A])
    eta = -0.8 + 1.1 * A[:, 0] + 0.3 * A[:, 1]
    delta = (eta + rng.standard_normal(p) > 0).astype(np.float64)
    return {"p": p, "D": D, "delta": delta, "X": rng.standard_normal((24, p))}


def posterior_engine(engine, case):
    engine.load_dense(case["X"])
    engine.setup_blocks(8 if not hasattr(engine, "_L") else 64, "f64")
    engine.init_state("BayesC", 1)
    engine.set_state(0, delta=case["delta"])
    engine.annot_begin("BayesC", case["D"], np.zeros(3), POSTERIOR_VARIANCE, np.full(case["p"], 0.5))
    return engine


def batch_means(chain, nbatches=POSTERIOR_BATCHES):
    chain = np.asarray(chain)
    bm = chain.reshape(nbatches, -1, chain.shape[1]).mean(axis=1)
    return chain.mean(axis=0), bm.std(axis=0, ddof=1) / np.sqrt(nbatches)


def posterior_chain(engine, steps=POSTERIOR_STEPS, seed=POSTERIOR_SEED):
    """The coefficient chain of `steps` device-form steps at the fixed variance."""
    chain = np.empty((steps, 3))
    for it in range(1, steps + 1):
        chain[it - 1] = engine.annot_step(iteration=it, seed=seed, variance=POSTERIOR_VARIANCE)["coefficients"]
    return chain


def host_chain(case, steps=POSTERIOR_STEPS, seed=5):
    """The same model through annotations.update_bayesc_binary_priors on numpy's generator, the variance held fixed."""
    from jwas_jl_amd import annotations as A_
    rng = np.random.default_rng(seed)
    ann = A_.MarkerAnnotations(case["D"].copy(), variance=POSTERIOR_VARIANCE)
    ann.mu = ann.design_matrix @ ann.coefficients
    chain = np.empty((steps, 3))
    for it in range(steps):
        A_.update_bayesc_binary_priors(ann, case["delta"], rng)
        ann.variance = POSTERIOR_VARIANCE
        chain[it] = ann.coefficients
    return chain
