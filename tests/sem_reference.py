"""TEST INFRASTRUCTURE: a numpy restatement of the device's structural-equation-model step (csrc/sem.hpp) on the same Philox
counters, and stand-in engines that add the sem methods of HipEngine to OracleEngine, OracleEngine64 and LocparOracleEngine*.

t traits, y (t x n) the constant phenotypes, cs the strictly lower 0/1 causal structure (cs[i, j] = 1: trait j acts on trait i),
P_i the parents of trait i ascending.  The residual is r_i = y_i - sum_{j in P_i} lambda_ij y_j - fitted_i.  One step, for every
trait i with parents:
    S     = y y'
    C_ji  = y_j'r_i                                j in P_i
    rhs   = (C_{P_i,i} + S_{P_i P_i} lambda_i,old) / R_ii
    F     = S_{P_i P_i} / R_ii + I,   F = L L',   mu = inv(F) rhs,   lambda_i,new = mu + inv(L') z
    r_i,n = T(((double(r_i,n) + d_1 y_j1,n) + d_2 y_j2,n) + ...)          d = lambda_old - lambda_new, parents ascending
z_q = sqrt(-2 ln u1) cos(2 pi u2) from philox(q, iteration, 0x04000000 | i, 7): u1 from words (1, 0), u2 from words (3, 2).
The sums run in numpy's order, the device's in the order of its grid: the two differ by the rounding of a reordered sum of the
same doubles, which tests/test_gpu_sem.py bounds.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine, OracleEngine64  # noqa: E402
from liability_reference import philox4x32_10  # noqa: E402
from locpar_reference import LocparOracleEngine, LocparOracleEngine64, _u52  # noqa: E402

SEM_TAG, SEM_SLOT = 0x04000000, 7
MAX_TRAITS = 4


def sem_normal(nparents, iteration, trait, seed):
    """The device's normals of the parents 0 .. nparents - 1 (their ordinals among the parents) of trait `trait`."""
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(np.arange(nparents, dtype=np.uint64), np.uint64(iteration), np.uint64(SEM_TAG | int(trait)),
                                   np.uint64(SEM_SLOT), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(6.283185307179586476925286766559 * _u52(w2, w3))


def parents(cs):
    cs = np.asarray(cs)
    return [np.flatnonzero(cs[i, :i]) for i in range(cs.shape[0])]


def check_structure(cs, t):
    cs = np.asarray(cs)
    if t < 2:
        raise ValueError("Causal strutures are only allowed in multi-trait analysis")
    if cs.shape != (t, t) or not np.all((cs == 0) | (cs == 1)):
        raise ValueError("the causal structure must be a t x t matrix of 0 and 1")
    if np.any(np.triu(cs) != 0):
        raise ValueError("The causal structue needs to be a lower triangular matrix.")
    return cs.astype(np.int32)


def sem_draw(y, r64, cs, lam, R_diag, *, iteration, seed, S=None, normals=None):
    """The new coefficient matrix from the residuals r64 (t x n doubles) and the old coefficients.  Returns (new, detail): detail
    holds, per trait with parents, what the bounds of the GPU test are built from."""
    t = y.shape[0]
    S = y @ y.T if S is None else S
    new = np.array(lam, dtype=np.float64, copy=True)
    C, mu_m, detail = np.zeros((t, t)), np.zeros((t, t)), {}
    for i, P in enumerate(parents(cs)):
        if P.size == 0:
            continue
        Rii = float(R_diag[i])
        Ci = y[P] @ r64[i]
        absC = np.abs(y[P]) @ np.abs(r64[i])
        Spp = S[np.ix_(P, P)]
        old = new[i, P].copy()
        rhs = (Ci + Spp @ old) / Rii
        F = Spp / Rii + np.eye(P.size)
        L = np.linalg.cholesky(F)
        mu = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        z = sem_normal(P.size, iteration, i, seed) if normals is None else np.asarray(normals[i], dtype=np.float64)
        x = np.linalg.solve(L.T, z)
        new[i, P] = mu + x
        C[i, P], mu_m[i, P] = Ci, mu
        detail[i] = {"P": P, "C": Ci, "absC": absC, "S": Spp, "old": old, "rhs": rhs, "F": F, "L": L, "mu": mu, "z": z, "R": Rii}
    return new, {"C": C, "mu": mu_m, "traits": detail}


def sem_apply(r, y, cs, d):
    """r_i,n = T(((double(r_i,n) + d_1 y_j1,n) + d_2 y_j2,n) + ...), parents ascending; traits without parents are not touched."""
    out = r.copy()
    for i, P in enumerate(parents(cs)):
        if P.size == 0:
            continue
        v = r[i].astype(np.float64)
        for j in P:
            v = v + d[i, j] * y[j]
        out[i] = v.astype(r.dtype)
    return out


def indirect_matrix(lam):
    """K = sum_{m=1}^{t-1} Lambda^m (compute_indirect_effect, SEM.jl:245-252)."""
    lam = np.asarray(lam, dtype=np.float64)
    K, P = np.zeros_like(lam), np.eye(lam.shape[0])
    for _ in range(lam.shape[0] - 1):
        P = P @ lam
        K = K + P
    return K


def indirect_overall(K, alpha):
    """indirect_k = sum_j K[k, j] alpha_j (j ascending, from 0), overall_k = alpha_k + indirect_k; alpha t x p doubles."""
    t = alpha.shape[0]
    ind = np.zeros_like(alpha)
    for k in range(t):
        for j in range(t):
            ind[k] = ind[k] + K[k, j] * alpha[j]
    return ind, alpha + ind


class _SemMixin:
    """The sem methods of HipEngine on an engine that keeps its residuals in self.r (t x n) and its effects in self.alpha."""

    @staticmethod
    def sem_estimate_bytes(n, p, ntraits):
        t = max(int(ntraits), 1)
        return 8 * (t * int(n) + 6 * t * int(p) + 512 * 10 + 16 + 64)

    def sem_begin(self, y, structure):
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 2 or y.shape != (self.ntraits, self.n):
            raise ValueError("y must be ntraits x n")
        if not np.all(np.isfinite(y)):
            raise ValueError("the phenotypes must be finite")
        self._sem_cs = check_structure(structure, self.ntraits)
        self._sem_y = y.copy()
        self._sem_S = y @ y.T
        self._sem_lam = np.zeros((self.ntraits, self.ntraits))
        self._sem_acc = {kind: [np.zeros((self.ntraits, self.p)) for _ in range(3)] for kind in ("indirect", "overall")}

    def _sem_need(self):
        if getattr(self, "_sem_cs", None) is None:
            raise ValueError("sem_begin has not been called")

    def sem_step(self, *, iteration, seed, R_diag, details=None):
        self._sem_need()
        R_diag = np.asarray(R_diag, dtype=np.float64).reshape(-1)
        if int(iteration) < 1:
            raise ValueError("iteration must be >= 1")
        if R_diag.shape != (self.ntraits,) or not np.all(np.isfinite(R_diag) & (R_diag > 0)):
            raise ValueError("R_diag must be positive and finite")
        new, det = sem_draw(self._sem_y, self.r.astype(np.float64), self._sem_cs, self._sem_lam, R_diag, iteration=iteration, seed=seed,
                            S=self._sem_S)
        d = self._sem_lam - new
        self.r[...] = sem_apply(self.r, self._sem_y, self._sem_cs, d)
        self._sem_lam = new
        if details is not None:
            det["d"] = d
            details.append(det)
        return {"lambda": new.copy(), "mean": det["mu"], "ypr": det["C"], "step_ms": 0.0}

    def sem_get_lambda(self):
        self._sem_need()
        return self._sem_lam.copy()

    def sem_set_lambda(self, lam):
        self._sem_need()
        lam = np.asarray(lam, dtype=np.float64)
        if lam.shape != self._sem_lam.shape or not np.all(np.isfinite(lam)) or np.any(lam[self._sem_cs == 0] != 0.0):
            raise ValueError("lambda must be finite, t x t and zero outside the structure")
        self._sem_lam = lam.copy()

    def sem_get_gram(self):
        self._sem_need()
        return self._sem_S.copy()

    def sem_accumulate(self, K, nsamples):
        self._sem_need()
        K = np.asarray(K, dtype=np.float64)
        if K.shape != self._sem_lam.shape or not np.all(np.isfinite(K)) or not nsamples >= 1:
            raise ValueError("K must be finite and t x t, nsamples >= 1")
        ind, ov = indirect_overall(K, np.asarray(self.alpha, dtype=np.float64))
        for kind, v in (("indirect", ind), ("overall", ov)):
            m, m2, f = self._sem_acc[kind]
            m += (v - m) / nsamples
            m2 += (v * v - m2) / nsamples
            f += ((v != 0.0).astype(np.float64) - f) / nsamples

    def sem_get_effects(self, kind, trait):
        self._sem_need()
        return tuple(a[trait].copy() for a in self._sem_acc[kind])

    def sem_end(self):
        self._sem_need()
        self._sem_cs = None


class SemOracleEngine(_SemMixin, OracleEngine):
    pass


class SemOracleEngine64(_SemMixin, OracleEngine64):
    pass


class SemLocparOracleEngine(_SemMixin, LocparOracleEngine):
    pass


class SemLocparOracleEngine64(_SemMixin, LocparOracleEngine64):
    pass


# ---- the exact-conditional case shared by tests/test_sem_host.py and tests/test_gpu_sem.py ---------------------------------------
CONDITIONAL_STEPS = 4000
CONDITIONAL_SEED = 11


def conditional_case():
    """n = 403 records, three traits, the full structure.  With everything else held fixed -- the plain residual e_i = r_i +
    sum lambda_ij y_j does not depend on lambda -- every step draws lambda_i from the same N(mu_i, inv(F_i)), independently from
    step to step (the Philox counter changes with the iteration)."""
    rng = np.random.default_rng(403)
    n = 403
    y = np.empty((3, n))
    y[0] = 1.0 + rng.standard_normal(n)
    y[1] = 0.5 + 0.6 * y[0] + 0.8 * rng.standard_normal(n)
    y[2] = -0.2 + 0.3 * y[0] - 0.5 * y[1] + 0.7 * rng.standard_normal(n)
    fitted = 0.3 * rng.standard_normal((3, n))
    return {"n": n, "y": y, "cs": np.tril(np.ones((3, 3), dtype=np.int32), -1), "e": y - fitted, "R_diag": np.array([1.1, 0.8, 0.6]),
            "X": rng.standard_normal((n, 8))}


def conditional_engine(engine, case):
    engine.load_dense(case["X"])
    engine.setup_blocks(8 if not hasattr(engine, "_L") else 64, "f64")
    engine.init_state("MTBayesC", 3)
    for k in range(3):
        engine.set_residual(case["e"][k].astype(engine.get_residual(k).dtype), k)       # lambda = 0: r = e
    engine.sem_begin(case["y"], case["cs"])
    return engine


def conditional_moments(case):
    """(mu, V) of every trait with parents: the exact conditional N(mu_i, inv(F_i))."""
    y, e, out = case["y"], case["e"], {}
    for i, P in enumerate(parents(case["cs"])):
        if P.size:
            F = y[P] @ y[P].T / case["R_diag"][i] + np.eye(P.size)
            V = np.linalg.inv(F)
            out[i] = (P, V @ (y[P] @ e[i] / case["R_diag"][i]), V)
    return out


def conditional_check(engine, case, seed=CONDITIONAL_SEED, steps=CONDITIONAL_STEPS):
    """Run `steps` steps and return [(trait, parent, |mean - mu| / (sqrt(V_kk / N)), |var - V_kk| / (V_kk sqrt(2 / (N - 1))))]:
    both figures must be <= 5."""
    draws = np.empty((steps, 3, 3))
    for it in range(1, steps + 1):
        draws[it - 1] = engine.sem_step(iteration=it, seed=seed, R_diag=case["R_diag"])["lambda"]
    rows = []
    for i, (P, mu, V) in conditional_moments(case).items():
        for q, j in enumerate(P):
            x = draws[:, i, j]
            rows.append((i, int(j), abs(x.mean() - mu[q]) / np.sqrt(V[q, q] / steps),
                         abs(x.var(ddof=1) - V[q, q]) / (V[q, q] * np.sqrt(2.0 / (steps - 1)))))
    return rows


# ---- runMCMC cases shared by the host and the GPU tests -----------------------------------------------------------------------------
def sem_phenotypes(small_data, traits, nmarkers=None):
    """(genotype frame, phenotype frame): recursive traits built from small_data's y -- every trait is driven by the one before
    it (coefficient 0.5) and, from the third on, by the first (-0.3)."""
    import pandas as pd
    n, p = small_data["raw"].shape
    p = p if nmarkers is None else int(nmarkers)
    rng = np.random.default_rng(37)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(small_data["raw"][:, :p].astype(np.float64), columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    ph = pd.DataFrame({"ID": ids, "age": rng.uniform(1, 5, n), "weights": rng.uniform(0.5, 2.0, n)})
    y = small_data["y"].astype(np.float64)
    cols = []
    for k, tr in enumerate(traits):
        v = (1.0 - 0.2 * k) * y + 0.5 * rng.standard_normal(n)
        if k >= 1:
            v = v + 0.5 * cols[k - 1]
        if k >= 2:
            v = v - 0.3 * cols[0]
        cols.append(v)
        ph[tr] = v
    return gdf, ph
