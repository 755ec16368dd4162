"""TEST INFRASTRUCTURE: a numpy restatement of the device's location-parameter step (csrc/locpar.hpp) on the same Philox counters,
and stand-in engines that add the locpar methods of HipEngine to OracleEngine / OracleEngine64.

For level l of a term of trait k (c = inv(R); one trait: c = 1), d_l = sum_{i in l} w_i x_i^2:
    rho_i  = sum_m c_km r_m,i
    S_l    = sum_{i in l} w_i x_i rho_i
    lhs_l  = d_l c_kk + prior              prior = vare Gi (one trait), Gi_kk (several traits), 0 (fixed)
    mean_l = (S_l + d_l c_kk sol_l - sum_{m != k} Gi_km u_m,l) / lhs_l
    sol_l' = mean_l + z sqrt(s / lhs_l)    s = vare (one trait), 1 (several); lhs_l == 0: the level is left alone
    r_k,i  = T(double(r_k,i) - x_i (sol_l' - sol_l))
z = sqrt(-2 ln u1) cos(2 pi u2) from philox(level, iteration, 0x20000000 | term ordinal, 3 + 16 trait): u1 from words (1, 0), u2 from
words (3, 2).  The sums run in numpy's order (np.bincount: ascending record), the device's in the order of its term layout: the two
differ by the rounding of a reordered sum of the same doubles, which tests/test_gpu_locpar.py bounds.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine, OracleEngine64  # noqa: E402
from liability_reference import philox4x32_10  # noqa: E402

MAX_GROUPS = 8


def _u52(lo, hi):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def locpar_normal(levels, iteration, term, trait, seed):
    """The device's normal of every level of term `term` (its ordinal in the order added)."""
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(np.asarray(levels, dtype=np.uint64), np.uint64(iteration), np.uint64(0x20000000 | int(term)),
                                   np.uint64(3 + 16 * int(trait)), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(6.283185307179586476925286766559 * _u52(w2, w3))


class Term:
    def __init__(self, trait, x, level, nlevels, group, pos, off, w):
        self.trait, self.nlevels, self.group, self.pos, self.off = int(trait), int(nlevels), int(group), int(pos), int(off)
        n = len(w)
        self.x = np.ones(n) if x is None else np.asarray(x, dtype=np.float64).copy()
        self.level = np.zeros(n, dtype=np.int64) if level is None else np.asarray(level, dtype=np.int64).copy()
        self.inl = self.level >= 0
        self.wx = w * self.x
        self.d = np.bincount(self.level[self.inl], weights=(self.wx * self.x)[self.inl], minlength=self.nlevels)


def term_draw(T, ordinal, r, sol, partner_offs, gi_row, *, iteration, seed, vare, Rinv, normals=None):
    """The new values of term T from the residuals r (t x n doubles) and the solution vector.  Returns (new, detail): detail holds
    what the bound of the GPU test is built from (S, lhs, mean, sd and the sum of absolute terms A)."""
    t = r.shape[0]
    k = T.trait
    c = np.ones(1) if t == 1 else np.asarray(Rinv, dtype=np.float64).reshape(t, t)[k]
    rho = r[0] if t == 1 else sum(c[m] * r[m] for m in range(t))
    absrho = np.abs(r[0]) if t == 1 else sum(np.abs(c[m] * r[m]) for m in range(t))
    lv = T.level[T.inl]
    S = np.bincount(lv, weights=(T.wx * rho)[T.inl], minlength=T.nlevels)
    A = np.bincount(lv, weights=(np.abs(T.wx) * absrho)[T.inl], minlength=T.nlevels)
    ckk = 1.0 if t == 1 else c[k]
    s = float(vare) if t == 1 else 1.0
    old = sol[T.off:T.off + T.nlevels]
    prior = 0.0
    num = S + T.d * ckk * old
    A = A + np.abs(T.d * ckk * old)
    if T.group >= 0:
        prior = float(vare) * gi_row[T.pos] if t == 1 else gi_row[T.pos]
        for m, po in enumerate(partner_offs):
            if m != T.pos:
                um = sol[po:po + T.nlevels]
                num = num - gi_row[m] * um
                A = A + np.abs(gi_row[m] * um)
    lhs = T.d * ckk + prior
    live = lhs != 0.0
    safe = np.where(live, lhs, 1.0)
    mean = num / safe
    sd = np.sqrt(s / safe)
    z = locpar_normal(np.arange(T.nlevels), iteration, ordinal, k, seed) if normals is None else normals
    new = np.where(live, mean + z * sd, old)
    return new, {"S": S, "A": A, "lhs": lhs, "mean": mean, "sd": sd, "live": live, "n_l": np.bincount(lv, minlength=T.nlevels), "z": z}


def term_apply(T, r_k, delta, dtype):
    """r_k,i = T(double(r_k,i) - x_i delta[level_i]) for the records in a level whose delta is not zero."""
    out = r_k.copy()
    dl = np.where(T.inl, delta[np.maximum(T.level, 0)], 0.0)
    touch = T.inl & (dl != 0.0)
    out[touch] = (r_k[touch].astype(np.float64) - T.x[touch] * dl[touch]).astype(dtype)
    return out


class _LocparMixin:
    """The locpar methods of HipEngine on an engine that keeps its residuals in self.r (t x n)."""

    @staticmethod
    def locpar_estimate_bytes(n, nterms, total_levels):
        return int(nterms) * (24 * int(n) + 12 * (int(n) // 1024 + 2)) + int(total_levels) * 56 + 8 * MAX_GROUPS * 16 * 3

    def _locpar_weights(self):
        w = getattr(self, "_rinv", None) if isinstance(self, OracleEngine) else getattr(self, "_w", None)
        return np.ones(self.n) if w is None or callable(w) else np.asarray(w, dtype=np.float64)

    def locpar_begin(self, ntraits=None):
        t = self.ntraits if ntraits is None else int(ntraits)
        if t != self.ntraits:
            raise ValueError("ntraits differs from init_state's")
        self._lp_terms, self._lp_groups, self._lp_q, self._lp_final = [], {}, 0, False
        self._lp_w = self._locpar_weights()

    def _lp_add(self, trait, x, level, nlevels, group):
        if self._lp_final:
            raise ValueError("terms are added before sol is first used")
        if not 0 <= int(trait) < self.ntraits:
            raise ValueError("trait outside the model")
        pos = 0
        if group >= 0:
            members = self._lp_groups.setdefault(group, [])
            if any(self._lp_terms[j].trait == trait for j in members):
                raise NotImplementedError("correlated terms within a trait stay on the reference")
            if members and self._lp_terms[members[0]].nlevels != nlevels:
                raise ValueError("the member terms of a random effect must have the same levels")
            pos = len(members)
            members.append(len(self._lp_terms))
        self._lp_terms.append(Term(trait, x, level, nlevels, group, pos, self._lp_q, self._lp_w))
        self._lp_q += int(nlevels)

    def locpar_add_covariate(self, trait, x=None):
        if x is not None and (len(x) != self.n or not np.all(np.isfinite(x))):
            raise ValueError("the covariate must hold n finite values")
        self._lp_add(int(trait), x, None, 1, -1)

    def locpar_add_factor(self, trait, level, nlevels, random_group=-1):
        lv = np.asarray(level)
        if len(lv) != self.n or lv.min() < -1 or lv.max() >= nlevels:
            raise ValueError("levels outside -1 .. nlevels - 1")
        if not -1 <= random_group < MAX_GROUPS:
            raise ValueError("random_group outside -1 .. 7")
        self._lp_add(int(trait), None, lv, int(nlevels), int(random_group))

    def _lp_finalize(self):
        if not self._lp_final:
            self._lp_sol = np.zeros(self._lp_q)
            self._lp_mean, self._lp_mean2 = np.zeros(self._lp_q), np.zeros(self._lp_q)
            self._lp_final = True

    def locpar_size(self):
        return self._lp_q

    def locpar_set_sol(self, sol):
        self._lp_finalize()
        sol = np.asarray(sol, dtype=np.float64)
        if sol.shape != (self._lp_q,):
            raise ValueError("q differs from the number of location parameters")
        self._lp_sol = sol.copy()

    def locpar_get_sol(self):
        self._lp_finalize()
        return self._lp_sol.copy()

    def locpar_step(self, *, iteration, seed, vare=None, Rinv=None, Gi=(), first_term=0, last_term=-1, details=None):
        t = self.ntraits
        nterms = len(self._lp_terms)
        last = nterms if last_term < 0 else int(last_term)
        if int(iteration) < 1:
            raise ValueError("iteration must be >= 1")
        if not 0 <= first_term <= last <= nterms:
            raise ValueError("terms outside the scan")
        if t == 1 and not (vare is not None and np.isfinite(vare) and vare > 0):
            raise ValueError("vare must be positive and finite")
        if len(Gi) != len(self._lp_groups):
            raise ValueError("Gi must hold one matrix per random effect")
        Gi = [np.atleast_2d(np.asarray(M, dtype=np.float64)) for M in Gi]
        self._lp_finalize()
        for j in range(first_term, last):
            T = self._lp_terms[j]
            offs, row = (), None
            if T.group >= 0:
                offs = [self._lp_terms[m].off for m in self._lp_groups[T.group]]
                row = Gi[T.group][T.pos]
            r64 = self.r.astype(np.float64)
            new, det = term_draw(T, j, r64, self._lp_sol, offs, row, iteration=iteration, seed=seed, vare=vare, Rinv=Rinv)
            delta = new - self._lp_sol[T.off:T.off + T.nlevels]
            self._lp_sol[T.off:T.off + T.nlevels] = new
            self.r[T.trait] = term_apply(T, self.r[T.trait], delta, self.r.dtype)
            if details is not None:
                det["delta"] = delta
                details.append(det)
        utu = []
        for g in sorted(self._lp_groups):
            U = np.stack([self._lp_sol[self._lp_terms[m].off:self._lp_terms[m].off + self._lp_terms[m].nlevels] for m in self._lp_groups[g]])
            utu.append(U @ U.T)
        return {"utu": utu, "step_ms": 0.0}

    def locpar_accumulate(self, nsamples):
        self._lp_finalize()
        self._lp_mean += (self._lp_sol - self._lp_mean) / nsamples
        self._lp_mean2 += (self._lp_sol ** 2 - self._lp_mean2) / nsamples

    def locpar_get_means(self):
        self._lp_finalize()
        return self._lp_mean.copy(), self._lp_mean2.copy()

    def locpar_end(self):
        self._lp_terms = None


from liability_reference import _LiabilityMixin  # noqa: E402


class LocparOracleEngine(_LocparMixin, _LiabilityMixin, OracleEngine):
    pass


class LocparOracleEngine64(_LocparMixin, _LiabilityMixin, OracleEngine64):
    pass


def dense_mme(terms, groups, w, r, sol, *, vare=None, Rinv=None, Gi=()):
    """A and b of the mixed model equations (build_MME.jl:339, MCMC_BayesianAlphabet.jl:211; random_effects.jl:219-240), densely:
    A = X' Ri X + prior, b = X' Ri (r + X sol), Ri = kron(inv(R), diag(w)) (one trait: diag(w), the lambda form)."""
    t, n = r.shape
    q = sum(T.nlevels for T in terms)
    X = [np.zeros((n, q)) for _ in range(t)]        # X[k]: the columns of trait k's terms (zero elsewhere)
    for T in terms:
        rows = np.flatnonzero(T.inl)
        X[T.trait][rows, T.off + T.level[rows]] = T.x[rows]
    c = np.ones((1, 1)) if t == 1 else np.asarray(Rinv, dtype=np.float64).reshape(t, t)
    ycorr = [r[k] + X[k] @ sol for k in range(t)]
    A = sum(c[k, m] * (X[k].T @ (w[:, None] * X[m])) for k in range(t) for m in range(t))
    b = sum(c[k, m] * (X[k].T @ (w * ycorr[m])) for k in range(t) for m in range(t))
    for g, members in groups.items():
        G = np.atleast_2d(np.asarray(Gi[g], dtype=np.float64))
        for a, ja in enumerate(members):
            for e, je in enumerate(members):
                Ta, Te = terms[ja], terms[je]
                A[Ta.off:Ta.off + Ta.nlevels, Te.off:Te.off + Te.nlevels] += np.eye(Ta.nlevels) * (G[a, e] * (vare if t == 1 else 1.0))
    return A, b


def reference_scan(A, x, b, z, vare=None):
    """Gibbs(A, x, b[, vare]) of iterative_solver/solver.jl:143-162 fed the normals z (one per equation)."""
    x = x.copy()
    for i in range(len(x)):
        if A[i, i] != 0.0:
            invlhs = 1.0 / A[i, i]
            mu = invlhs * (b[i] - A[:, i] @ x) + x[i]
            x[i] = z[i] * np.sqrt(invlhs * (vare if vare is not None else 1.0)) + mu
    return x


# ---- the exact-posterior case shared by tests/test_locpar_host.py and tests/test_gpu_locpar.py --------------------------------
POSTERIOR_STEPS, POSTERIOR_BATCHES = 4000, 40
POSTERIOR_SEED = 7


def posterior_case():
    """n = 403 records, one trait: intercept, a covariate and a 9-level random factor; the variances are fixed, so the step alone
    is a Gibbs sampler on a Gaussian whose mean solves the mixed model equations."""
    rng = np.random.default_rng(403)
    n = 403
    x = rng.standard_normal(n)
    lev = rng.integers(0, 9, n).astype(np.int32)
    u = rng.standard_normal(9) * 0.7
    y = 1.5 + 0.8 * x + u[lev] + rng.standard_normal(n)
    return {"n": n, "x": x, "level": lev, "nlevels": 9, "y": y, "vare": 1.0, "Gi": [np.array([[2.0]])],
            "X": rng.standard_normal((n, 8))}


def posterior_z(engine, case, seed=POSTERIOR_SEED):
    """Run POSTERIOR_STEPS steps on `engine` (loaded and initialised by the caller: one trait, residual = y, the three terms
    added) and return |chain mean - solve| in batch-means standard errors (POSTERIOR_BATCHES batches) for every entry of sol."""
    terms = [Term(0, None, None, 1, -1, 0, 0, np.ones(case["n"])), Term(0, case["x"], None, 1, -1, 0, 1, np.ones(case["n"])),
             Term(0, None, case["level"], case["nlevels"], 0, 0, 2, np.ones(case["n"]))]
    A, b = dense_mme(terms, {0: [2]}, np.ones(case["n"]), case["y"][None, :].astype(np.float64), np.zeros(11), vare=case["vare"], Gi=case["Gi"])
    solve = np.linalg.solve(A, b)
    chain = np.empty((POSTERIOR_STEPS, 11))
    for it in range(1, POSTERIOR_STEPS + 1):
        engine.locpar_step(iteration=it, seed=seed, vare=case["vare"], Gi=case["Gi"])
        chain[it - 1] = engine.locpar_get_sol()
    bm = chain.reshape(POSTERIOR_BATCHES, -1, 11).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / np.sqrt(POSTERIOR_BATCHES)
    return np.abs(chain.mean(axis=0) - solve) / se


def posterior_engine(engine, case):
    engine.load_dense(case["X"])
    engine.setup_blocks(8 if not hasattr(engine, "_L") else 64, "f64")
    engine.init_state("BayesC", 1)
    engine.set_residual(case["y"].astype(engine.get_residual(0).dtype), 0)
    engine.locpar_begin(1)
    engine.locpar_add_covariate(0, None)
    engine.locpar_add_covariate(0, case["x"])
    engine.locpar_add_factor(0, case["level"], case["nlevels"], 0)
    return engine
