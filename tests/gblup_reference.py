"""TEST INFRASTRUCTURE: numpy Float64 restatements of the device's relationship matrix and GBLUP step (csrc/gblup.hpp) on the same
Philox counters, stand-in engines with grm and the gblup_* methods of HipEngine on the oracle stand-ins, and the closed-form
posterior of y = intercept + a + e.  The package never imports this file.

    K = (Z Z' + 1e-5 I) / p,  Z = X ./ divisor (divided in X's precision: the device's Z bit for bit)
One step (GBLUP!, megaGBLUP!, MTGBLUP!; markers/BayesianAlphabet/GBLUP.jl), L the eigenvectors, D the eigenvalues, T traits:
    r+_k = T(r_k + L alpha_k);  s_ik = l_i' r+_k
    diagonal:  lhs = 1 + vare_kk / (G_kk D_i),  alpha_ik = s_ik / lhs + z sqrt(vare_kk / lhs)
    joint:     lhs_i = inv(vare) + inv(G) / D_i,  S = inv(lhs_i),  alpha_i = S inv(vare) s_i + chol_lower(S) z_i
    r_k = T(r+_k - L alpha_k)                (T: one rounding to the element type)
z of coefficient q of pseudo-marker i: Box-Muller of philox(i, iteration, 0x03000000, 13 + 16 q).  The O(n) sums run in numpy's order,
the device's in its grid's: where the two are compared the tests carry a rounding bound; where bits are compared both sides are the
device.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from liability_reference import philox4x32_10  # noqa: E402
from locpar_reference import LocparOracleEngine, LocparOracleEngine64  # noqa: E402

GBLUP_TAG, SLOT_Z = 0x03000000, 13
TWO_PI = 6.283185307179586476925286766559
U = 2.0 ** -53


def _u52(lo, hi):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def gblup_normal(index, iteration, seed, q):
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(np.asarray(index, dtype=np.uint64), np.uint64(iteration), np.uint64(GBLUP_TAG), np.uint64(SLOT_Z + 16 * int(q)),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.sqrt(-2.0 * np.log(_u52(w0, w1))) * np.cos(TWO_PI * _u52(w2, w3))


def draws(n, T, iteration, seed, first_trait=0):
    """z [n, T] of one step."""
    return np.stack([gblup_normal(np.arange(n), iteration, seed, first_trait + q) for q in range(T)], axis=1)


# ---- the relationship matrix ----------------------------------------------------------------------------------------------------------
def grm_z(X, divisor):
    X = np.asarray(X)
    return X / np.asarray(divisor, dtype=X.dtype)[None, :]          # (IEEE division in X's precision)


def grm_reference(X, divisor):
    """(K in double from the same Z, the bound's sum_k |z_ik z_jk|)."""
    Z = grm_z(X, divisor).astype(np.float64)
    p = Z.shape[1]
    return (Z @ Z.T + 1e-5 * np.eye(len(Z))) / p, np.abs(Z) @ np.abs(Z).T


def grm_bound(absZZ, p, dtype, chunk):
    """Float32: chunks of `chunk` markers are fp32 fma chains (chunk roundings), folded in double; + 1e-5 and / p are two more.
    Float64: one chain of p roundings and the same two."""
    if np.dtype(dtype) == np.float32:
        return (chunk + 2) * 2.0 ** -24 * (absZZ + 1e-5) / p
    return (p + 2) * 2.0 ** -53 * (absZZ + 1e-5) / p


# ---- one step ---------------------------------------------------------------------------------------------------------------------------
def inv_small(A):
    """Gauss-Jordan with partial pivoting in double: the operation order of csrc/ctx.hpp's inv_small."""
    t = len(A)
    M = np.hstack([np.array(A, dtype=np.float64), np.eye(t)])
    for c in range(t):
        piv = c
        for i in range(c + 1, t):
            if abs(M[i, c]) > abs(M[piv, c]):
                piv = i
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for i in range(t):
            if i != c and M[i, c] != 0.0:
                M[i] = M[i] - M[i, c] * M[c]
    return M[:, t:].copy()


def chol_lower(A):
    t = len(A)
    C = np.zeros((t, t))
    for a in range(t):
        for b in range(a + 1):
            s = A[a, b]
            for k in range(b):
                s = s - C[a, k] * C[b, k]
            C[a, b] = np.sqrt(s) if a == b else s / C[b, b]
    return C


def sample_from_rhs(s, D, z, vare, G, diagonal):
    """alpha [n, T] (double, before the store's rounding) and, per pseudo-marker, what the tests' bounds and laws read:
    {"mean", "sd"} (diagonal) or {"mean", "C", "S", "lhs", "w"} (joint)."""
    s, z = np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64)
    n, T = s.shape
    vare, G = np.asarray(vare, dtype=np.float64).reshape(T, T), np.asarray(G, dtype=np.float64).reshape(T, T)
    if diagonal or T == 1:
        ve, g = np.diag(vare)[None, :], np.diag(G)[None, :]
        lhs = 1.0 + ve / (g * D[:, None])
        mean, sd = s / lhs, np.sqrt(ve / lhs)
        return mean + z * sd, {"mean": mean, "sd": sd}
    Rinv, Ginv = inv_small(vare), inv_small(G)
    alpha = np.zeros((n, T))
    info = {"mean": np.zeros((n, T)), "C": np.zeros((n, T, T)), "S": np.zeros((n, T, T)), "lhs": np.zeros((n, T, T)), "w": np.zeros((n, T))}
    for i in range(n):
        lhs = Rinv + Ginv / D[i]
        w = np.array([sum(Rinv[k, l] * s[i, l] for l in range(T)) for k in range(T)])
        S = inv_small(lhs)
        C = chol_lower(S)
        for k in range(T):
            mu = 0.0
            for l in range(T):
                mu = mu + S[k, l] * w[l]
            info["mean"][i, k] = mu
            for l in range(k + 1):
                mu = mu + C[k, l] * z[i, l]
            alpha[i, k] = mu
        info["C"][i], info["S"][i], info["lhs"][i], info["w"][i] = C, S, lhs, w
    return alpha, info


def alpha_bound(s, D, z, vare, G, diagonal, dtype):
    """|alpha_device - restatement| evaluated from the device's own s.  Both sides run the same operations on the same doubles: they
    differ by the libm behind Box-Muller (2^-46 times the factor that multiplies z: the argument of tests/test_gpu_sem.py and
    mega_reference.marker_bound), a few ulp of the solve -- bounded by twice the first-order bound of a solve perturbed by (T + 2) u --
    and the store's rounding to the element type."""
    alpha, info = sample_from_rhs(s, D, z, vare, G, diagonal)
    ur = 2.0 ** -24 if np.dtype(dtype) == np.float32 else U
    if "sd" in info:
        b = 4 * U * np.abs(info["mean"]) + (2.0 ** -46 + 4 * U * np.abs(z)) * info["sd"]
    else:
        T = s.shape[1]
        absS, absC = np.abs(info["S"]), np.abs(info["C"])
        cond = np.abs(info["lhs"]).sum(axis=2).max(axis=1) * absS.sum(axis=2).max(axis=1)
        b = 2 * (T + 2) * U * cond[:, None] * np.einsum("ikl,il->ik", absS, np.abs(info["w"]))
        b = b + 2.0 ** -46 * absC.sum(axis=2) + 4 * U * (T + 2) * cond[:, None] * np.einsum("ikl,il->ik", absC, np.abs(z))
    return alpha, b + ur * np.abs(alpha), info


def step_reference(L, D, r, alpha, *, iteration, seed, vare, G, diagonal, dtype, first_trait=0):
    """One step from (r [T, n], alpha [T, n]) in the element type `dtype`.  Returns a dict: rplus, s, alpha, r (element type where
    the device stores it), alpha_ss, resid_ss, resid_sum."""
    L64, D = np.asarray(L, dtype=np.float64), np.asarray(D, dtype=np.float64)
    r, alpha = np.asarray(r, dtype=dtype), np.asarray(alpha, dtype=dtype)
    T, n = r.shape
    rplus = (r.astype(np.float64) + alpha.astype(np.float64) @ L64.T).astype(dtype)
    s = (rplus.astype(np.float64) @ L64).T                         # [n, T]
    a64, _ = sample_from_rhs(s, D, draws(n, T, iteration, seed, first_trait), vare, G, diagonal)
    anew = a64.T.astype(dtype)
    rnew = (rplus.astype(np.float64) - anew.astype(np.float64) @ L64.T).astype(dtype)
    a_, r_ = anew.astype(np.float64), rnew.astype(np.float64)
    return {"rplus": rplus, "s": s, "alpha": anew, "r": rnew, "alpha_ss": (a_ / D[None, :]) @ a_.T, "resid_ss": r_ @ r_.T, "resid_sum": r_.sum(axis=1)}


# ---- stand-in engines ------------------------------------------------------------------------------------------------------------------
class _GblupMixin:
    """grm and the gblup_* methods of HipEngine on the restatements above; the residual and the effects are the stand-in's own."""
    GRM_CHUNK = 64

    def grm(self, divisor):
        dt = np.float64 if getattr(self, "precision", 32) == 64 else np.float32
        X = np.asarray(self.X, dtype=dt)
        d = np.asarray(divisor, dtype=dt)
        if d.shape != (self.p,) or not np.all(np.isfinite(d) & (d > 0)):
            raise ValueError("divisor must be positive and finite, one per marker")
        return grm_reference(X, d)[0].astype(dt)

    @staticmethod
    def gblup_estimate_bytes(n, ntraits=1, precision=32):
        return 8 * n * (2 + 8 * ntraits)

    def gblup_begin(self, D):
        D = np.asarray(D, dtype=np.float64)
        if self.n != self.p or D.shape != (self.p,) or not np.all(np.isfinite(D) & (D > 0)):
            raise ValueError("GBLUP needs the n x n matrix of eigenvectors and positive finite eigenvalues")
        if getattr(self, "alpha", None) is None:
            raise ValueError("init_state first")
        self._gb = {"D": D, "s": np.zeros((self.n, self.ntraits))}

    def gblup_step(self, *, iteration, seed, vare, G, diagonal=False, first_trait=0):
        gb = self._gb
        dt = self.r.dtype
        out = step_reference(self.X, gb["D"], self.r, self.alpha, iteration=iteration, seed=seed, vare=vare, G=G,
                             diagonal=bool(diagonal) or self.ntraits == 1, dtype=dt, first_trait=first_trait)
        self.r[...] = out["r"]
        self.alpha[...] = out["alpha"]
        self.beta[...] = out["alpha"]
        gb["s"] = out["s"]
        return {"alpha_ss": out["alpha_ss"], "resid_ss": out["resid_ss"], "resid_sum": out["resid_sum"], "step_ms": 0.0}

    def gblup_rhs(self):
        return self._gb["s"].copy()

    def gblup_end(self):
        self._gb = None


class GblupStandInEngine(_GblupMixin, LocparOracleEngine):
    precision = 32
    dtype = np.float32


class GblupStandInEngine64(_GblupMixin, LocparOracleEngine64):
    pass


# ---- the closed-form posterior -----------------------------------------------------------------------------------------------------------
def mme_posterior(Y, K, R, G):
    """y_k = 1 mu_k + a_k + e_k, vec(a) ~ N(0, G (x) K), vec(e) ~ N(0, R (x) I), flat prior on mu: the posterior of the breeding
    values is N(mean, cov) with [mu; a] ~ N(C^-1 W'Ri y, C^-1), C the coefficient matrix of the mixed-model equations.  Y: t x n.
    Returns (E a, E a a') with a trait-major (a[k n + i])."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    t, n = Y.shape
    R, G = np.asarray(R, dtype=np.float64).reshape(t, t), np.asarray(G, dtype=np.float64).reshape(t, t)
    Ri = np.kron(np.linalg.inv(R), np.eye(n))
    W = np.hstack([np.kron(np.eye(t), np.ones((n, 1))), np.eye(t * n)])
    C = W.T @ Ri @ W
    C[t:, t:] += np.kron(np.linalg.inv(G), np.linalg.inv(np.asarray(K, dtype=np.float64)))
    Ci = np.linalg.inv(C)
    mean = Ci @ (W.T @ Ri @ Y.reshape(-1))
    Ea, cov = mean[t:], Ci[t:, t:]
    return Ea, cov + np.outer(Ea, Ea)


def posterior_case(t, n, nmarkers=60, seed=5):
    """y = intercept + geno with a relationship matrix from `nmarkers` markers; both variances fixed."""
    rng = np.random.default_rng(seed)
    X = rng.binomial(2, 0.3 + 0.4 * rng.random(nmarkers), size=(n, nmarkers)).astype(np.float64)
    X = X[:, X.std(axis=0) > 0]
    pfreq = X.mean(axis=0) / 2
    Z = (X - X.mean(axis=0)) / np.sqrt(2 * pfreq * (1 - pfreq))
    K = (Z @ Z.T + 1e-5 * np.eye(n)) / Z.shape[1] + 0.05 * np.eye(n)      # (centred Z: the ridge keeps K well conditioned)
    if t == 1:
        G, R = np.array([[0.6]]), np.array([[0.4]])
    else:
        G, R = np.array([[0.6, 0.2], [0.2, 0.5]]), np.array([[0.4, -0.1], [-0.1, 0.5]])
    a = np.linalg.cholesky(np.kron(G, K)) @ rng.standard_normal(t * n)
    e = np.linalg.cholesky(np.kron(R, np.eye(n))) @ rng.standard_normal(t * n)
    Y = (1.0 + a + e).reshape(t, n)
    return {"K": K, "Y": Y, "G": G, "R": R, "ids": [f"a{i + 1}" for i in range(n)]}


def run_posterior_chain(api, case, engine, folder, *, double_precision, chain_length=20_500, burnin=500, seed=11):
    """The case through get_genotypes -> build_model -> runMCMC with fixed variances and location parameters on the device; returns
    the saved EBV samples [N, t n] (trait-major) computed from the saved pseudo-marker effects."""
    import pandas as pd
    K, Y, G, R = case["K"], case["Y"], case["G"], case["R"]
    t, n = Y.shape
    dt = np.float64 if double_precision else np.float32
    Kd = pd.DataFrame(K.astype(dt), columns=case["ids"])
    Kd.insert(0, "ID", case["ids"])
    traits = [f"y{k + 1}" for k in range(t)]
    geno = api.get_genotypes(Kd, G[0, 0] if t == 1 else G, method="GBLUP", estimate_variance=False, double_precision=double_precision)
    model = api.build_model("\n".join(f"{tr} = intercept + geno" for tr in traits), R[0, 0] if t == 1 else R, estimate_variance=False,
                            genotypes={"geno": geno})
    ph = pd.DataFrame({"ID": case["ids"], **{tr: Y[k] for k, tr in enumerate(traits)}})
    api.runMCMC(model, ph, chain_length=chain_length, burnin=burnin, output_samples_frequency=1, seed=seed, output_folder=folder,
                double_precision=double_precision, location_parameters="device", gblup_eigen="host", _engine=engine,
                output_samples_for_all_parameters=True)
    Kr = geno.genotypes.astype(dt)
    _, L = np.linalg.eigh(Kr)
    cols = []
    for tr in traits:
        a = np.loadtxt(os.path.join(folder, f"MCMC_samples_marker_effects_geno_{tr}.txt"), delimiter=",", skiprows=1, ndmin=2)
        cols.append(a @ L.astype(np.float64).T)
    return np.hstack(cols), geno
