"""Float64 restatement of the multi-trait samplers the Float64 device context runs beyond sampler I with one shared covariance:
_MTBayesABC_samplerII! (MTBayesABC.jl:129-210), sampler I / II with one t x t effect covariance per marker (multi-trait BayesA/B,
MTBayesABC.jl:66,86-90) and with marker-specific joint priors (MarkerSpecificPiPrior, :22-47), plus the per-marker
inverse-Wishart draw (variance_components.jl:181-186).  TEST INFRASTRUCTURE, plain numpy / Python floats.

The chain is the plain sequential block form of the reference (BayesABC_block! / MTBayesABC block sweep, :243-333; independent
blocks :190-255): per block the right-hand sides X_b'R^-1 r, then every marker in order (nreps passes), each change corrects
the block's right-hand sides through the block Gram, then the residual takes the block's changes.  With one pass per block this
is the literal per-marker chain up to the association of the sums.  Draws: the exported counter RNG (oracle.uniform /
oracle.normal / oracle.philox) on the slots of the Float32 path and the oracle (mt1_update / mt2_update,
orc_sample_marker_covariances in oracle/jwas_oracle.c), so this chain, the Float32 oracle and the device see the same draws.
The t x t algebra follows the oracle's operation order (Cholesky lhs = L L', M = L^-1, inv = M'M, det = prod L_ii^2)."""
import math

import numpy as np

import oracle as O
from oracle_engine import OracleEngine64, MTBAYESC1, MTBAYESC2, MTBAYESB1, MTBAYESB2

SAMPLER_I, SAMPLER_II = 1, 2


def _exp(x):
    return math.exp(x) if x < 709.0 else math.inf


def _log(x):
    return math.log(x) if x > 0.0 else (-math.inf if x == 0.0 else math.nan)


def inv_gj(A):
    """t x t inverse, Gauss-Jordan with partial pivoting (the library's inv(vare) / inv(G_j) order); NaN when singular."""
    t = A.shape[0]
    M = np.zeros((t, 2 * t))
    M[:, :t] = A
    M[:, t:] = np.eye(t)
    M = M.tolist()
    for c in range(t):
        piv = c
        for i in range(c + 1, t):
            if abs(M[i][c]) > abs(M[piv][c]):
                piv = i
        if M[piv][c] == 0.0:
            return np.full((t, t), np.nan)
        M[c], M[piv] = M[piv], M[c]
        d = M[c][c]
        M[c] = [v / d for v in M[c]]
        for i in range(t):
            if i != c:
                f = M[i][c]
                if f != 0.0:
                    M[i] = [M[i][q] - f * M[c][q] for q in range(2 * t)]
    return np.array([row[t:] for row in M])


def _chol(t, A):
    L = [[0.0] * t for _ in range(t)]
    for j in range(t):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        L[j][j] = math.sqrt(s) if s >= 0.0 else math.nan
        for i in range(j + 1, t):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    return L


def mt2_state(t, st, w, d, R, G, z):
    """One joint state (MTBayesABC.jl:178-185): q = -0.5 (log det lhs - rhs'gHat) and the candidate gHat + chol(lhs^-1) z."""
    D = [1.0 if (st >> a) & 1 else 0.0 for a in range(t)]
    lhs = [[((D[a] * R[a][c]) * D[c]) * d + G[a][c] for c in range(t)] for a in range(t)]
    rhs = []
    for a in range(t):
        s = 0.0
        for m in range(t):
            s = s + (R[m][a] * D[a]) * w[m]
        rhs.append(s)
    L = _chol(t, lhs)
    M = [[0.0] * t for _ in range(t)]
    for j in range(t):
        M[j][j] = 1.0 / L[j][j]
        for i in range(j + 1, t):
            s = 0.0
            for k in range(j, i):
                s = s + L[i][k] * M[k][j]
            M[i][j] = -s / L[i][i]
    inv = [[0.0] * t for _ in range(t)]
    for a in range(t):
        for c in range(t):
            s = 0.0
            for k in range(max(a, c), t):
                s = s + M[k][a] * M[k][c]
            inv[a][c] = s
    det = 1.0
    for j in range(t):
        det = det * (L[j][j] * L[j][j])
    quad, gHat = 0.0, []
    for a in range(t):
        s = 0.0
        for c in range(t):
            s = s + inv[a][c] * rhs[c]
        gHat.append(s)
        quad = quad + rhs[a] * s
    q = -0.5 * (_log(det) - quad)
    C = _chol(t, inv)
    cand = []
    for a in range(t):
        s = gHat[a]
        for c in range(a + 1):
            s = s + C[a][c] * z[c]
        cand.append(s)
    return q, cand


def mt2_update(t, w, d, R, G, lpr, seed, marker, it, rep):
    """_MTBayesABC_samplerII! for one marker: (alpha, beta, delta) lists.  Draws: normal slot k < t, uniform slot 0."""
    z = [O.normal(seed, marker, it, rep, k) for k in range(t)]
    u = O.uniform(seed, marker, it, rep, 0)
    ns = 1 << t
    ld, cands = [], []
    mx = -math.inf
    for s in range(ns):
        q, cand = mt2_state(t, s, w, d, R, G, z)
        v = q + lpr[s]
        ld.append(v)
        cands.append(cand)
        if v > mx:
            mx = v
    den = 0.0
    for s in range(ns):
        ld[s] = _exp(ld[s] - mx)
        den += ld[s]
    which, cp = ns - 1, 0.0
    for s in range(ns):
        cp += ld[s] / den
        if u < cp:
            which = s
            break
    dl = [1.0 if (which >> k) & 1 else 0.0 for k in range(t)]
    b = cands[which]
    return [dl[k] * b[k] for k in range(t)], list(b), dl


def mt1_update(t, w, d, a, b, dl, R, G, lpr, seed, marker, it, rep):
    """_MTBayesABC_samplerI! for one marker (MTBayesABC.jl:76-121), T = Float64, the literal order (no linear-form rule)."""
    a, b, dl = list(a), list(b), list(dl)
    for k in range(t):
        Ginv11 = G[k][k]
        C11 = Ginv11 + R[k][k] * d
        rhs0 = c12b = wR = 0.0
        for m in range(t):
            wR = wR + w[m] * R[m][k]
            if m == k:
                continue
            C12m = G[k][m] + (d * dl[m]) * R[k][m]
            rhs0 = rhs0 + G[k][m] * b[m]
            c12b = c12b + C12m * b[m]
        rhs0 = -rhs0
        invLhs0 = 1.0 / Ginv11
        gHat0 = rhs0 * invLhs0
        invLhs1 = 1.0 / C11
        rhs1 = wR - c12b
        gHat1 = rhs1 * invLhs1
        s0 = 0
        for m in range(t):
            if m != k and dl[m] != 0.0:
                s0 |= 1 << m
        s1 = s0 | (1 << k)
        ld0 = -0.5 * (_log(Ginv11) - gHat0 * gHat0 * Ginv11) + lpr[s0]
        ld1 = -0.5 * (_log(C11) - gHat1 * gHat1 * C11) + lpr[s1]
        prob1 = 1.0 / (1.0 + _exp(ld0 - ld1))
        u = O.uniform(seed, marker, it, rep, k)
        z = O.normal(seed, marker, it, rep, k)
        if u < prob1:
            dl[k] = 1.0
            b[k] = gHat1 + z * math.sqrt(invLhs1)
            a[k] = b[k]
        else:
            b[k] = gHat0 + z * math.sqrt(invLhs0)
            dl[k] = 0.0
            a[k] = 0.0
    return a, b, dl


def mt_block_sweep(kind, X, xpx, r, alpha, beta, delta, vare, var_effect, log_prior, seed, it, starts, nreps=1,
                   independent=False, w=None, ginv_mat=None, marker0=0):
    """One sweep, in place.  X n x p; r, alpha, beta, delta t x p (r: t x n) float64; log_prior 2^t or p x 2^t;
    ginv_mat: p x t x t per-marker G_j^-1 (BayesA/B) or None (var_effect shared); starts: block starts (0-based)."""
    t, p = alpha.shape
    R = inv_gj(np.asarray(vare, dtype=np.float64).reshape(t, t)).tolist()
    G0 = None if ginv_mat is not None else inv_gj(np.asarray(var_effect, dtype=np.float64).reshape(t, t)).tolist()
    lp = np.asarray(log_prior, dtype=np.float64)
    ww = np.ones(X.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    bounds = list(starts) + [p]
    a_start = alpha.copy()
    snap = r * ww
    for bi in range(len(starts)):
        j0, j1 = int(bounds[bi]), int(bounds[bi + 1])
        b = j1 - j0
        Xb = X[:, j0:j1]
        Gram = Xb.T @ (ww[:, None] * Xb)
        rhs = (snap if independent else r * ww) @ Xb                        # t x b: X_b'R^-1 r
        for rep in range(nreps if nreps > 0 else b):
            for c in range(b):
                j = j0 + c
                d = float(xpx[j])
                a_old = alpha[:, j].tolist()
                wv = [float(rhs[k, c]) + d * a_old[k] for k in range(t)]
                Gj = ginv_mat[j].tolist() if ginv_mat is not None else G0
                lpr = (lp[j] if lp.ndim == 2 else lp).tolist()
                if kind == SAMPLER_II:
                    an, bn, dn = mt2_update(t, wv, d, R, Gj, lpr, seed, marker0 + j, it, rep)
                else:
                    an, bn, dn = mt1_update(t, wv, d, a_old, beta[:, j].tolist(), delta[:, j].tolist(), R, Gj, lpr,
                                            seed, marker0 + j, it, rep)
                alpha[:, j], beta[:, j], delta[:, j] = an, bn, dn
                for k in range(t):
                    coef = a_old[k] - an[k]
                    if coef != 0.0:
                        rhs[k] += coef * Gram[c]
        if not independent:
            r += (a_start[:, j0:j1] - alpha[:, j0:j1]) @ Xb.T
    if independent:
        r += (a_start - alpha) @ X.T


# ---- per-marker inverse-Wishart draw (orc_sample_marker_covariances, in double) -----------------------------------------
def _u52(lo, hi):
    return ((((int(hi) << 32) | int(lo)) >> 12) + 0.5) * 2.0 ** -52


def _iw_chi2(seed, marker, it, slot, nu):
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    a, boost = 0.5 * nu, 1.0
    if a < 1.0:
        wd = O.philox([marker, it, 0x80000000 | 0xFFFF, slot], key)
        boost = math.exp(math.log(_u52(wd[0], wd[1])) / a)
        a = a + 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    g = d
    for attempt in range(64):
        wd = O.philox([marker, it, 0x80000000 | attempt, slot], key)
        w2 = O.philox([marker, it, 0x80000000 | attempt, slot + 1], key)
        x = math.sqrt(-2.0 * math.log(_u52(wd[0], wd[1]))) * math.cos(6.283185307179586476925286766559 * _u52(wd[2], wd[3]))
        u = _u52(w2[0], w2[1])
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        g = d * v
        if math.log(u) < 0.5 * x * x + d - d * v + d * math.log(v):
            break
    return 2.0 * g * boost


def sample_marker_covariances(beta, df, scale, seed, it, marker0=0):
    """G_j ~ InverseWishart(df, scale + b_j b_j') for every marker from the double beta (t x p): p x t x t float64 --
    Bartlett's decomposition on the counters of orc_sample_marker_covariances, nothing rounded to float."""
    t, p = beta.shape
    sc = np.asarray(scale, dtype=np.float64).reshape(t, t).tolist()
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    out = np.empty((p, t, t))
    for j in range(p):
        marker = marker0 + j
        bj = beta[:, j].tolist()
        S = [[sc[a][c] + bj[a] * bj[c] for c in range(t)] for a in range(t)]
        C = _chol(t, S)
        A = [[0.0] * t for _ in range(t)]
        for i in range(t):
            A[i][i] = math.sqrt(_iw_chi2(seed, marker, it, 32 + 2 * i, df - i))
            for k in range(i):
                wd = O.philox([marker, it, 0x80000000, 64 + 4 * i + k], key)
                A[i][k] = math.sqrt(-2.0 * math.log(_u52(wd[0], wd[1]))) * math.cos(6.283185307179586476925286766559 * _u52(wd[2], wd[3]))
        Kt = [[0.0] * t for _ in range(t)]
        for i in range(t):
            for c in range(t):
                acc = C[c][i]
                for k in range(i):
                    acc = acc - A[i][k] * Kt[k][c]
                Kt[i][c] = acc / A[i][i]
        for a in range(t):
            for c in range(t):
                s = 0.0
                for i in range(t):
                    s = s + Kt[i][a] * Kt[i][c]
                out[j, a, c] = s
    return 0.5 * (out + out.transpose(0, 2, 1))


class RestatementEngine64(OracleEngine64):
    """The sweep-engine protocol for runMCMC(double_precision=true) with the multi-trait kinds on the restatement above:
    sampler I / II, shared or per-marker covariances, shared or marker-specific joint priors; the per-marker covariances
    resident here like on the device (sweep(var_effect_matrix=...) uploads, sample_marker_covariances draws)."""

    def init_state(self, method, ntraits=1):
        code = self._code = {"MTBayesC": MTBAYESC1, "MTBayesC_II": MTBAYESC2, "MTBayesB": MTBAYESB1,
                             "MTBayesB_II": MTBAYESB2}.get(method, method) if isinstance(method, str) else int(method)
        if code in (MTBAYESC1, MTBAYESC2, MTBAYESB1, MTBAYESB2):
            super().init_state(MTBAYESC1, ntraits)
            self.method = code
        else:
            super().init_state(method, ntraits)
        self.var_mat = None

    def sample_marker_covariances(self, df, scale, *, seed, iteration, marker_offset=0):
        self.var_mat = sample_marker_covariances(self.beta, df, scale, int(seed), int(iteration), marker_offset)

    def marker_covariances(self):
        return self.var_mat.copy()

    def sweep(self, *, iteration, seed, vare, var_effect, log_prior_states=None, var_effect_matrix=None, nreps=1,
              marker_offset=0, independent_blocks=False, **kw):
        if self.method not in (MTBAYESC1, MTBAYESC2, MTBAYESB1, MTBAYESB2):
            return super().sweep(iteration=iteration, seed=seed, vare=vare, var_effect=var_effect, log_prior_states=log_prior_states,
                                 nreps=nreps, marker_offset=marker_offset, independent_blocks=independent_blocks, **kw)
        t = self.ntraits
        ginv = None
        if self.method in (MTBAYESB1, MTBAYESB2):
            if var_effect_matrix is not None:
                self.var_mat = np.array(var_effect_matrix, dtype=np.float64).reshape(self.p, t, t)
            ginv = np.stack([inv_gj(g) for g in self.var_mat])
        kind = SAMPLER_II if self.method in (MTBAYESC2, MTBAYESB2) else SAMPLER_I
        a_before = self.alpha.copy()
        mt_block_sweep(kind, self.X, self._xpx, self.r, self.alpha, self.beta, self.delta, vare, var_effect, log_prior_states,
                       int(seed), int(iteration), self.block_starts(), nreps=nreps, independent=independent_blocks,
                       w=getattr(self, "_w", None), ginv_mat=ginv, marker0=marker_offset)
        ww = np.ones(self.n) if getattr(self, "_w", None) is None else self._w
        state = np.zeros(self.p, dtype=np.int64)
        for k in range(t):
            state |= (self.delta[k] != 0).astype(np.int64) << k
        return {"alpha_ss": self.alpha @ self.alpha.T, "beta_ss": self.beta @ self.beta.T, "resid_ss": (self.r * ww) @ self.r.T,
                "resid_sum": (self.r * ww).sum(axis=1), "n_events": float(np.any(a_before != self.alpha, axis=0).sum()),
                "sweep_ms": 0.0, "class_counts": np.zeros(4), "bayesr_ssq": 0.0, "bayesr_nnz": 0.0,
                "sum_delta": self.delta.sum(axis=1), "state_counts": np.bincount(state, minlength=1 << t).astype(np.float64)}
