"""TEST INFRASTRUCTURE: a numpy / scipy.special restatement of the device's liability step (csrc/liability.hpp) on the same
Philox counters, and stand-in engines that add the liability methods of HipEngine to OracleEngine / OracleEngine64.

The formula (one counter uniform per draw, no rejection loop), with lo < hi the standardised bounds and S(x) = Phi(-x):
    lo + hi >= 0 (or NaN)   q = max(S(lo) - u (S(lo) - S(hi)), 2^-1074),  z = -Phi^-1(q)
    otherwise               the mirror image: the draw for (-hi, -lo), negated
    S(lo) < 2^-1022         z = lo - log1p(-u (1 - exp(-lo (hi - lo)))) / lo        (exponential tail; an approximation)
    z clamped into [lo, hi]; liability = clamp(cmean + eps, L, U), residual = eps = m + s z.
S and Phi^-1 are scipy.special.ndtr / ndtri here and erfc / erfcinv of the device's libm there: two implementations of the same
few-ulp functions (tests/test_liability_host.py measures this one against a 50-digit evaluation).
"""
import os
import sys

import numpy as np
from scipy.special import ndtr, ndtri

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine, OracleEngine64  # noqa: E402

CONTINUOUS, CATEGORICAL, CENSORED = 0, 1, 2
DBL_MIN = 2.2250738585072014e-308
DBL_TRUE_MIN = 4.9406564584124654e-324
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised over the counter words (csrc/rng.hpp)."""
    c0, c1, c2, c3 = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & _MASK, np.uint64(k1) & _MASK
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _MASK, (k1 + np.uint64(0xBB67AE85)) & _MASK
    return c0, c1, c2, c3


def liability_uniform(individuals, iteration, gibbs_round, trait, seed):
    """u = (k + 0.5) 2^-52, k = the top 52 bits of words (1, 0) of philox(individual, iteration, 0x40000000 | round, 2 + 16 trait)."""
    seed = int(seed)
    w0, w1, _, _ = philox4x32_10(np.asarray(individuals, dtype=np.uint64), np.uint64(iteration), np.uint64(0x40000000 | int(gibbs_round)),
                                 np.uint64(2 + 16 * int(trait)), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    k = ((w1 << np.uint64(32)) | w0) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def _tn_upper(lo, hi, u):
    with np.errstate(all="ignore"):
        a, b = ndtr(-lo), ndtr(-hi)
        q = np.fmax(a - u * (a - b), DBL_TRUE_MIN)
        z_main = -ndtri(q)
        z_tail = lo - np.log1p(-u * (1.0 - np.exp(-lo * (hi - lo)))) / lo
    z = np.where(a >= DBL_MIN, z_main, z_tail)
    return np.fmin(np.fmax(z, lo), hi)


def truncated_std_normal(lo, hi, u):
    lo, hi, u = [np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(lo, hi, u)]
    with np.errstate(invalid="ignore"):
        mirror = lo + hi < 0.0
    return np.where(mirror, -_tn_upper(np.where(mirror, -hi, lo), np.where(mirror, -lo, hi), u), _tn_upper(lo, hi, u))


def truncated_std_normal_mp(lo, hi, u, dps=50):
    """The same formula for ONE case at `dps` digits (mpmath): what the doubles above approximate."""
    import mpmath as mp
    with mp.workdps(dps):
        lo, hi, u = mp.mpf(lo), mp.mpf(hi), mp.mpf(u)

        def S(x):
            return mp.erfc(x / mp.sqrt(2)) / 2

        def upper(lo, hi):
            a, b = S(lo), S(hi)
            return _mp_upper_quantile(a - u * (a - b))

        z = -upper(-hi, -lo) if lo + hi < 0 else upper(lo, hi)
        return max(min(z, hi), lo)


def _mp_upper_quantile(q):
    """z with S(z) = q: Newton on log S (well conditioned in the tail, where erfinv(1 - 2q) would lose the digits of q)."""
    import mpmath as mp
    if q > mp.mpf("0.5"):
        return -_mp_upper_quantile(1 - q)
    z = mp.sqrt(-2 * mp.log(q)) if q < mp.mpf("0.1") else mp.mpf("0.5")
    for _ in range(200):
        s = mp.erfc(z / mp.sqrt(2)) / 2
        step = (mp.log(s) - mp.log(q)) * s / (mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi))
        z += step
        if abs(step) < mp.mpf(10) ** (-(mp.mp.dps - 5)):
            break
    return z


def inv_small_f64(A):
    """Gauss-Jordan with partial pivoting: the operation sequence of the library's inv_small_f64."""
    n = A.shape[0]
    M = np.hstack([np.array(A, dtype=np.float64), np.eye(n)])
    for c in range(n):
        piv = c
        for i in range(c + 1, n):
            if abs(M[i, c]) > abs(M[piv, c]):
                piv = i
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for i in range(n):
            if i != c and M[i, c] != 0.0:
                M[i] = M[i] - M[i, c] * M[c]
    return M[:, n:]


def conditional(R, init=False):
    """B (row k: R_12 R_22^-1 against the other traits) and sd (sqrt of R_11 - R_12 R_22^-1 R_21), summed as the library sums."""
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    t = R.shape[0]
    B, sd = np.zeros((t, t)), np.zeros(t)
    for k in range(t):
        var = R[k, k]
        if not init and t > 1:
            o = [j for j in range(t) if j != k]
            R22i, R12 = inv_small_f64(R[np.ix_(o, o)]), R[k, o]
            for a in range(len(o)):
                acc = 0.0
                for e in range(len(o)):
                    acc += R12[e] * R22i[e, a]
                B[k, o[a]] = acc
            for a in range(len(o)):
                var -= B[k, o[a]] * R12[a]
        sd[k] = np.sqrt(var)
    return B, sd


def bounds_from_thresholds(thresholds, codes):
    th = np.asarray(thresholds, dtype=np.float64)
    c = np.asarray(codes)
    return np.where(c == 0, -np.inf, th[np.maximum(c, 1) - 1]), np.where(c == 0, np.inf, th[c])


def liability_draw(r, y, kinds, lower, upper, *, iteration, seed, ngibbs, R, init, dtype, unrounded=False):
    """One call of k_liability_sample.  r: (t, n) residuals; y / lower / upper: per trait vectors (None for continuous traits).
    Returns (r_new, y_new) rounded to `dtype`, the arithmetic in double like the device's (unrounded: the doubles themselves)."""
    t, n = len(kinds), np.shape(r)[1]
    B, sd = conditional(R, init)
    r = [np.asarray(r[k], dtype=dtype).astype(np.float64) for k in range(t)]
    yv = [None if kinds[k] == CONTINUOUS else np.asarray(y[k], dtype=dtype).astype(np.float64) for k in range(t)]
    cm = [None if kinds[k] == CONTINUOUS else yv[k] - r[k] for k in range(t)]
    ind = np.arange(n)
    for rnd in range(1 if init else ngibbs):
        for k in range(t):
            if kinds[k] == CONTINUOUS:
                continue
            L, U = np.asarray(lower[k], dtype=np.float64), np.asarray(upper[k], dtype=np.float64)
            exact = L == U
            m = np.zeros(n)
            for j in range(t):
                if j != k:
                    m = m + B[k, j] * r[j]
            with np.errstate(invalid="ignore"):
                lo, hi = ((L - cm[k]) - m) / sd[k], ((U - cm[k]) - m) / sd[k]
            u = liability_uniform(ind, 0 if init else iteration, rnd, k, seed)
            safe_lo, safe_hi = np.where(exact, -1.0, lo), np.where(exact, 1.0, hi)
            eps = m + sd[k] * truncated_std_normal(safe_lo, safe_hi, u)
            ynew = np.fmin(np.fmax(cm[k] + eps, L), U)
            if init:
                yv[k] = np.where(exact, L, ynew)
                with np.errstate(invalid="ignore"):
                    r[k] = np.where(exact, L - cm[k], eps)
            else:
                yv[k] = np.where(exact, yv[k], ynew)
                r[k] = np.where(exact, r[k], eps)
    if unrounded:
        return r, yv
    return ([r[k].astype(dtype) for k in range(t)], [None if yv[k] is None else yv[k].astype(dtype) for k in range(t)])


def liability_draw_mp(i, r, y, kinds, lower, upper, *, iteration, seed, ngibbs, R, init, dps=50):
    """Record i of liability_draw with every operation at `dps` digits, from the same double inputs, B, sd and uniforms: what
    the doubles approximate.  Returns (r_new, y_new) as lists of mpmath numbers (None for continuous traits)."""
    import mpmath as mp
    t = len(kinds)
    B, sd = conditional(R, init)
    with mp.workdps(dps):
        rr = [mp.mpf(float(r[k][i])) for k in range(t)]
        yy = [None if kinds[k] == CONTINUOUS else mp.mpf(float(y[k][i])) for k in range(t)]
        cm = [None if kinds[k] == CONTINUOUS else yy[k] - rr[k] for k in range(t)]
        for rnd in range(1 if init else ngibbs):
            for k in range(t):
                if kinds[k] == CONTINUOUS:
                    continue
                L, U = mp.mpf(float(lower[k][i])), mp.mpf(float(upper[k][i]))
                if L == U:
                    if init:
                        yy[k], rr[k] = L, L - cm[k]
                    continue
                m = mp.mpf(0)
                for j in range(t):
                    if j != k:
                        m += mp.mpf(float(B[k, j])) * rr[j]
                s = mp.mpf(float(sd[k]))
                u = float(liability_uniform([i], 0 if init else iteration, rnd, k, seed)[0])
                eps = m + s * truncated_std_normal_mp(((L - cm[k]) - m) / s, ((U - cm[k]) - m) / s, u, dps)
                yy[k], rr[k] = min(max(cm[k] + eps, L), U), eps
        return rr, yy


def category_minmax(y, codes, nthresholds):
    """(max_below, min_above) per threshold, as jwas_hip_liability_minmax returns them."""
    y, codes = np.asarray(y, dtype=np.float64), np.asarray(codes)
    mx, mn = np.full(nthresholds, -np.inf), np.full(nthresholds, np.inf)
    mn[0], mx[nthresholds - 1] = -np.inf, np.inf
    for i in range(1, nthresholds - 1):
        below, above = y[codes == i], y[codes == i + 1]
        mx[i] = below.max() if below.size else -np.inf
        mn[i] = above.min() if above.size else np.inf
    return mx, mn


class _LiabilityMixin:
    """The liability methods of HipEngine on an engine that keeps its residuals in self.r (t x n)."""

    def init_state(self, method, ntraits=1):
        super().init_state(method, ntraits)
        self._linited = False                   # (jwas_hip_init_state zeroes the residual: the set-up draw has to be repeated)

    def liability_begin(self, ntraits=None):
        t = self.ntraits if ntraits is None else int(ntraits)
        assert t == self.ntraits
        self._lk = [CONTINUOUS] * t
        self._ly, self._lcodes, self._lthr = [None] * t, [None] * t, [None] * t
        self._llo, self._lup = [None] * t, [None] * t
        self._linited = False

    def set_categorical(self, trait, codes, thresholds):
        self._lk[trait], self._linited = CATEGORICAL, False
        self._lcodes[trait] = np.asarray(codes, dtype=np.int32).copy()
        self._ly[trait] = self._lcodes[trait].astype(self.r.dtype)
        self.set_thresholds(trait, thresholds)

    def set_censored(self, trait, lower, upper):
        lo, up = np.asarray(lower, dtype=np.float64).copy(), np.asarray(upper, dtype=np.float64).copy()
        self._lk[trait], self._linited = CENSORED, False
        self._llo[trait], self._lup[trait] = lo, up
        self._ly[trait] = np.where(lo == -np.inf, np.where(up == np.inf, 0.0, up), lo).astype(self.r.dtype)

    def set_thresholds(self, trait, thresholds):
        self._lthr[trait] = np.asarray(thresholds, dtype=np.float64).copy()
        self._llo[trait], self._lup[trait] = bounds_from_thresholds(self._lthr[trait], self._lcodes[trait])

    def _liab_draw(self, iteration, seed, ngibbs, R, init):
        # what jwas_hip_liability_init / _sample refuse (liab_draw in csrc/session_liability.hip), refused here too
        Rm = np.atleast_2d(np.asarray(R, dtype=np.float64))
        t = self.ntraits
        if all(k == CONTINUOUS for k in self._lk):
            raise ValueError("no trait was declared categorical or censored")
        if not init and not getattr(self, "_linited", False):
            raise ValueError("liability_init has not been called")
        if not init and int(iteration) < 1:
            raise ValueError("iteration must be >= 1 (0 is the set-up draw)")
        if not init and not 1 <= int(ngibbs) <= 1000:
            raise ValueError("ngibbs must be 1..1000")
        if Rm.shape != (t, t) or not np.all(np.isfinite(Rm)) or not np.array_equal(Rm, Rm.T):
            raise ValueError("R must be finite and symmetric")
        with np.errstate(invalid="ignore"):
            sd = conditional(Rm, init)[1]
        if not np.all(np.isfinite(sd) & (sd > 0)):
            raise ValueError("R is not positive definite")
        if init:
            self._linited = True
        rn, yn = liability_draw(self.r, self._ly, self._lk, self._llo, self._lup, iteration=iteration, seed=seed, ngibbs=ngibbs,
                                R=R, init=init, dtype=self.r.dtype)
        for k in range(self.ntraits):
            if self._lk[k] != CONTINUOUS:
                self.r[k], self._ly[k] = rn[k], yn[k]

    def liability_init(self, *, seed, R):
        self._liab_draw(0, seed, 1, R, True)

    def liability_sample(self, *, iteration, seed, ngibbs, R):
        self._liab_draw(iteration, seed, ngibbs, R, False)

    def liability_minmax(self, trait):
        return category_minmax(self._ly[trait], self._lcodes[trait], len(self._lthr[trait]))

    def liabilities(self, trait):
        return self._ly[trait].astype(np.float64)

    def liability_end(self):
        self._lk = None


class LiabilityOracleEngine(_LiabilityMixin, OracleEngine):
    pass


class LiabilityOracleEngine64(_LiabilityMixin, OracleEngine64):
    pass
