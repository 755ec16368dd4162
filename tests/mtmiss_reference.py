"""TEST INFRASTRUCTURE: a numpy restatement of the device's handling of multi-trait records that miss some traits (csrc/mtmiss.hpp
and the per-record-weight instantiations of csrc/locpar.hpp) on the same Philox counters, as mixins over the stand-in engines of
tests/locpar_reference.py and tests/locpar_ped_reference.py.

A record's code has bit k set when trait k is observed.  With the per-code tables B, U, C of jwas_jl_amd.mcmc.missing_pattern_tables
(o = the observed traits ascending, m = the missing ones ascending):
    e_m[c] = sum_j B[code][c][j] e_o[j] + sum_{a <= c} z_m[a] U[code][a][c]           in that order, in double, rounded to T once
    z_k    = sqrt(-2 ln u1) cos(2 pi u2) from philox(record, iteration, 0x10000000, 4 + 16 k)
and, for level l of a term of trait k under per-record weights:
    rho_i  = sum_m C[code_i][k][m] r_m,i
    S_l    = sum_{i in l} w_i x_i rho_i            D_l = sum_{i in l} (w_i x_i) x_i C[code_i][k][k]
    lhs_l  = D_l + prior                           mean_l = (S_l + D_l sol_l - prior sums) / lhs_l,  s = 1
The level sums run in np.bincount's order, the device's in the order of its term layout (tests/test_gpu_mtmiss.py bounds that).
"""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locpar_reference as LP  # noqa: E402
from liability_reference import philox4x32_10  # noqa: E402
from locpar_ped_reference import PedOracleEngine, PedOracleEngine64  # noqa: E402
from locpar_reference import LocparOracleEngine, LocparOracleEngine64  # noqa: E402

REP_TAG, SLOT = 0x10000000, 4
MAX_T = 4


def mtmiss_normal(records, iteration, trait, seed):
    """The device's normal of trait `trait` of every record in `records`."""
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(np.asarray(records, dtype=np.uint64), np.uint64(iteration), np.uint64(REP_TAG),
                                   np.uint64(SLOT + 16 * int(trait)), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.sqrt(-2.0 * np.log(LP._u52(w0, w1))) * np.cos(6.283185307179586476925286766559 * LP._u52(w2, w3))


def impute(r, codes, B, U, *, iteration, seed, normals=None, details=None):
    """The residuals r (t x n, any float dtype) with the missing cells redrawn; observed cells and complete records are the input's.
    normals (tests only): n x t, the normal of record i, trait k.  details: a dict that receives, per missing cell, the sum of the
    absolute terms ("A"), the number of terms ("nterms") and sum |U| of its column ("absU"), each t x n (0 on observed cells)."""
    t, n = r.shape
    out = r.copy()
    if details is not None:
        details.update(A=np.zeros((t, n)), nterms=np.zeros((t, n)), absU=np.zeros((t, n)))
    for code in np.unique(codes):
        if code == (1 << t) - 1:
            continue
        rows = np.flatnonzero(codes == code)
        o = [k for k in range(t) if (code >> k) & 1]
        m = [k for k in range(t) if not (code >> k) & 1]
        eo = [r[k][rows].astype(np.float64) for k in o]
        z = [mtmiss_normal(rows, iteration, k, seed) if normals is None else normals[rows, k] for k in m]
        for c, k in enumerate(m):
            acc, absacc = np.zeros(len(rows)), np.zeros(len(rows))
            for j in range(len(o)):
                acc = acc + B[code, c, j] * eo[j]
                absacc += np.abs(B[code, c, j] * eo[j])
            for a in range(c + 1):
                acc = acc + z[a] * U[code, a, c]
                absacc += np.abs(z[a] * U[code, a, c])
            out[k][rows] = acc.astype(r.dtype)
            if details is not None:
                details["A"][k, rows] = absacc
                details["nterms"][k, rows] = len(o) + c + 1
                details["absU"][k, rows] = np.abs(U[code, :c + 1, c]).sum()
    return out


def term_draw_w(T, ordinal, r, sol, partner_offs, gi_row, Ck, *, iteration, seed, normals=None):
    """locpar_reference.term_draw under per-record weights: Ck (n x t) is row `trait` of C[code_i] for every record."""
    t = r.shape[0]
    k = T.trait
    rho = sum(Ck[:, m] * r[m] for m in range(t))
    absrho = sum(np.abs(Ck[:, m] * r[m]) for m in range(t))
    lv = T.level[T.inl]
    S = np.bincount(lv, weights=(T.wx * rho)[T.inl], minlength=T.nlevels)
    A = np.bincount(lv, weights=(np.abs(T.wx) * absrho)[T.inl], minlength=T.nlevels)
    D = np.bincount(lv, weights=((T.wx * T.x) * Ck[:, k])[T.inl], minlength=T.nlevels)
    old = sol[T.off:T.off + T.nlevels]
    prior = 0.0
    num = S + D * old
    A = A + np.abs(D * old)
    if T.group >= 0:
        prior = gi_row[T.pos]
        for m, po in enumerate(partner_offs):
            if m != T.pos:
                um = sol[po:po + T.nlevels]
                num = num - gi_row[m] * um
                A = A + np.abs(gi_row[m] * um)
    lhs = D + prior
    live = lhs != 0.0
    safe = np.where(live, lhs, 1.0)
    mean = num / safe
    sd = np.sqrt(1.0 / safe)
    z = LP.locpar_normal(np.arange(T.nlevels), iteration, ordinal, k, seed) if normals is None else normals
    new = np.where(live, mean + z * sd, old)
    return new, {"S": S, "A": A, "D": D, "lhs": lhs, "mean": mean, "sd": sd, "live": live, "n_l": np.bincount(lv, minlength=T.nlevels), "z": z}


def structured_term_draw_w(T, ordinal, r, sol, partner_offs, p_row, W, Ck, *, iteration, seed, normals=None):
    """locpar_ped_reference.structured_term_draw under per-record weights (D_l in the place of d_l c_kk)."""
    free = copy.copy(T)
    free.group = -1
    _, det = term_draw_w(free, ordinal, r, sol, (), None, Ck, iteration=iteration, seed=seed, normals=normals)
    nl = T.nlevels
    old = sol[T.off:T.off + nl].copy()
    cur = old.copy()
    pkk = p_row[T.pos]
    D = det["D"]
    lhs = D + pkk * W["vdiag"]
    z = det["z"]
    fixed, Afix = np.zeros(nl), np.zeros(nl)
    for m, po in enumerate(partner_offs):
        if m != T.pos:
            um = sol[po:po + nl]
            fixed += p_row[m] * (W["V"] @ um)
            Afix += np.abs(p_row[m]) * (W["Vabs"] @ np.abs(um))
    mean, A = np.zeros(nl), np.zeros(nl)
    for L, rows, absrows in zip(W["levels"], W["rows"], W["absrows"]):
        num = det["S"][L] + D[L] * old[L] - fixed[L] - pkk * (rows @ cur)
        A[L] = det["A"][L] + Afix[L] + np.abs(pkk) * (absrows @ np.abs(cur))
        mean[L] = num / lhs[L]
        cur[L] = mean[L] + z[L] * np.sqrt(1.0 / lhs[L])
    return cur, {"S": det["S"], "A": A, "D": D, "lhs": lhs, "mean": mean, "sd": np.sqrt(1.0 / lhs), "live": np.ones(nl, dtype=bool),
                 "n_l": det["n_l"] + len(partner_offs) * W["nnz_l"], "z": z, "pkk": pkk}


class _MtmissMixin:
    """mtmiss_begin / _impute / _set_record_weights / _end and the record-weighted locpar_step of HipEngine."""

    @staticmethod
    def mtmiss_estimate_bytes(n):
        return 12 * int(n) + 8 * 3 * 16 * 16

    def _mt_table(self, tab):
        t = self.ntraits
        tab = np.asarray(tab, dtype=np.float64)
        if tab.shape != (1 << t, t, t) or not np.all(np.isfinite(tab)):
            raise ValueError("a table must hold [2^t][t][t] finite values")
        return tab.copy()

    def mtmiss_begin(self, observed):
        ob = np.asarray(observed)
        if ob.ndim == 2:
            ob = ob.astype(np.int64) @ (1 << np.arange(ob.shape[1]))
        if ob.shape != (self.n,) or ob.min() < 1 or ob.max() >= 1 << self.ntraits:
            raise ValueError("codes outside 1 .. 2^t - 1, or not one per record")
        self._mt_codes, self._mt_C = ob.astype(np.int64), None

    def mtmiss_impute(self, *, iteration, seed, B, U, normals=None, details=None):
        if getattr(self, "_mt_codes", None) is None:
            raise RuntimeError("mtmiss_begin has not been called")
        if int(iteration) < 1:
            raise ValueError("iteration must be >= 1")
        self.r[:] = impute(self.r, self._mt_codes, self._mt_table(B), self._mt_table(U), iteration=iteration, seed=seed, normals=normals,
                           details=details)

    def mtmiss_set_record_weights(self, Ctab):
        if getattr(self, "_mt_codes", None) is None:
            raise RuntimeError("mtmiss_begin has not been called")
        if Ctab is not None and self.ntraits == 1:
            raise RuntimeError("per-record weights need more than one trait")
        self._mt_C = None if Ctab is None else self._mt_table(Ctab)

    def mtmiss_end(self):
        self._mt_codes, self._mt_C = None, None

    def locpar_step(self, *, iteration, seed, vare=None, Rinv=None, Gi=(), first_term=0, last_term=-1, details=None, normals=None):
        """normals (tests only): {term ordinal: the normals to use instead of the counter's}."""
        kw = dict(iteration=iteration, seed=seed, vare=vare, Rinv=Rinv, Gi=Gi)
        if getattr(self, "_mt_C", None) is None:
            if normals is not None:
                kw["normals"] = normals
            return super().locpar_step(first_term=first_term, last_term=last_term, details=details, **kw)
        nterms = len(self._lp_terms)
        last = nterms if last_term < 0 else int(last_term)
        if not 0 <= first_term <= last <= nterms:
            raise ValueError("terms outside the scan")
        structs = getattr(self, "_lp_struct", {})
        Gm = [np.atleast_2d(np.asarray(M, dtype=np.float64)) for M in Gi]
        self._lp_finalize()
        for j in range(first_term, last):
            T = self._lp_terms[j]
            Ck = self._mt_C[self._mt_codes, T.trait, :]
            offs, row = (), None
            if T.group >= 0:
                offs = [self._lp_terms[m].off for m in self._lp_groups[T.group]]
                row = Gm[T.group][T.pos]
            zz = None if normals is None else normals.get(j)
            r64 = self.r.astype(np.float64)
            if T.group in structs:
                new, det = structured_term_draw_w(T, j, r64, self._lp_sol, offs, row, structs[T.group], Ck, iteration=iteration, seed=seed, normals=zz)
            else:
                new, det = term_draw_w(T, j, r64, self._lp_sol, offs, row, Ck, iteration=iteration, seed=seed, normals=zz)
            delta = new - self._lp_sol[T.off:T.off + T.nlevels]
            self._lp_sol[T.off:T.off + T.nlevels] = new
            self.r[T.trait] = LP.term_apply(T, self.r[T.trait], delta, self.r.dtype)
            if details is not None:
                det["delta"] = delta
                details.append(det)
        return super().locpar_step(first_term=first_term, last_term=first_term, **kw)          # (no terms: the checks and utu)


class MtmissOracleEngine(_MtmissMixin, LocparOracleEngine):
    pass


class MtmissOracleEngine64(_MtmissMixin, LocparOracleEngine64):
    pass


class MtmissPedOracleEngine(_MtmissMixin, PedOracleEngine):
    pass


class MtmissPedOracleEngine64(_MtmissMixin, PedOracleEngine64):
    pass


def dense_mme_w(terms, groups, structs, w, Ri_rows, r, sol, *, Gi=()):
    """A = X' Ri X + prior and b = X' Ri (r + X sol) with the per-record Ri (n x t x t; the caller multiplies the weights in), formed
    as the host path forms them (jwas_jl_amd/mcmc.py, the branch `has_missing and (it == 1 or not R.estimate_variance)`); the priors
    are kron(Gi, I) or kron(Gi, V) for an effect with a structure."""
    import scipy.sparse as sp
    t, n = r.shape
    q = sum(T.nlevels for T in terms)
    X = [np.zeros((n, q)) for _ in range(t)]
    for T in terms:
        rows = np.flatnonzero(T.inl)
        X[T.trait][rows, T.off + T.level[rows]] = T.x[rows]
    rr = [r[k] + X[k] @ sol for k in range(t)]
    A = sum(X[k].T @ (Ri_rows[:, k, l][:, None] * X[l]) for k in range(t) for l in range(t))
    b = sum(X[k].T @ sum(Ri_rows[:, k, l] * rr[l] for l in range(t)) for k in range(t))
    for g, members in groups.items():
        G = np.atleast_2d(np.asarray(Gi[g], dtype=np.float64))
        for a, ja in enumerate(members):
            for e, je in enumerate(members):
                Ta, Te = terms[ja], terms[je]
                Vd = np.asarray(sp.csr_matrix(structs[g]).todense()) if g in structs else np.eye(Ta.nlevels)
                A[Ta.off:Ta.off + Ta.nlevels, Te.off:Te.off + Te.nlevels] += Vd * G[a, e]
    return A, b
