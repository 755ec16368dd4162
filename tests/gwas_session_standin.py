"""numpy stand-in for the device's GWAS session (jwas_hip_gwas_begin / _sample / _local_ebv / _end) on top of OracleEngine,
and the pieces the session tests share: the literal restatement of GWAS.jl:149-173 and the derived tolerance."""
import numpy as np

from oracle_engine import OracleEngine


def csr_of_sample(nz, cs, ce):
    """The CSR description `gwas.py` builds for `window_sums`: window 0 = all markers, then every window's own slice."""
    nz = np.asarray(nz)
    lo, hi = np.searchsorted(nz, cs), np.searchsorted(nz, ce)
    counts = hi - lo
    wptr = np.concatenate([[0, nz.size], nz.size + np.cumsum(counts)]).astype(np.int32)
    gather = np.concatenate([nz] + [nz[l:h] for l, h in zip(lo, hi) if h > l]) if nz.size else nz
    return wptr, gather


class SessionOracleEngine(OracleEngine):
    """OracleEngine + the session protocol.  Sums come from the engine's own `window_sums` on the CSR of the sample (the
    contract of the device: same bits as `window_sums`); local EBVs as a running SUM divided on read-out, like the device."""
    hbm_free = 64 << 30

    def device_info(self):
        return {"n_cu": 256, "hbm_total": 288 << 30, "hbm_free": self.hbm_free}

    @staticmethod
    def gwas_estimate_bytes(n_rows, nwin, max_nnz, local_ebv=False):
        ld = (n_rows + 255) // 256 * 256
        nent = nwin + 1
        return (8 * nwin + 8 * nent + max(max_nnz, 1) * 12 + 16 * nent * (ld // 256) + 16 * nent
                + (8 * ld * nwin if local_ebv else 0))

    def gwas_begin(self, col_start, col_end, local_ebv=False, use_output_rows=False):
        self._gw_cs, self._gw_ce = np.asarray(col_start, dtype=np.int64), np.asarray(col_end, dtype=np.int64)
        self._gw_out = use_output_rows
        X = self.X_out if use_output_rows else self.X
        self._gw_X = np.asarray(X, dtype=np.float64)
        self._gw_acc = np.zeros((X.shape[0], self._gw_cs.size)) if local_ebv else None
        self._gw_ns = 0
        self.begun = getattr(self, "begun", 0) + 1

    def gwas_sample(self, idx, val):
        idx = np.asarray(idx, dtype=np.int64)
        assert idx.size == 0 or (np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < self.p)
        wptr, gather = csr_of_sample(idx, self._gw_cs, self._gw_ce)
        dense = np.zeros(self.p, dtype=np.asarray(val).dtype)
        dense[idx] = val
        s, q = self.window_sums(wptr, gather, dense[gather], use_output_rows=self._gw_out)
        if self._gw_acc is not None:
            lo, hi = np.searchsorted(idx, self._gw_cs), np.searchsorted(idx, self._gw_ce)
            v64 = np.asarray(val, dtype=np.float64)
            for w in range(self._gw_cs.size):
                if hi[w] > lo[w]:
                    self._gw_acc[:, w] += self._gw_X[:, idx[lo[w]:hi[w]]] @ v64[lo[w]:hi[w]]
        self._gw_ns += 1
        return s, q

    def gwas_local_ebv(self):
        if self._gw_acc is None:
            raise RuntimeError("the session was begun without local_ebv")
        return (self._gw_acc / self._gw_ns if self._gw_ns else self._gw_acc.copy()), self._gw_ns

    def gwas_end(self):
        self._gw_acc = self._gw_X = None
        self.ended = getattr(self, "ended", 0) + 1


def literal_local_ebv(X, samples, col_start, col_end):
    """GWAS.jl:149-173 as written there, in Float64: per sample BV = X[:, w] * alpha[w]; localEBV[:, w] += (BV - localEBV[:, w]) / i."""
    X = np.asarray(X, dtype=np.float64)
    m = np.zeros((X.shape[0], len(col_start)))
    for i, a in enumerate(np.asarray(samples, dtype=np.float64), start=1):
        for w, (c0, c1) in enumerate(zip(col_start, col_end)):
            BV = X[:, c0:c1] @ a[c0:c1]
            m[:, w] += (BV - m[:, w]) / i
    return m


def local_ebv_bound(X, samples, col_start, col_end):
    """|device - numpy64| <= (K_w + 4 S) 2^-52 A_iw: K_w = the largest nonzero count of window w over the samples,
    S = the number of samples, A_iw = max_s sum_j |x_ij| |alpha_sj| (Float64).  Every BV is a chain of K correctly rounded
    additions (a Float32 x Float32 product is exact in a double, a Float64 product under fma is rounded once with its sum),
    the mean adds a few roundings per sample, and the numpy value carries the same kind of error."""
    Xa = np.abs(np.asarray(X, dtype=np.float64))
    Sa = np.abs(np.asarray(samples, dtype=np.float64))
    S = Sa.shape[0]
    bound = np.zeros((Xa.shape[0], len(col_start)))
    for w, (c0, c1) in enumerate(zip(col_start, col_end)):
        K = int((Sa[:, c0:c1] != 0).sum(axis=1).max()) if S else 0
        A = (Xa[:, c0:c1] @ Sa[:, c0:c1].T).max(axis=1) if S else np.zeros(Xa.shape[0])
        bound[:, w] = (K + 4 * S) * 2.0 ** -52 * A
    return bound
