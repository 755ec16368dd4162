"""TEST INFRASTRUCTURE for output rows in 2-bit packed storage (plink.load_plink_output, HipEngine.load_output_packed2bit /
plink_commit_output / get_output_packed2bit / ebv_output): numpy stand-ins for the four engine methods, and a stand-in that also
carries a chain.  The package never imports this file.

The output rows are a second packed matrix with no means of its own: a field decodes with the TRAINING storage's marker mean and
centring (PackedCols::dec, kernels.hpp): v = code == 3 ? mu : Float32(code); x = centered ? v - mu : v.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grm_packed_reference as PKR  # noqa: E402
import plink_reference as PR  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402


def ebv_reference(X, alpha):
    """s = fma(double(alpha_j), double(x_ij), s) over the markers in ascending order, then one cast to Float32: the result rule of
    k_mul_alpha_list / k_mul_alpha / k_ebv_packed.  A Float32 product is exact in double, so the fma is a product and a sum."""
    X = np.asarray(X, dtype=np.float32)
    s = np.zeros(X.shape[0], dtype=np.float64)
    for j in np.flatnonzero(np.asarray(alpha) != 0):
        s = s + np.float64(alpha[j]) * X[:, j].astype(np.float64)
    return s.astype(np.float32)


class PlinkOutputStandInEngine(PR.PlinkStandInEngine):
    """PlinkStandInEngine plus the output rows: the payload of the output individuals over the training selection."""

    def __init__(self):
        super().__init__()
        self.n_out = 0
        self._out_payload = None
        self.output_loads = 0

    def _need_training(self):
        if self._payload is None:
            raise RuntimeError("packed output rows need 2-bit packed training storage")

    def load_output_packed2bit(self, payload, n_out):
        self._need_training()
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2 or payload.shape[0] != self.p or payload.shape[1] < (int(n_out) + 3) // 4:
            raise ValueError("payload must be p x stride with stride >= cld(n_out,4)")
        codes = PKR.unpack(payload, int(n_out))                  # (fields at rows >= n_out are not the output rows')
        self._out_payload, self.n_out = PR.pack_codes(codes), int(n_out)
        self.output_loads += 1

    def plink_commit_output(self, selected):
        if self._pending is None:
            raise RuntimeError("plink_scan has not been called")
        self._need_training()
        selected = np.asarray(selected, dtype=np.int64)
        if selected.size != self.p:
            raise ValueError("the selection is the training set's: p_sel differs from p")
        if np.any(np.diff(selected) <= 0) or selected[0] < 0 or selected[-1] >= self._pending.shape[1]:
            raise ValueError("selected must be strictly ascending and in range")
        codes = self._pending[:, selected]
        self._out_payload, self.n_out = PR.pack_codes(codes), codes.shape[0]
        self._pending = None
        self.output_loads += 1

    def get_output_packed2bit(self, j0, count):
        return self._out_payload[int(j0):int(j0) + int(count)].copy()

    def decoded_output(self):
        return PKR.decode(PKR.unpack(self._out_payload, self.n_out), self.means, self.centered)

    def ebv_output(self):
        X = self.decoded_output()
        return np.stack([ebv_reference(X, self.alpha[k]) for k in range(self.ntraits)])


class PlinkOutputChainEngine(PlinkOutputStandInEngine, OracleEngine):
    """... that also runs a chain: the committed training genotypes go, decoded, to the CPU oracle's sweep (oracle_engine.py)."""
    dtype = np.float32

    def __init__(self):
        PlinkOutputStandInEngine.__init__(self)
        OracleEngine.__init__(self, "block")
        self.ebv_calls = 0

    def plink_commit(self, selected, means, centered=True):
        super().plink_commit(selected, means, centered)
        self.load_dense(PKR.decode(PKR.unpack(self._payload, self.n), self.means, self.centered))

    def device_info(self):
        return {"hbm_free": 1 << 40}

    def resident_block_sizes(self):
        return list(self._sets)

    def mul_alpha_output(self, trait=0):
        return ebv_reference(self.decoded_output(), self.alpha[trait])

    def ebv_output(self):
        self.ebv_calls += 1
        return super().ebv_output()
