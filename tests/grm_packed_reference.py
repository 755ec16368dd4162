"""TEST INFRASTRUCTURE for the relationship matrix of 2-bit packed genotypes (csrc/gblup.hpp k_grm_packed, HipEngine.grm_packed):
the decode of a packed payload restated in numpy, test payloads with the missing-value patterns the kernel's staging has to get right,
and stand-in engines for the host side of api.genomic_relationship_matrix.  The package never imports this file.

A payload is p x cld(n,4) bytes; individual i of a marker sits in byte i >> 2 at bit shift (i & 3) << 1; codes 0/1/2 are genotypes,
3 is missing.  A marker decodes (PackedCols::dec, kernels.hpp) to  v = code == 3 ? mu : Float32(code);  x = centered ? v - mu : v.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gblup_reference as GR  # noqa: E402
import plink_reference as PR  # noqa: E402


def unpack(payload, n):
    """p x stride payload -> n x p codes, one individual at a time."""
    payload = np.asarray(payload, dtype=np.uint8)
    codes = np.empty((n, payload.shape[0]), dtype=np.uint8)
    for i in range(n):
        codes[i] = (payload[:, i >> 2] >> np.uint8((i & 3) << 1)) & np.uint8(3)
    return codes


def decode(codes, means, centered):
    """n x p Float32 columns of n x p codes: PackedCols::dec."""
    mu = np.asarray(means, dtype=np.float32)[None, :]
    v = np.where(codes == 3, mu, codes.astype(np.float32)).astype(np.float32)
    return np.asfortranarray((v - mu).astype(np.float32) if centered else v)


def case_codes(n, p, seed):
    """n x p codes, about 3 % missing, every marker with 0 < mean < 2.  Marker 1 has one byte (rows 4 .. 7, as many as exist) whose
    codes are all missing; with n > 128, marker 2 is missing for the whole first 128-row panel and row 128 holds a genotype.
    Returns (codes, the Float32 means of the non-missing codes)."""
    rng = np.random.default_rng(seed)
    freq = 0.15 + 0.7 * rng.random(p)
    codes = rng.binomial(2, freq, size=(n, p)).astype(np.uint8)
    codes[rng.random((n, p)) < 0.03] = 3
    if n >= 7:
        codes[4:8, 1 % p] = 3
    if p > 2 and n > 128:
        codes[:128, 2] = 3
        codes[128, 2] = 1
    for j in range(p):                                            # 0 < mean < 2: the divisor is positive
        rows = np.flatnonzero(codes[:, j] != 3)
        if rows.size == 0:
            codes[0, j], codes[1, j] = 0, 2
        elif codes[rows, j].sum() in (0, 2 * rows.size):
            codes[rows[0], j] = 1
    miss = codes == 3
    cnt = (~miss).sum(axis=0)
    means = (np.where(miss, 0, codes).sum(axis=0) / cnt).astype(np.float32)
    return codes, means


def divisor_of(means):
    """Float32 sqrt(2 p (1 - p)), p = mean / 2: api.genomic_relationship_matrix's expression."""
    f = (np.asarray(means, dtype=np.float32) / np.float32(2.0)).astype(np.float32)
    return np.sqrt(np.float32(2.0) * f * (np.float32(1.0) - f)).astype(np.float32)


class GrmPackedStandInEngine(PR.PlinkStandInEngine):
    """PlinkStandInEngine plus what genomic_relationship_matrix and plink_genotypes ask of an engine that holds packed genotypes:
    grm_packed (numpy, on the decoded columns), load_jgb2, storage_info.  It counts what a caller must not do to a resident engine."""
    GRM_CHUNK = 64
    dtype = np.float32

    def __init__(self):
        super().__init__()
        self.block_size = 0
        self.loads = self.closes = 0

    def plink_scan(self, *a, **kw):
        self.loads += 1
        return super().plink_scan(*a, **kw)

    def load_jgb2(self, path):
        from jwas_jl_amd import streaming as S
        b = S.load_streaming_backend(path)
        self.loads += 1
        self._payload = np.fromfile(b["data_path"], dtype=np.uint8).reshape(b["nMarkers"], b["stride_bytes"])
        self.n, self.p = b["nObs"], b["nMarkers"]
        self.means, self.centered = b["marker_means"].astype(np.float32), b["centered"]

    def setup_blocks(self, block_size=256, gram_mode="mfma"):
        self.block_size = int(block_size)

    def storage_info(self):
        return {"kind": "packed2bit", "n": self.n, "p": self.p, "bytes": int(self._payload.size)}

    def decoded(self):
        return decode(unpack(self._payload, self.n), self.means, self.centered)

    def grm_packed(self, divisor):
        d = np.asarray(divisor, dtype=np.float32)
        if d.shape != (self.p,) or not np.all(np.isfinite(d) & (d > 0)):
            raise ValueError("divisor must be positive and finite, one per marker")
        return GR.grm_reference(self.decoded(), d)[0].astype(np.float32)

    def close(self):
        self.closes += 1


class DenseResidentStandIn(GR.GblupStandInEngine):
    """GblupStandInEngine as the resident engine of device_genotypes on a dense matrix."""

    def __init__(self):
        super().__init__()
        self.loads = self.closes = 0

    def load_dense(self, X):
        self.loads += 1
        super().load_dense(X)

    def setup_blocks(self, block_size=256, gram_mode="f64"):
        self.block_size = int(block_size)

    def storage_info(self):
        return {"kind": "dense_f32", "n": self.n, "p": self.p, "bytes": 4 * self.n * self.p}

    def close(self):
        self.closes += 1
