"""Test infrastructure for PLINK 1 binary filesets: a numpy writer and reader of .bed/.bim/.fam, written from the format's field
table and not through the library, and a numpy stand-in for the four engine methods the host side drives.

A .bed file: three bytes 6C 1B 01 (the last one: variant-major), then for every marker cld(n,4) bytes; individual i sits in byte
i >> 2 at bit shift (i & 3) << 1 with the field
    0 = homozygous for the .bim's first allele (A1)     1 = missing     2 = heterozygous     3 = homozygous for the second (A2).
Unused fields of a marker's last byte are 0.  A genotype matrix here holds the copies of A1 (0/1/2) and 9 for a missing value.
"""
import numpy as np

MAGIC = bytes([0x6C, 0x1B, 0x01])
FIELD_OF_A1_COUNT = {2: 0, 9: 1, 1: 2, 0: 3}                     # copies of A1 (9: missing) -> .bed field
A1_COUNT_OF_FIELD = np.array([2, 9, 1, 0], dtype=np.int64)       # .bed field -> copies of A1
A2_COUNT_OF_FIELD = np.array([0, 9, 1, 2], dtype=np.int64)       # .bed field -> copies of A2


def bed_bytes(G):
    """The .bed file of an n x p matrix of A1 counts (0/1/2, 9 = missing), as bytes."""
    G = np.asarray(G)
    n, p = G.shape
    stride = (n + 3) // 4
    rows = np.zeros((p, stride), dtype=np.uint8)
    for i in range(n):
        fields = np.array([FIELD_OF_A1_COUNT[int(v)] for v in G[i]], dtype=np.uint8)
        rows[:, i >> 2] |= fields << np.uint8((i & 3) << 1)
    return MAGIC + rows.tobytes()


def write_fileset(prefix, G, obs_ids=None, marker_ids=None, fids=None):
    """Writes <prefix>.bed/.bim/.fam for an n x p matrix of A1 counts; returns (obs_ids, marker_ids, a1, a2)."""
    G = np.asarray(G)
    n, p = G.shape
    obs_ids = [f"id{i + 1}" for i in range(n)] if obs_ids is None else [str(v) for v in obs_ids]
    marker_ids = [f"snp{j + 1}" for j in range(p)] if marker_ids is None else [str(v) for v in marker_ids]
    fids = [f"fam{i % 7}" for i in range(n)] if fids is None else [str(v) for v in fids]
    a1 = ["ACGT"[j % 4] for j in range(p)]
    a2 = ["CGTA"[j % 4] for j in range(p)]
    prefix = str(prefix)
    with open(prefix + ".bed", "wb") as fh:
        fh.write(bed_bytes(G))
    with open(prefix + ".fam", "w") as fh:
        for i in range(n):
            fh.write(f"{fids[i]} {obs_ids[i]} 0 0 {1 + i % 2} -9\n")
    with open(prefix + ".bim", "w") as fh:
        for j in range(p):
            fh.write(f"{1 + j % 22}\t{marker_ids[j]}\t0\t{1000 + j}\t{a1[j]}\t{a2[j]}\n")
    return obs_ids, marker_ids, a1, a2


def read_bed(path, n, p, counted="A1"):
    """The n x p matrix of counts of the counted allele (9 = missing) of a variant-major .bed file."""
    raw = open(path, "rb").read()
    stride = (n + 3) // 4
    if raw[:3] != MAGIC:
        raise ValueError("not a variant-major PLINK 1 .bed file")
    if len(raw) != 3 + p * stride:
        raise ValueError("the .bed file's size does not match n and p")
    rows = np.frombuffer(raw, dtype=np.uint8, offset=3).reshape(p, stride)
    fields = np.empty((n, p), dtype=np.int64)
    for i in range(n):
        fields[i] = (rows[:, i >> 2] >> ((i & 3) << 1)) & 3
    return (A1_COUNT_OF_FIELD if counted == "A1" else A2_COUNT_OF_FIELD)[fields]


def codes_of(G):
    """.jgb2 codes of a count matrix: 0/1/2, 3 for missing."""
    G = np.asarray(G)
    return np.where(G == 9, 3, G).astype(np.uint8)


def pack_codes(codes):
    """n x p codes -> p x cld(n,4) payload, one individual at a time (independent of the library's packer)."""
    n, p = codes.shape
    out = np.zeros((p, (n + 3) // 4), dtype=np.uint8)
    for i in range(n):
        out[:, i >> 2] |= codes[i].astype(np.uint8) << np.uint8((i & 3) << 1)
    return out


class PlinkStandInEngine:
    """numpy stand-in for HipEngine's plink_scan / plink_commit / plink_discard / get_packed2bit."""

    def __init__(self):
        self.n = self.p = 0
        self.precision = 32
        self._pending = None
        self._payload = None
        self.means = None
        self.centered = True
        self.discards = 0

    def plink_scan(self, bed_path, n_file, p_file, rows=None, count_a1=True):
        G = read_bed(bed_path, int(n_file), int(p_file), "A1" if count_a1 else "A2")
        if rows is not None:
            rows = np.asarray(rows, dtype=np.int64)
            if rows.size == 0 or rows.min() < 0 or rows.max() >= n_file or np.unique(rows).size != rows.size:
                raise ValueError("rows out of range or listed twice")
            G = G[rows]
        self._pending = codes_of(G)
        return np.stack([(self._pending == c).sum(axis=0) for c in range(4)], axis=1).astype(np.int64)

    def plink_commit(self, selected, means, centered=True):
        if self._pending is None:
            raise RuntimeError("plink_scan has not been called")
        selected = np.asarray(selected, dtype=np.int64)
        if selected.size == 0 or np.any(np.diff(selected) <= 0) or selected[0] < 0 or selected[-1] >= self._pending.shape[1]:
            raise ValueError("selected must be strictly ascending and in range")
        codes = self._pending[:, selected]
        self._payload = pack_codes(codes)
        self.n, self.p = codes.shape
        self.means, self.centered = np.asarray(means, dtype=np.float32).copy(), bool(centered)
        self._pending = None

    def plink_discard(self):
        self._pending = None
        self.discards += 1

    def get_packed2bit(self, j0, count):
        return self._payload[int(j0):int(j0) + int(count)].copy()

    def close(self):
        pass
