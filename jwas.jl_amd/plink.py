"""PLINK 1 binary filesets (<prefix>.bed/.bim/.fam) straight into the 2-bit packed storage of an engine.

A variant-major .bed file is already marker-major with four individuals per byte, individual i in byte i>>2 at bit shift (i&3)<<1:
the layout of the streaming backend's .jgb2 payload (streaming.py).  What differs is the meaning of a field (.bed: 0 = homozygous
for the .bim's first allele A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; .jgb2: 0/1/2 = copies of the counted allele,
3 = missing), the individuals that are kept and their order, and the markers that pass quality control.  The engine transcodes
every marker and counts its codes (plink_scan); the counts go through the ONE copy of the quality control, streaming._marker_summaries
(streaming_genotypes.jl:274-296); the kept markers then become the engine's packed storage (plink_commit).  Neither the raw file
nor a dense matrix exists on the host.
"""
import os

import numpy as np

from . import streaming


def resolve_bfile(bfile):
    """The prefix of a fileset from the prefix itself or the path of any of its three files."""
    path = str(bfile)
    for ext in (".bed", ".bim", ".fam"):
        if path.endswith(ext):
            return path[:-len(ext)]
    return path


def _columns(path, ncol, what):
    rows = []
    with open(path) as fh:
        for k, line in enumerate(fh):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < ncol:
                raise ValueError(f"{path}: line {k + 1} has {len(parts)} fields; a {what} line has {ncol}")
            rows.append(parts)
    return rows


def read_fam(path, id_column="IID"):
    """The individuals' IDs of a .fam file in file order: the within-family ID (id_column="IID", column 2) or family and
    within-family ID joined by an underscore ("FID_IID")."""
    if id_column not in ("IID", "FID_IID"):
        raise ValueError('id_column must be "IID" or "FID_IID"')
    rows = _columns(path, 6, ".fam")
    return [r[1] if id_column == "IID" else r[0] + "_" + r[1] for r in rows]


def read_bim(path):
    """(marker IDs, first alleles A1, second alleles A2) of a .bim file in file order."""
    rows = _columns(path, 6, ".bim")
    return [r[1] for r in rows], [r[4] for r in rows], [r[5] for r in rows]


def _keep_rows(fam_ids, keep):
    if keep is None:
        return None, list(fam_ids)
    index = {}
    for i, v in enumerate(fam_ids):
        if v in index:
            raise ValueError(f"individual {v} is listed twice in the .fam file; keep= needs unique IDs")
        index[v] = i
    rows, seen = [], set()
    for v in (str(x) for x in keep):
        if v not in index:
            raise ValueError(f"keep: individual {v} is not in the .fam file")
        if v in seen:
            raise ValueError(f"keep: individual {v} is listed twice")
        seen.add(v)
        rows.append(index[v])
    if not rows:
        raise ValueError("keep: no individual is listed")
    return np.asarray(rows, dtype=np.int64), [fam_ids[i] for i in rows]


def load_plink(engine, bfile, *, keep=None, counted_allele="A1", quality_control=True, MAF=0.01, center=True, id_column="IID"):
    """Loads <bfile>.bed into `engine` as 2-bit packed storage.  keep: the IDs of the individuals wanted, in the order wanted
    (None: all, file order).  counted_allele: "A1" (the .bim's first allele, what PLINK counts) or "A2".  Quality control as
    prepare_streaming_genotypes has it.  Returns what streaming.load_streaming_backend returns for the backend of the same
    genotypes (prefix and data_path None: nothing is on disk), plus "selected" (0-based file indices of the kept markers) and
    "counted_alleles" (the counted allele of every kept marker)."""
    if counted_allele not in ("A1", "A2"):
        raise ValueError('counted_allele must be "A1" or "A2"')
    prefix = resolve_bfile(bfile)
    for ext in (".bed", ".bim", ".fam"):
        if not os.path.isfile(prefix + ext):
            raise FileNotFoundError(f"PLINK fileset is incomplete: {prefix + ext} is not found")
    fam_ids = read_fam(prefix + ".fam", id_column)
    marker_all, a1, a2 = read_bim(prefix + ".bim")
    rows, obs_ids = _keep_rows(fam_ids, keep)
    n, p_all = len(obs_ids), len(marker_all)
    counts = engine.plink_scan(prefix + ".bed", len(fam_ids), p_all, rows, counted_allele == "A1")
    try:
        cnt = counts[:, 0] + counts[:, 1] + counts[:, 2]
        s1 = (counts[:, 1] + 2 * counts[:, 2]).astype(np.float64)
        s2 = (counts[:, 1] + 4 * counts[:, 2]).astype(np.float64)
        selected, mean, afreq, xp = streaming._marker_summaries(cnt, s1, s2, n, quality_control, MAF, center, marker_all)
        engine.plink_commit(selected, mean, center)
    except BaseException:
        engine.plink_discard()
        raise
    alleles = a1 if counted_allele == "A1" else a2
    source = PlinkSource(prefix, id_column, counted_allele, selected, fam_ids, p_all)
    return {
        "source": source,
        "prefix": None, "data_path": None, "nObs": n, "nMarkers": int(selected.size), "stride_bytes": (n + 3) // 4,
        "nMarkersAll": p_all, "centered": bool(center),
        "sum2pq": float((np.float32(2.0) * afreq * (np.float32(1.0) - afreq)).sum(dtype=np.float32)),
        "obsID": obs_ids, "markerID": [marker_all[j] for j in selected],
        "marker_means": mean, "xpRinvx": xp, "allele_freq": afreq,
        "selected": selected, "counted_alleles": [alleles[j] for j in selected], "markerID_all": marker_all,
    }


class PlinkSource:
    """Where the packed genotypes of an engine came from (plink_genotypes keeps it as g.plink_source): the fileset's prefix, the ID
    column and counted allele they were read with, the kept markers (0-based file indices) and ALL individuals of the .fam file --
    what it takes to bring further individuals of the same fileset to the device with the training set's decode."""

    def __init__(self, prefix, id_column, counted_allele, selected, fam_ids, p_file):
        self.prefix, self.id_column, self.counted_allele = prefix, id_column, counted_allele
        self.selected = np.asarray(selected, dtype=np.int64)
        self.fam_ids, self.p_file = list(fam_ids), int(p_file)


def resolve_plink_output_ids(source, want):
    """check_outputID (input_data_validation.jl:143-196) with ALL individuals of the fileset as the genotyped ones: `want` without
    the IDs the .fam file does not list, dropped with the reference's note."""
    known = set(source.fam_ids)
    want = [str(i) for i in want]
    if not all(i in known for i in want):
        print("Testing individuals are not a subset of genotyped individuals (complete genomic data,non-single-step). "
              "Only output EBV for tesing individuals with genotypes.")
        want = [i for i in want if i in known]
    return want


def load_plink_output(engine, source, ids, *, memory_guard="error", memory_guard_ratio=0.80):
    """The individuals `ids` of the fileset behind `source` become the packed output rows of `engine`, in that order: a scan of
    their rows with the training's counted allele, then the training's marker selection (the individuals' own allele counts play
    no part; a missing genotype decodes to the training mean).  ids: as keep= of load_plink -- each in the .fam file, none twice.
    The rows stay resident for a whole chain, so nothing is chunked: the staging buffer of the scan and the rows themselves must
    fit the free HBM together."""
    ids = [str(i) for i in ids]
    n_file, p_file, p = len(source.fam_ids), source.p_file, int(source.selected.size)
    if ids == source.fam_ids:
        rows, n_out = None, n_file                       # all of the file in file order: the direct transcode
    else:
        rows, _ = _keep_rows(source.fam_ids, ids)
        n_out = int(rows.size)
    if n_out == 0:
        raise ValueError("keep: no individual is listed")
    if memory_guard != "off" and hasattr(engine, "device_info"):
        sb = (n_out + 255) // 256 * 256 // 4
        stage, rows_b = sb * p_file, sb * p
        free = engine.device_info()["hbm_free"]
        if stage + rows_b > memory_guard_ratio * free:
            msg = (f"the output rows of {n_out} individuals need {stage / 1e9:.2f} GB of HBM for the scan's staging buffer and "
                   f"{rows_b / 1e9:.2f} GB for the rows, more than {memory_guard_ratio:.2f} x free ({free / 1e9:.2f} GB)")
            if memory_guard == "error":
                raise MemoryError(msg)
            print("WARNING: " + msg)
    engine.plink_scan(source.prefix + ".bed", n_file, p_file, rows, source.counted_allele == "A1")
    try:
        engine.plink_commit_output(source.selected)
    except BaseException:
        engine.plink_discard()
        raise
    return n_out


def write_streaming_backend(engine, backend, prefix, chunk_bytes=64 << 20):
    """The streaming backend <prefix>.{jgb2,meta,...} of what load_plink left on `engine`: the payload read back in chunks
    of markers, the sidecars by streaming's own writer."""
    n, p, stride = backend["nObs"], backend["nMarkers"], backend["stride_bytes"]
    step = max(1, chunk_bytes // max(stride, 1))
    with open(prefix + ".jgb2", "wb") as fh:
        for j0 in range(0, p, step):
            engine.get_packed2bit(j0, min(step, p - j0)).tofile(fh)
    streaming._write_sidecars(prefix, n, backend["nMarkersAll"], backend["selected"], backend["marker_means"], backend["allele_freq"],
                              backend["xpRinvx"], backend["centered"], backend["obsID"], backend["markerID_all"])
    return prefix
