"""A PLINK 1 .bed file into 2-bit packed device storage on one MI355X (csrc/plink.hpp, jwas_hip_plink_scan / _commit): wall clock of
every leg.    python scripts/plink_bench.py [--n 20000] [--p 100000] [--legs device,host] [--dir /tmp] [--out FILE]

The .bed file is synthesised directly as bytes: `--unique` distinct marker rows (Hardy-Weinberg genotypes at f ~ U(0.05, 0.5), 3 %
missing fields, a few monomorphic rows, pad fields 0) tiled to p -- what a leg costs does not depend on the values.  Legs, each by
wall clock and on its own:
    read_s        reading the file once in 64 MB pieces (the page cache is warm: the file was just written)
    scan_s        plink_scan of all individuals in file order (file -> pinned buffer -> device -> transcode + counts), twice
    scan_rows_s   plink_scan with a shuffled half of the individuals (the gather path)
    commit_output_s  plink_commit_output of that scan: the half becomes the packed output rows of the committed training storage (the load
                  of output rows is scan_rows_s + commit_output_s)
    qc_s          the host's quality control on the counts (streaming._marker_summaries)
    commit_qc_s   plink_commit of the markers that pass it (allocation + compaction)
    commit_all_s  plink_commit of every marker (the staging buffer becomes the storage)
    write_s       the equivalent backend read back with get_packed2bit and written (not a leg of the load; it makes the next one possible)
    load_jgb2_s   load_jgb2 of that backend: the same payload bytes through the same pinned path -- the floor of scan_s, twice
    host_s        (--legs host) prepare_streaming_genotypes(matrix) of the same genotypes on the host
One JSON line on stdout, and --out FILE.  With --p 600000 --n 50000 the file has 7.5 GB; the script refuses a size for which
`--dir` lacks 2.2 x the file's bytes."""
import argparse
import json
import os
import shutil
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402
from jwas_jl_amd import streaming as S  # noqa: E402
from jwas_jl_amd import plink as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--unique", type=int, default=1024)
ap.add_argument("--legs", default="device")
ap.add_argument("--dir", default="/tmp")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p, U = args.n, args.p, min(args.unique, args.p)
legs = set(args.legs.split(","))
stride = (n + 3) // 4
file_bytes = 3 + p * stride
work = os.path.join(args.dir, f"plink_bench_{os.getpid()}")
res = {"n": n, "p": p, "file_bytes": file_bytes, "unique_rows": U}
free = shutil.disk_usage(args.dir).free
if free < 2.2 * file_bytes:
    res["skipped"] = f"{args.dir} has {free / 1e9:.1f} GB free; {2.2 * file_bytes / 1e9:.1f} GB are needed"
    print(json.dumps(res))
    sys.exit(0)
os.makedirs(work)
t_of = {}


def timed(name, f):
    t0 = time.perf_counter()
    out = f()
    t_of.setdefault(name, []).append(time.perf_counter() - t0)
    return out


try:
    # ---- the fileset: U distinct rows as .bed fields (0 = hom A1, 1 = missing, 2 = het, 3 = hom A2), tiled
    rng = np.random.default_rng(2026)
    f = rng.uniform(0.05, 0.5, U)
    a1 = rng.binomial(2, f[:, None], size=(U, n)).astype(np.uint8)                   # copies of A1
    a1[::97] = 0                                                                      # monomorphic rows: quality control drops them
    fields = np.array([3, 2, 0], dtype=np.uint8)[a1]
    fields[rng.random((U, n)) < 0.03] = 1
    padded = np.zeros((U, stride * 4), dtype=np.uint8)
    padded[:, :n] = fields
    q = padded.reshape(U, stride, 4)
    pool = np.ascontiguousarray(q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6))
    bfile = os.path.join(work, "g")
    with open(bfile + ".bed", "wb") as fh:
        fh.write(bytes([0x6C, 0x1B, 0x01]))
        for j0 in range(0, p, U):
            fh.write(pool[:min(U, p - j0)].tobytes())
    with open(bfile + ".fam", "w") as fh:
        fh.write("".join(f"f{i} i{i} 0 0 0 -9\n" for i in range(n)))
    with open(bfile + ".bim", "w") as fh:
        fh.write("".join(f"1\tm{j}\t0\t{j}\tA\tC\n" for j in range(p)))
    assert os.path.getsize(bfile + ".bed") == file_bytes

    def read_file():
        buf = bytearray(64 << 20)
        with open(bfile + ".bed", "rb", buffering=0) as fh:
            while fh.readinto(buf):
                pass

    timed("read_s", read_file)
    if "device" in legs:
        eng = J.HipEngine(0)
        marker_all = P.read_bim(bfile + ".bim")[0]
        counts = timed("scan_s", lambda: eng.plink_scan(bfile + ".bed", n, p))
        cnt = counts[:, 0] + counts[:, 1] + counts[:, 2]
        s1 = (counts[:, 1] + 2 * counts[:, 2]).astype(np.float64)
        s2 = (counts[:, 1] + 4 * counts[:, 2]).astype(np.float64)
        assert int(counts.sum()) == n * p and np.array_equal(counts[:U, 3], (fields == 1).sum(axis=1))
        selected, mean, afreq, xp = timed("qc_s", lambda: S._marker_summaries(cnt, s1, s2, n, True, 0.01, True, marker_all))
        timed("commit_qc_s", lambda: eng.plink_commit(selected, mean, True))
        res["p_selected"] = int(selected.size)
        half = np.random.default_rng(1).permutation(n)[:n // 2]
        timed("scan_rows_s", lambda: eng.plink_scan(bfile + ".bed", n, p, half))
        timed("commit_output_s", lambda: eng.plink_commit_output(selected))      # that half as packed output rows beside the training storage
        assert eng.n_out == half.size
        timed("scan_s", lambda: eng.plink_scan(bfile + ".bed", n, p))
        sel_all, mean_all, afreq_all, xp_all = S._marker_summaries(cnt, s1, s2, n, False, 0.01, True, marker_all)
        timed("commit_all_s", lambda: eng.plink_commit(sel_all, mean_all, True))
        backend = {"nObs": n, "nMarkers": p, "stride_bytes": stride, "nMarkersAll": p, "selected": sel_all, "marker_means": mean_all,
                   "allele_freq": afreq_all, "xpRinvx": xp_all, "centered": True, "obsID": P.read_fam(bfile + ".fam"),
                   "markerID_all": marker_all}
        prefix = timed("write_s", lambda: P.write_streaming_backend(eng, backend, os.path.join(work, "eq")))
        for _ in range(2):
            timed("load_jgb2_s", lambda: eng.load_jgb2(prefix))
        eng.close()
        res["scan_over_load_jgb2"] = min(t_of["scan_s"]) / min(t_of["load_jgb2_s"])
        res["scan_GBps"] = file_bytes / min(t_of["scan_s"]) / 1e9
        res["load_jgb2_GBps"] = file_bytes / min(t_of["load_jgb2_s"]) / 1e9
        res["read_GBps"] = file_bytes / min(t_of["read_s"]) / 1e9
    if "host" in legs:
        cols = np.arange(p) % U
        M = np.where(fields == 1, 9, np.array([2, 9, 1, 0], dtype=np.uint8)[fields]).astype(np.float32).T       # n x U copies of A1
        G = M[:, cols]
        timed("host_s", lambda: S.prepare_streaming_genotypes(G, os.path.join(work, "host")))
    res.update({k: [round(v, 4) for v in t] for k, t in t_of.items()})
finally:
    shutil.rmtree(work, ignore_errors=True)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")
