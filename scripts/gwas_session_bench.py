"""Window GWAS per saved sample on one MI355X: the per-sample `window_sums` path against the resident GWAS session.
python scripts/gwas_session_bench.py [--n N] [--p P] [--window W] [--samples S] [--reps R] [--legs a,b,c] [--out FILE]

Synthetic genotypes (jwas_hip_synth_genotypes) n x p dense Float32, p / W windows of W markers, S samples at 1 % nonzero
effects plus one with every effect nonzero.  Three legs, alternated in one process, one warm-up pass and R timed passes each;
every call returns its sums to the host, so the host clock around a pass is device-synchronised:
  (a) `window_sums` per sample as `gwas.py` drives it with local_EBV=false, host CSR building included
      (entry points of the commit before the session only: `--legs a` runs on that checkout, the baseline)
  (b) the session, sums only            (c) the session with local EBVs.
Reported: ms per sample (sparse samples; the dense one apart) per pass, median and spread; the bytes the accumulator moves per
sparse sample (read + write of the touched windows' padded columns) and the share of the HBM peak (8 TB/s) that (c) - (b)
implies.  One JSON line on stdout, and --out FILE."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import jwas_jl_amd as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--window", type=int, default=100)
ap.add_argument("--samples", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", default="a,b,c")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p = args.n, args.p
legs = args.legs.split(",")
HBM_PEAK = 8.0e12

e = J.HipEngine(0)
e.alloc_dense(n, p)
e.synth(seed=7, kind=0, center=True)
cs = np.arange(0, p, args.window)
ce = np.minimum(cs + args.window, p)
nwin = cs.size
rng = np.random.default_rng(3)
sparse = []
for _ in range(args.samples):
    a = np.zeros(p, dtype=np.float32)
    nz = np.sort(rng.choice(p, p // 100, replace=False))
    a[nz] = rng.standard_normal(nz.size).astype(np.float32) * 0.05
    sparse.append(a)
dense = (rng.standard_normal(p) * 0.01).astype(np.float32)
dense[dense == 0] = 0.01


def leg_a(a):
    nz = np.flatnonzero(a)
    lo, hi = np.searchsorted(nz, cs), np.searchsorted(nz, ce)
    counts = hi - lo
    wptr = np.concatenate([[0, nz.size], nz.size + np.cumsum(counts)]).astype(np.int32)
    gather = np.concatenate([nz] + [nz[l:h] for l, h in zip(lo, hi) if h > l]) if nz.size else nz
    return e.window_sums(wptr, gather, a[gather])


def leg_session(a):
    nz = np.flatnonzero(a)
    return e.gwas_sample(nz, a[nz])


def one_pass(leg):
    """(ms per sparse sample, ms of the dense sample)"""
    if leg != "a":
        e.gwas_begin(cs, ce, local_ebv=(leg == "c"))
    fn = leg_a if leg == "a" else leg_session
    t0 = time.perf_counter()
    for a in sparse:
        fn(a)
    t1 = time.perf_counter()
    fn(dense)
    t2 = time.perf_counter()
    if leg != "a":
        e.gwas_end()
    return (t1 - t0) * 1e3 / len(sparse), (t2 - t1) * 1e3


# the legs agree before anything is timed: same bits
if "a" in legs and "b" in legs:
    e.gwas_begin(cs, ce, local_ebv=False)
    for a in (sparse[0], dense):
        s0, q0 = leg_a(a)
        s1, q1 = leg_session(a)
        assert np.array_equal(s0, s1) and np.array_equal(q0, q1), "session sums differ from window_sums"
    e.gwas_end()

times = {leg: [] for leg in legs}
for leg in legs:
    one_pass(leg)                                   # warm-up
for _ in range(args.reps):
    for leg in legs:                                # alternated
        times[leg].append(one_pass(leg))

res = {"n": n, "p": p, "nwin": int(nwin), "window": args.window, "samples": args.samples, "nnz_sparse": p // 100, "reps": args.reps}
for leg in legs:
    sp = np.array([t[0] for t in times[leg]]); de = np.array([t[1] for t in times[leg]])
    res[leg] = {"sparse_ms_per_sample": [round(float(v), 4) for v in sp], "sparse_median_ms": round(float(np.median(sp)), 4),
                "sparse_spread_ms": round(float(sp.max() - sp.min()), 4),
                "dense_ms": [round(float(v), 3) for v in de], "dense_median_ms": round(float(np.median(de)), 3)}
if "b" in legs and "c" in legs:
    ld = (n + 255) // 256 * 256
    touched = np.mean([np.count_nonzero(np.add.reduceat(a != 0, cs)) for a in sparse])
    acc_bytes = 2 * 8 * ld * touched                # read + write of every touched window's padded column
    extra_ms = res["c"]["sparse_median_ms"] - res["b"]["sparse_median_ms"]
    res["accumulator"] = {"bytes_per_sparse_sample": int(acc_bytes), "windows_touched": float(touched), "total_bytes": int(8 * ld * nwin),
                          "c_minus_b_ms": round(extra_ms, 4),
                          "fraction_of_hbm_peak": round(acc_bytes / (extra_ms * 1e-3) / HBM_PEAK, 4) if extra_ms > 0 else None}
if hasattr(e, "gwas_geometry") and "b" in legs:
    e.gwas_begin(cs, ce)
    res["geometry"] = e.gwas_geometry()
    e.gwas_end()
e.close()
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
