"""EBVs of 2-bit packed output rows on one MI355X (jwas_hip_ebv_output, csrc/output.hpp k_ebv_packed): wall clock of one saved
sample's EBVs, three legs.    python scripts/plink_output_bench.py [--n 100000] [--p 100000] [--mode full|parent] [--out FILE]

The genotypes are synthesised on the device into packed storage (jwas_hip_synth_genotypes); the SAME individuals then become the
packed output rows (the payload read back and loaded with load_output_packed2bit), so the three legs do the same arithmetic:
    a  ebv_output()                        all t traits, one launch of k_ebv_packed on the output rows
    b  mul_alpha_output(k), k = 0 .. t-1   k_mul_alpha_list / k_mul_alpha <PackedCols> on the output rows, one trait at a time
    c  mul_alpha(k), k = 0 .. t-1          the same kernels on the packed TRAINING storage: --mode parent runs this leg alone and
                                           uses only entry points older than the packed output rows (the baseline of an older library)
Cases: t = 1 and 3, 5 % and 100 % nonzero effects (each trait its own random 5 %).  Per case and leg: `--warmup` calls, then
`--repeats` timed calls, the legs alternating inside every repeat; a call ends with its results on the host, so the clock stops
behind a device synchronise.  Reported: the median, the minimum and the maximum of the repeats in ms, the bytes of genotype payload
the leg's kernels read (marker rows of ld / 4 bytes: a, the union of the traits' nonzero markers once; b and c, every trait's own) and
that over the median as a fraction of 8 TB/s -- an end-to-end figure of the call (allocation, list compaction, copy back included),
not a kernel's.  a and b are checked for equal bits in every case.  One JSON line on stdout, and --out FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--mode", default="full", choices=["full", "parent"])
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p = args.n, args.p
ld = (n + 255) // 256 * 256
res = {"n": n, "p": p, "mode": args.mode, "warmup": args.warmup, "repeats": args.repeats, "marker_row_bytes": ld // 4, "cases": []}

eng = J.HipEngine(0)
eng.alloc_packed(n, p, centered=True)
eng.synth(2026, kind=0, center=True)
if args.mode == "full":
    t0 = time.perf_counter()
    step = max(1, (256 << 20) // (ld // 4))
    payload = np.concatenate([eng.get_packed2bit(j0, min(step, p - j0)) for j0 in range(0, p, step)])
    res["read_back_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    eng.load_output_packed2bit(payload, n)
    res["load_output_packed2bit_s"] = round(time.perf_counter() - t0, 3)
    del payload


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def summary(ms, nbytes):
    med = float(np.median(ms))
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "bytes": int(nbytes),
            "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


rng = np.random.default_rng(7)
for t in (1, 3):
    for share in (0.05, 1.0):
        A = np.zeros((t, p), dtype=np.float32)
        for k in range(t):
            nz = np.arange(p) if share == 1.0 else np.sort(rng.permutation(p)[:int(share * p)])
            A[k, nz] = (0.01 * rng.standard_normal(nz.size)).astype(np.float32) + np.float32(1e-3)
        eng.init_state("BayesC" if t == 1 else "MTBayesC", t)
        for k in range(t):
            eng.set_state(k, alpha=A[k])
        legs = {"c": lambda: [eng.mul_alpha(k) for k in range(t)]}
        if args.mode == "full":
            legs = {"a": eng.ebv_output, "b": lambda: [eng.mul_alpha_output(k) for k in range(t)], "c": legs["c"]}
        for _ in range(args.warmup):
            last = {name: f() for name, f in legs.items()}
        ms = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, f in legs.items():
                last[name], dt = timed(f)
                ms[name].append(dt)
        per_trait = sum(int(np.count_nonzero(A[k])) for k in range(t)) * (ld // 4)
        union = int(np.count_nonzero(np.any(A != 0, axis=0))) * (ld // 4)
        case = {"t": t, "nonzero_share": share, "c": summary(ms["c"], per_trait)}
        if args.mode == "full":
            case["a"], case["b"] = summary(ms["a"], union), summary(ms["b"], per_trait)
            case["a_equals_b"] = bool(all(np.array_equal(last["a"][k], last["b"][k]) for k in range(t)))
            case["b_equals_c"] = bool(all(np.array_equal(last["b"][k], last["c"][k]) for k in range(t)))
            case["b_spread_ms"] = round(max(ms["b"]) - min(ms["b"]), 3)
            case["a_beats_b_by_more_than_the_spread"] = bool(case["b"]["median_ms"] - case["a"]["median_ms"] > case["b_spread_ms"])
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
eng.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")
