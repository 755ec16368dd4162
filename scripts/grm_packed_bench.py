"""The relationship matrix from 2-bit packed storage against the dense kernel, one MI355X (csrc/gblup.hpp: k_grm_packed, k_grm<float>).
python scripts/grm_packed_bench.py [--n 20000] [--p 100000] [--warmup 2] [--repeats 5] [--rounds 2] [--pause 5] [--out FILE]

The protocol of scripts/gblup_bench.py's GRM part, for jwas_hip_grm_packed2bit and jwas_hip_grm in the same run on the same card:
genotypes synthesised on the device in either storage (what the kernels cost does not depend on the values), divisor 0.65.  Both calls
return K on the host, so a call is timed by the wall clock and includes the n x n copy; the same call with 1 024 markers carries the
same copy and allocation, and the difference of the two medians over the difference in work, 2 n (n + 128) (p - 1024) / 2 flop on the
tiles on or below the diagonal, is the kernel's rate -- against the 155 TF/s measured f32-MFMA peak.  `warmup` calls first, the median
and the spread (min .. max) of `repeats`, the whole measurement repeated `rounds` times with `pause` seconds between.  One JSON line on
stdout, and --out FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--pause", type=float, default=5.0)
ap.add_argument("--out", default="")
args = ap.parse_args()
MFMA_PEAK_TF, TILE, P0 = 155.0, 128, 1024


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def measure(storage, n, p):
    """Wall seconds of the storage's relationship-matrix call at 1 024 and at p markers, and the kernel by difference."""
    one = {}
    for pp in (P0, p):
        e = J.HipEngine(0)
        (e.alloc_packed if storage == "packed2bit" else e.alloc_dense)(n, pp)
        e.synth(7)
        d = np.full(pp, 0.65, dtype=np.float32)
        call = e.grm_packed if storage == "packed2bit" else e.grm
        one[pp] = stats(timed(lambda: call(d), args.warmup, args.repeats))
        one[pp]["storage_bytes"] = e.storage_info()["bytes"]
        e.close()
    flop = 2.0 * n * (n + TILE) / 2 * (p - P0)
    dt = one[p]["median"] - one[P0]["median"]
    return {"wall_s": one[p], "wall_s_p1024": one[P0], "kernel_s_by_difference": dt, "tflops": flop / dt / 1e12,
            "of_mfma_peak": flop / dt / 1e12 / MFMA_PEAK_TF}


rounds = []
for rd in range(args.rounds):
    row = {s: measure(s, args.n, args.p) for s in ("packed2bit", "dense_f32")}
    row["kernel_s_packed_over_dense"] = row["packed2bit"]["kernel_s_by_difference"] / row["dense_f32"]["kernel_s_by_difference"]
    rounds.append(row)
    time.sleep(args.pause)
line = json.dumps({"n": args.n, "p": args.p, "warmup": args.warmup, "repeats": args.repeats, "rounds": rounds})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
