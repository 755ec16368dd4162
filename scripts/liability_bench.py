"""The liability step of threshold / censored traits on one MI355X (csrc/liability.hpp), per call.
python scripts/liability_bench.py [--sizes 50000,280000] [--traits 1,3] [--calls 200] [--reps 5] [--out profiles/liability.json]

For every n and t (t = 1: one 3-category trait; t = 3: 3-category + continuous + censored, 5 Gibbs rounds) three things:
  device   jwas_hip_liability_sample per call: `calls` asynchronous launches closed by one synchronising call, host clock around
           them, one warm-up pass and `reps` timed passes (median and spread); and the whole step of an iteration -- the draw, the
           threshold bounds (jwas_hip_liability_minmax: one launch, one read-back) and the new thresholds
  numpy    the restatement of tests/liability_reference.py on the same inputs (the BLAS / OpenMP pools capped at 16 threads)
  copies   the residual get + set round trip per trait that a host-side step would add to an iteration
Bytes the draw must move per call: every liability trait reads and writes residual and liability, a continuous trait is read,
plus codes (4 B) or bounds (16 B) per record; reported against the 8 TB/s HBM peak.  One JSON line on stdout, and --out FILE."""
import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import jwas_jl_amd as J  # noqa: E402
import liability_reference as LR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="50000,280000")
ap.add_argument("--traits", default="1,3")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--numpy-reps", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
HBM_PEAK = 8.0e12
TH = np.array([-np.inf, 0.0, 0.6, np.inf])


def med(v):
    return {"median_ms": float(np.median(v)) * 1e3, "min_ms": float(np.min(v)) * 1e3, "max_ms": float(np.max(v)) * 1e3}


results = []
for n in [int(v) for v in args.sizes.split(",")]:
    for t in [int(v) for v in args.traits.split(",")]:
        rng = np.random.default_rng(n + t)
        kinds = [LR.CATEGORICAL] if t == 1 else [LR.CATEGORICAL, LR.CONTINUOUS, LR.CENSORED]
        ngibbs = 1 if t == 1 else 5
        A = rng.standard_normal((t, t))
        R = np.array([[1.0]]) if t == 1 else (A @ A.T / t + np.eye(t)) * 0.7
        codes = rng.integers(1, 4, n).astype(np.int32)
        cmean = rng.standard_normal((t, n))
        lo = cmean[t - 1] + rng.uniform(-2, 2, n)
        up = np.where(rng.random(n) < 0.5, np.inf, lo + 1.0)
        row = {"n": n, "traits": t, "ngibbs": ngibbs}
        for precision in (32, 64):
            e = J.HipEngine(0, precision=precision)
            e.load_dense(np.asfortranarray(rng.integers(0, 3, (n, 64)).astype(e.dtype)))
            e.setup_blocks(64, "f64")
            e.init_state("BayesC" if t == 1 else "MTBayesC", t)
            e.liability_begin(t)
            e.set_categorical(0, codes, TH)
            if t == 3:
                e.set_censored(2, lo, up)
            for k in range(t):
                e.set_residual(rng.standard_normal(n) if kinds[k] == LR.CONTINUOUS else e.liabilities(k) - cmean[k], k)
            e.liability_init(seed=1, R=R)
            it = [0]

            def draws():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    it[0] += 1
                    e.liability_sample(iteration=it[0], seed=1, ngibbs=ngibbs, R=R)
                e.set_thresholds(0, TH)                               # synchronises the stream
                return (time.perf_counter() - t0) / args.calls

            def steps():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    it[0] += 1
                    e.liability_sample(iteration=it[0], seed=1, ngibbs=ngibbs, R=R)
                    mx, mn = e.liability_minmax(0)
                    th = TH.copy()
                    th[2] = 0.5 * (mx[2] + mn[2])
                    e.set_thresholds(0, th)
                return (time.perf_counter() - t0) / args.calls

            def copies():
                t0 = time.perf_counter()
                for _ in range(20):
                    for k in range(t):
                        e.set_residual(e.get_residual(k), k)
                return (time.perf_counter() - t0) / 20

            draws(); steps(); copies()
            sz = 8 if precision == 64 else 4
            nbytes = n * sum((4 * sz + (4 if kd == LR.CATEGORICAL else 16)) if kd != LR.CONTINUOUS else sz for kd in kinds)
            d = med([draws() for _ in range(args.reps)])
            row[f"device_f{precision}"] = {"draw": d, "step_with_threshold_update": med([steps() for _ in range(args.reps)]),
                                            "residual_get_set_all_traits": med([copies() for _ in range(args.reps)]),
                                            "draw_bytes": nbytes, "draw_share_of_hbm_peak": nbytes / (d["median_ms"] * 1e-3) / HBM_PEAK}
            e.close()
        # the numpy restatement on the same inputs (Float64)
        y0 = [codes.astype(np.float64), None, np.where(np.isinf(lo), 0.0, lo)][:t] if t == 3 else [codes.astype(np.float64)]
        r0 = np.stack([rng.standard_normal(n) if kinds[k] == LR.CONTINUOUS else y0[k] - cmean[k] for k in range(t)])
        lows, ups = [None] * t, [None] * t
        lows[0], ups[0] = LR.bounds_from_thresholds(TH, codes)
        if t == 3:
            lows[2], ups[2] = lo, up
        tn = []
        for rep in range(args.numpy_reps + 1):
            t0 = time.perf_counter()
            LR.liability_draw(r0, y0, kinds, lows, ups, iteration=rep + 1, seed=1, ngibbs=ngibbs, R=R, init=False, dtype=np.float64)
            tn.append(time.perf_counter() - t0)
        row["numpy_restatement"] = med(tn[1:])
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
out = {"bench": "liability step", "calls_per_pass": args.calls, "reps": args.reps, "results": results}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
