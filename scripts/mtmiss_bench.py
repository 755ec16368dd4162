"""Multi-trait records that miss some traits on one MI355X (csrc/mtmiss.hpp, the per-record-weight instantiations of csrc/locpar.hpp).
python scripts/mtmiss_bench.py [--n 50000] [--steps 50] [--out profiles/mtmiss.json]

t = 3 traits, n records, 20 % of them incomplete; per trait an intercept, a 1 000-level fixed factor and an n-level i.i.d. random
term (one level per record).  Float32 and Float64 contexts:
  impute          one jwas_hip_mtmiss_impute (two table uploads and the kernel): HIP events recorded on the context's stream around
                  the call, and the call's wall clock
  weighted_step   one jwas_hip_locpar_step under per-record weights (jwas_locpar_stats.step_ms: HIP events around its launches)
  plain_step      the same step with kron(inv(R), diag(w)) -- the <false> instantiations, the code of the parent commit -- on the
                  same model with complete records
  host_round_trip what the host path does per iteration for the same data: get_residual x t, mcmc._impute_missing_residuals,
                  set_residual x t (wall clock)
`steps` repetitions after 5 warm-up ones, median / min / max.  One JSON line on stdout, and --out FILE."""
import argparse
import ctypes as C
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402
from jwas_jl_amd import _lib, mcmc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default="")
args = ap.parse_args()
n, t = args.n, 3
rng = np.random.default_rng(n)
f1000 = rng.integers(0, 1000, n).astype(np.int32)
fn = rng.permutation(n).astype(np.int32)
X = np.asfortranarray(rng.integers(0, 3, (n, 64)).astype(np.float32))
r0 = rng.standard_normal((t, n))
full = (1 << t) - 1
codes = np.where(rng.random(n) < 0.2, rng.integers(1, full, n), full).astype(np.int32)
observed = np.array([(codes >> k) & 1 for k in range(t)], dtype=bool).T
A = rng.standard_normal((t, t))
R0 = A @ A.T / t + np.eye(t)
R0 = (R0 + R0.T) / 2
Rinv = np.linalg.inv(R0)
Rinv = (Rinv + Rinv.T) / 2
B, U, Ctab = mcmc.missing_pattern_tables(R0)
Gi = [np.linalg.inv(R0 * 0.5)]
Gi = [(Gi[0] + Gi[0].T) / 2]


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}


def hip_runtime():
    """The HIP runtime the library itself has loaded (events on the context's stream have to come from the same runtime)."""
    _lib.load()
    with open("/proc/self/maps") as fh:
        paths = {ln.split()[-1] for ln in fh if "libamdhip64" in ln}
    H = C.CDLL(sorted(paths)[0])
    H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    H.hipEventSynchronize.argtypes = [C.c_void_p]
    H.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return H


def engine(precision):
    e = J.HipEngine(0, precision=precision)
    e.load_dense(X.astype(e.dtype))
    e.setup_blocks(64, "f64")
    e.init_state("MTBayesC", t)
    for k in range(t):
        e.set_residual(r0[k].astype(e.dtype), k)
    e.locpar_begin(t)
    for k in range(t):
        e.locpar_add_covariate(k, None)
        e.locpar_add_factor(k, f1000, 1000, -1)
        e.locpar_add_factor(k, fn, n, 0)
    return e


H = None
results = {"n": n, "traits": t, "incomplete_records": int((codes != full).sum()), "location_parameters": t * (1001 + n)}
for precision in (32, 64):
    row = {}
    e = engine(precision)
    if H is None:
        H = hip_runtime()
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert H.hipStreamCreate(C.byref(stream)) == 0 and H.hipEventCreate(C.byref(ev0)) == 0 and H.hipEventCreate(C.byref(ev1)) == 0
    e.set_stream(stream.value)
    # the plain step on complete records (no codes at all: the state of the parent commit)
    ms = [e.locpar_step(iteration=it, seed=1, Rinv=Rinv, Gi=Gi)["step_ms"] for it in range(1, args.steps + 6)][5:]
    row["plain_step"] = stats(ms)
    e.mtmiss_begin(codes)
    dev, wall = [], []
    for it in range(1, args.steps + 6):
        t0 = time.perf_counter()
        H.hipEventRecord(ev0, stream)
        e.mtmiss_impute(iteration=it, seed=1, B=B, U=U)
        H.hipEventRecord(ev1, stream)
        H.hipEventSynchronize(ev1)
        wall.append((time.perf_counter() - t0) * 1e3)
        el = C.c_float()
        H.hipEventElapsedTime(C.byref(el), ev0, ev1)
        dev.append(el.value)
    row["impute"] = stats(dev[5:])
    row["impute_wall"] = stats(wall[5:])
    e.mtmiss_set_record_weights(Ctab)
    ms = [e.locpar_step(iteration=it, seed=1, Gi=Gi)["step_ms"] for it in range(1, args.steps + 6)][5:]
    row["weighted_step"] = stats(ms)
    row["weighted_over_plain"] = row["weighted_step"]["median_ms"] / row["plain_step"]["median_ms"]
    # the host path's round trip
    hrng = np.random.default_rng(1)
    tt = []
    for _ in range(min(args.steps, 10) + 2):
        t0 = time.perf_counter()
        res = [e.get_residual(k).astype(np.float64) for k in range(t)]
        mcmc._impute_missing_residuals(res, observed, R0, hrng)
        for k in range(t):
            e.set_residual(res[k].astype(e.dtype), k)
        tt.append((time.perf_counter() - t0) * 1e3)
    row["host_round_trip"] = stats(tt[2:])
    e.close()
    results[f"f{precision}"] = row
    print(json.dumps({f"f{precision}": row}), file=sys.stderr, flush=True)
out = {"bench": "missing-trait records: imputation and the record-weighted step", "steps": args.steps, "results": results}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
