"""The location-parameter step on one MI355X (csrc/locpar.hpp) against the host step of location_parameters="host".
python scripts/locpar_bench.py [--n 50000] [--steps 50] [--out profiles/locpar.json]

One trait, n records, three models:
  (a) intercept only
  (b) intercept + a 1 000-level fixed factor
  (c) intercept + the factor + an n-level i.i.d. random term (one level per record)
device   jwas_hip_locpar_step, HIP events on the context's stream around the launches of one step (jwas_locpar_stats.step_ms):
         `steps` steps after 5 warm-up steps, median / min / max; Float32 and Float64 contexts
host     the step of location_parameters="host" on the same model: mcmc.host_location_step, the function run_chain itself calls
         (residual to the host, + Xf sol with the dense design matrix of mcmc._design, rhs, mcmc._gibbs, residual back), wall
         clock, for (a) and (b).  For (c) the dense
         n x (n + 1001) design matrix does not fit the host's memory at n = 50 000 (20 GB, and a 20 GB left-hand side): not run.
One JSON line on stdout, and --out FILE (merged into an existing file's other keys)."""
import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402
from jwas_jl_amd import mcmc  # noqa: E402
from jwas_jl_amd.api import Model, ModelTerm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--host-steps", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.n
rng = np.random.default_rng(n)
f1000 = rng.integers(0, 1000, n).astype(np.int32)
fn = rng.permutation(n).astype(np.int32)
y = rng.standard_normal(n)
X = np.asfortranarray(rng.integers(0, 3, (n, 64)).astype(np.float32))
MODELS = {"a_intercept": 1, "b_plus_1000_level_factor": 2, "c_plus_n_level_random_term": 3}


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}


def engine(precision):
    e = J.HipEngine(0, precision=precision)
    e.load_dense(X.astype(e.dtype))
    e.setup_blocks(64, "f64")
    e.init_state("BayesC", 1)
    e.set_residual(y.astype(e.dtype), 0)
    return e


results = {}
for name, nterms in MODELS.items():
    row = {"n": n, "location_parameters": [1, 1001, 1001 + n][nterms - 1]}
    for precision in (32, 64):
        e = engine(precision)
        e.locpar_begin(1)
        e.locpar_add_covariate(0, None)
        if nterms >= 2:
            e.locpar_add_factor(0, f1000, 1000, -1)
        if nterms >= 3:
            e.locpar_add_factor(0, fn, n, 0)
        Gi = [np.array([[2.0]])] if nterms >= 3 else []
        ms = [e.locpar_step(iteration=it, seed=1, vare=1.0, Gi=Gi)["step_ms"] for it in range(1, args.steps + 6)][5:]
        row[f"device_f{precision}"] = stats(ms)
        e.close()
    if nterms <= 2:
        # the step of location_parameters="host", on a Float32 context
        e = engine(32)
        terms = [ModelTerm("y", "intercept")] + ([ModelTerm("y", "f")] if nterms == 2 else [])
        model = Model("y = ...", ["y"], [terms], [], None)
        Xf, _ = mcmc._design(model, pd.DataFrame({"f": f1000}), None)
        w64 = np.ones(n)
        lhs = Xf[0].T @ (w64[:, None] * Xf[0])
        sol = np.zeros(Xf[0].shape[1])
        hrng = np.random.default_rng(1)
        tt = []
        for _ in range(args.host_steps + 1):
            t0 = time.perf_counter()
            mcmc.host_location_step(e, Xf[0], lhs, sol, w64, hrng, 1.0, np.float32)
            tt.append((time.perf_counter() - t0) * 1e3)
        row["host_step"] = stats(tt[1:])
        row["host_design_matrix_bytes"] = int(Xf[0].nbytes)
        e.close()
    else:
        row["host_step"] = None
        row["host_note"] = f"not run: the dense design matrix alone is {8 * n * (n + 1001) / 1e9:.1f} GB"
    results[name] = row
    print(json.dumps({name: row}), file=sys.stderr, flush=True)
out = {"bench": "location-parameter step", "steps": args.steps, "results": results}
print(json.dumps(out))
if args.out:
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            merged = json.load(fh)
    merged.update(out)
    with open(args.out, "w") as fh:
        json.dump(merged, fh, indent=1)
