"""Annotation priors on one MI355X: the host leg of an annotated iteration against the device step (csrc/annot.hpp).
python scripts/annot_bench.py [--n 50000] [--p 600000] [--annotations 8] [--steps 10] [--methods BayesC,BayesR] [--out FILE]

Synthetic 0/1/2 genotypes generated on the device, `annotations` standard-normal annotation columns (the first one 0 / 1), a
phenotype with 1 % causal markers.  Per method, after 3 warm-up iterations, per iteration (median / min / max over `steps`):
  sweep_resident    the sweep reading the session's resident table: jwas_sweep_stats.sweep_ms (device) and the call's wall clock
  sweep_host_table  the same sweep handed the p (x 4) table through the host pointer: wall clock -- the difference is the upload
  get_state         engine.get_state(0)[2]: the indicator download of the host path (wall clock)
  host_update       annotations.update_bayesc_binary_priors / update_bayesr_nested_priors on that vector (wall clock)
  host_leg          get_state + host_update + (sweep_host_table - sweep_resident): what "host" pays between two sweeps; the code
                    of that path is the parent commit's, unchanged
  annot_step        engine.annot_step: jwas_annot_stats.step_ms (device) and the call's wall clock, the download of the
                    coefficients included
One JSON line on stdout, and --out FILE."""
import argparse
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
from jwas_jl_amd import annotations as A_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", type=int, default=600000)
ap.add_argument("--annotations", type=int, default=8)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--block-size", type=int, default=256)
ap.add_argument("--methods", default="BayesC,BayesR")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p = args.n, args.p
rng = np.random.default_rng(p)
ann = rng.standard_normal((p, args.annotations))
ann[:, 0] = (rng.random(p) < 0.2).astype(np.float64)
D = np.hstack([np.ones((p, 1)), ann])


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


eng = J.HipEngine(0)
eng.alloc_dense(n, p)
eng.synth(2026, kind=0, center=True)
eng.setup_blocks(args.block_size, "mfma")
results = {"n": n, "p": p, "annotations": args.annotations, "block_size": args.block_size}
for method in args.methods.split(","):
    eng.init_state(method, 1)
    causal = rng.choice(p, max(p // 100, 1), replace=False)
    a0 = np.zeros(p, dtype=np.float32)
    a0[causal] = rng.standard_normal(causal.size).astype(np.float32) * 0.05
    eng.set_state(0, alpha=a0, beta=a0, delta=np.ones(p, dtype=np.int32 if method == "BayesR" else np.float32))
    g = eng.mul_alpha(0).astype(np.float64)
    y = g + rng.standard_normal(n) * max(g.std(), 1e-3)
    eng.set_state(0, alpha=np.zeros(p, dtype=np.float32), beta=np.zeros(p, dtype=np.float32))
    eng.set_residual((y - y.mean()).astype(np.float32), 0)
    vare, varg = float(y.var() * 0.5), float(y.var() * 0.5 / (0.01 * p * 0.5))
    if method == "BayesR":
        host = A_.MarkerAnnotations(D, nsteps=3, nclasses=4, coefficients=np.zeros((D.shape[1], 3)),
                                    snp_pi=np.tile(np.array([0.95, 0.03, 0.015, 0.005]), (p, 1)))
        table0, kw = host.snp_pi.copy(), dict(vare=vare, var_effect=varg, pi_classes=None)
        key, update = "pi_matrix", A_.update_bayesr_nested_priors
    else:
        host = A_.MarkerAnnotations(D)
        A_.initialize_bayesc_single_trait(host, np.full(p, 0.99))
        table0, kw = np.full(p, 0.99), dict(vare=vare, var_effect=varg)
        key, update = "pi_vec", A_.update_bayesc_binary_priors
    eng.annot_begin(method, D, host.coefficients, host.variance, table0)
    hrng = np.random.default_rng(1)
    rows = {k: [] for k in ("sweep_dev", "sweep_res", "sweep_tab", "get_state", "host_update", "step_dev", "step_wall")}
    var = np.ones(3) if method == "BayesR" else 1.0
    for it in range(1, args.steps + 4):
        st, w = wall(lambda: eng.sweep(iteration=2 * it - 1, seed=7, resident_priors=True, **kw))
        rows["sweep_dev"].append(st["sweep_ms"]); rows["sweep_res"].append(w)
        res, w = wall(lambda: eng.annot_step(iteration=it, seed=7, variance=var))
        rows["step_dev"].append(res["step_ms"]); rows["step_wall"].append(w)
        table = eng.annot_prior()
        eng.annot_end()                                              # the host path: the table goes up with the sweep
        _, w = wall(lambda: eng.sweep(iteration=2 * it, seed=7, **{k_: v_ for k_, v_ in kw.items() if k_ != "pi_classes"}, **{key: table}))
        rows["sweep_tab"].append(w)
        dlt, w = wall(lambda: eng.get_state(0)[2])
        rows["get_state"].append(w)
        _, w = wall(lambda: update(host, dlt, hrng))
        rows["host_update"].append(w)
        eng.annot_begin(method, D, host.coefficients, host.variance, table)
    r = {k: np.array(v[3:]) for k, v in rows.items()}
    upload = np.maximum(r["sweep_tab"] - r["sweep_res"], 0.0)
    out = {"sweep_resident": stats(r["sweep_dev"]), "sweep_resident_wall": stats(r["sweep_res"]), "sweep_host_table_wall": stats(r["sweep_tab"]),
           "get_state": stats(r["get_state"]), "host_update": stats(r["host_update"]),
           "host_leg": stats(r["get_state"] + r["host_update"] + upload),
           "annot_step": stats(r["step_dev"]), "annot_step_wall": stats(r["step_wall"])}
    out["host_leg_over_annot_step_wall"] = out["host_leg"]["median_ms"] / out["annot_step_wall"]["median_ms"]
    eng.annot_end()
    results[method] = out
    print(json.dumps({method: out}), file=sys.stderr, flush=True)
eng.close()
out = {"bench": "annotation priors: host leg against the device step", "steps": args.steps, "results": results}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
