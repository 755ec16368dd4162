"""K chains of one model in one device session (chains.py, csrc/mega.hpp) on one MI355X against what a user could do before it: K
separate runs on the single-trait sweep.  python scripts/chains_bench.py [--n 20000] [--p 100000] [--chains 2,4,8,16,64]
[--block 256] [--warmup 2] [--repeats 5] [--part both|yardstick|chains] [--yardstick FILE] [--out FILE]

Synthetic centred 0/1/2 genotypes as scripts/mega_bench.py builds them (`--unique` distinct columns tiled to p), Float32, ONE phenotype
with 0.1 % causal markers.  Two methods with fixed hyper-parameters: BayesC with pi = 0.95, and BayesR with the default gamma and
pi = (0.95, 0.03, 0.015, 0.005), which keeps about 5 % of the markers in the model (the measured fraction is reported).  Per (method,
K): `warmup` sweeps from the starting state, then the median device time (step_ms, HIP events on the context's stream) of `repeats`
sweeps.
The yardstick is the parent capability, not the new code: one sweep of the existing single-trait path for the same method at the
block size the single-chain driver picks (mcmc.pick_block_size from the changes of the sweep before: 512 or 1024), its median
sweep_ms times K.  ratio = that / the session's time (> 1: the session is faster).  --part yardstick measures only that (it runs on
a checkout without the session's new entry points, and --out FILE keeps it); --part chains --yardstick FILE reads it back.  There is
no pass mark.  One JSON line on stdout, and --out FILE."""
import argparse
import json
import os
import sys

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402
from jwas_jl_amd.mcmc import BAYESR_GAMMA, pick_block_size  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--chains", default="2,4,8,16,64")
ap.add_argument("--block", type=int, default=256)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--unique", type=int, default=2048)
ap.add_argument("--part", default="both", choices=("both", "yardstick", "chains"))
ap.add_argument("--yardstick", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p = args.n, args.p
chains = [int(v) for v in args.chains.split(",")]
rng = np.random.default_rng(2026)
nu = min(args.unique, p)
base = rng.binomial(2, rng.uniform(0.1, 0.4, nu), size=(n, nu)).astype(np.float64)
base -= base.mean(axis=0)
cols = np.arange(p) % nu
causal = rng.choice(p, max(p // 1000, 1), replace=False)
u = base[:, cols[causal]] @ (0.3 * rng.standard_normal(causal.size))
y = u / max(u.std(), 1e-9) * np.sqrt(0.5) + rng.standard_normal(n) * np.sqrt(0.5)
X = np.empty((n, p), dtype=np.float32, order="F")
for j0 in range(0, p, nu):
    j1 = min(p, j0 + nu)
    X[:, j0:j1] = base[:, :j1 - j0]
vare = 0.5
PI_C, PI_R = 0.95, np.array([0.95, 0.03, 0.015, 0.005])
var_c = 0.5 / (0.001 * p * 0.4)                                          # the causal markers' share of the genetic variance
var_r = var_c / float((BAYESR_GAMMA * PI_R).sum()) * (1.0 - PI_C)        # sigma2 with the same genetic variance (genetic2marker)
nsweeps = args.warmup + args.repeats

eng = J.HipEngine(0, precision=32)
eng.load_dense(X)
del X
results = {"n": n, "p": p, "storage": "Float32", "block": args.block, "warmup": args.warmup, "repeats": args.repeats, "unique_columns": nu,
           "pi_bayesc": PI_C, "pi_bayesr": PI_R.tolist()}


def single_trait(method, bs):
    eng.setup_blocks(bs)
    eng.init_state(method)
    eng.set_residual(y.astype(np.float32))
    if method == "BayesR":
        eng.set_state(delta=np.ones(p, dtype=np.int32))
    ms, events = [], []
    for it in range(1, nsweeps + 1):
        if method == "BayesR":
            st = eng.sweep(iteration=it, seed=3, vare=np.float32(vare), var_effect=np.float32(var_r), pi_classes=PI_R)
        else:
            st = eng.sweep(iteration=it, seed=3, vare=np.float32(vare), var_effect=np.float32(var_c), pi=PI_C)
        ms.append(st["sweep_ms"])
        events.append(float(st["n_events"]))
    return {"block": bs, "sweep_ms": ms, "steady_sweep_ms": float(np.median(ms[args.warmup:])), "events_per_sweep": float(np.median(events[args.warmup:]))}


# ---- the yardstick: one chain on the existing single-trait sweep, at both block sizes of the adaptive policy
yard = None
if args.part in ("both", "yardstick"):
    yard = {}
    for method in ("BayesC", "BayesR"):
        runs = {bs: single_trait(method, bs) for bs in (512, 1024)}
        pick = pick_block_size(runs[512]["events_per_sweep"], p)
        yard[method] = {"picked_block": pick, "steady_sweep_ms": runs[pick]["steady_sweep_ms"], "runs": list(runs.values())}
        print(f"# single-trait {method}: {runs[512]['steady_sweep_ms']:.2f} ms at 512, {runs[1024]['steady_sweep_ms']:.2f} ms at 1024 "
              f"({runs[512]['events_per_sweep']:.0f} changes per sweep: the driver picks {pick})", file=sys.stderr, flush=True)
elif args.yardstick:
    with open(args.yardstick) as fh:
        yard = json.loads(fh.readline())["single_trait"]
results["single_trait"] = yard

# ---- K chains in one session
rows = []
if args.part in ("both", "chains"):
    for method in ("BayesC", "BayesR"):
        for K in chains:
            eng.mega_begin(K, args.block, 0)
            eng.mega_set_residual(np.tile(y, (K, 1)))
            ms, changed, in_model = [], [], []
            for it in range(1, nsweeps + 1):
                if method == "BayesR":
                    st = eng.mega_sweep_r(iteration=it, seed=3, vare=np.full(K, vare), var_effect=np.full(K, var_r), gamma=BAYESR_GAMMA, pi=PI_R)
                    in_model.append(float(st["nnz"].mean()) / p)
                else:
                    st = eng.mega_sweep(iteration=it, seed=3, vare=np.full(K, vare), var_effect=np.full(K, var_c), pi=np.full(K, PI_C))
                    in_model.append(float(st["sum_delta"].mean()) / p)
                ms.append(st["step_ms"])
                changed.append(float(st["n_changed"].mean()))
            eng.mega_end()
            med = float(np.median(ms[args.warmup:]))
            row = {"method": method, "K": K, "step_ms": ms, "steady_step_ms": med, "ms_per_chain_sweep": med / K,
                   "changed_per_chain_sweep": float(np.median(changed[args.warmup:])), "fraction_in_model": float(np.median(in_model[args.warmup:]))}
            if yard is not None:
                row["sequential_ms"] = yard[method]["steady_sweep_ms"] * K
                row["ratio_sequential_over_session"] = row["sequential_ms"] / med
            rows.append(row)
            print(f"# {method} K={K}: {med:.2f} ms per sweep, {med / K:.3f} per chain-sweep, {100 * row['fraction_in_model']:.1f} % in the model"
                  + (f"; K sequential sweeps {row['sequential_ms']:.2f} ms, ratio {row['ratio_sequential_over_session']:.2f}" if yard else ""),
                  file=sys.stderr, flush=True)
results["chains"] = rows
eng.close()
line = json.dumps(results)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
