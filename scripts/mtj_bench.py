"""The joint multi-trait sweep of 5 to 8 traits (csrc/mtjoint.hpp: Gibbs sampler I, full G and R, Pi over 2^t states) on one MI355X,
with the mega-trait session's sweep (csrc/mega.hpp: t independent chains, diagonal covariances) at the same t beside it for context.
python scripts/mtj_bench.py [--n 20000] [--p 100000] [--traits 5,8] [--block 256] [--warmup 2] [--repeats 5] [--f64] [--out FILE]

Synthetic centred 0/1/2 genotypes as scripts/mega_bench.py: `--unique` distinct columns drawn on the host and tiled to p.  t correlated
phenotypes with 0.1 % causal markers.  Two priors per t: "sparse", Pi with 0.95 on the all-zero state and the rest spread evenly over
the other states, and "rrblup", all mass on the all-ones state (every marker changes in every sweep).  Per (t, prior): `warmup`
sweeps, then the median device time (jwas_mtj_stats.step_ms, HIP events on the context's stream) of `repeats` sweeps.  The mega-trait
session runs the same t traits with pi = 0.95 (sparse) and pi = 0 (rrblup) per trait.  Nothing ran this model on the device before:
the numbers are first measurements, not a comparison with a parent.  One JSON line on stdout, and --out FILE."""
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
from jwas_jl_amd.mtjoint import inv_gauss_jordan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--traits", default="5,8")
ap.add_argument("--block", type=int, default=256)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--unique", type=int, default=2048)
ap.add_argument("--f64", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p, bs = args.n, args.p, args.block
traits = [int(v) for v in args.traits.split(",")]
Tmax = max(traits)
rng = np.random.default_rng(2026)
nu = min(args.unique, p)
base = rng.binomial(2, rng.uniform(0.1, 0.4, nu), size=(n, nu)).astype(np.float64)
base -= base.mean(axis=0)
cols = np.arange(p) % nu
causal = rng.choice(p, max(p // 1000, 1), replace=False)
mix = np.eye(Tmax) + 0.3 * np.tril(rng.uniform(-1, 1, (Tmax, Tmax)), -1)
Ug = mix @ (0.3 * rng.standard_normal((Tmax, causal.size))) @ base[:, cols[causal]].T
Y = Ug / np.maximum(Ug.std(axis=1, keepdims=True), 1e-9) * np.sqrt(0.5) + (mix @ rng.standard_normal((Tmax, n))) * np.sqrt(0.5)
ld = (n + 255) // 256 * 256
dtype = np.float64 if args.f64 else np.float32
esize = np.dtype(dtype).itemsize
X = np.empty((n, p), dtype=dtype, order="F")
for j0 in range(0, p, nu):
    j1 = min(p, j0 + nu)
    X[:, j0:j1] = base[:, :j1 - j0]
vare0 = 0.5 * (mix @ mix.T)
G0 = (0.5 / (0.001 * p * 0.4)) * (mix @ mix.T)

eng = J.HipEngine(0, precision=64 if args.f64 else 32)
eng.load_dense(X)
del X
results = {"n": n, "p": p, "block": bs, "storage": "Float64" if args.f64 else "Float32", "warmup": args.warmup, "repeats": args.repeats, "unique_columns": nu}
rows = []
for T in traits:
    ns = 1 << T
    sparse = np.full(ns, 0.05 / (ns - 1))
    sparse[0] = 0.95
    dense = np.zeros(ns)
    dense[-1] = 1.0
    rinv, ginv = inv_gauss_jordan(vare0[:T, :T]), inv_gauss_jordan(G0[:T, :T])
    for prior, tab, pi_mega in (("sparse", sparse, 0.95), ("rrblup", dense, 0.0)):
        with np.errstate(divide="ignore"):
            lp = np.log(tab)
        eng.mtj_begin(T, bs)
        eng.mtj_set_residual(Y[:T])
        ms, changed = [], []
        for it in range(1, args.warmup + args.repeats + 1):
            st = eng.mtj_sweep(iteration=it, seed=3, rinv=rinv, ginv=ginv, log_pi=lp)
            ms.append(st["step_ms"])
            changed.append(float(st["n_changed"]))
        eng.mtj_end()
        eng.mega_begin(T, bs, 0)
        eng.mega_set_residual(Y[:T])
        mms = []
        for it in range(1, args.warmup + args.repeats + 1):
            st = eng.mega_sweep(iteration=it, seed=3, vare=np.diag(vare0)[:T], var_effect=np.diag(G0)[:T], pi=np.full(T, pi_mega))
            mms.append(st["step_ms"])
        eng.mega_end()
        med, mmed = float(np.median(ms[args.warmup:])), float(np.median(mms[args.warmup:]))
        rows.append({"T": T, "prior": prior, "step_ms": ms, "steady_step_ms": med, "changed_markers_per_sweep": float(np.median(changed[args.warmup:])),
                     "mega_step_ms": mms, "mega_steady_step_ms": mmed, "x_bytes": esize * ld * p, "x_gbps": esize * ld * p / med / 1e6,
                     "flops_rhs": 2 * ld * p * T})
        print(f"# t={T} {prior}: joint session {med:.2f} ms per sweep ({rows[-1]['changed_markers_per_sweep']:.0f} markers change); "
              f"mega-trait session at the same t {mmed:.2f} ms", file=sys.stderr, flush=True)
results["mtj"] = rows
eng.close()
line = json.dumps(results)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
