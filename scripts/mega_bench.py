"""The mega-trait sweep (csrc/mega.hpp) on one MI355X against what a user could do before it: the 4-trait JWAS_HIP_MEGABAYESC sweep
run T / 4 times over the same data.  python scripts/mega_bench.py [--n 20000] [--p 100000] [--traits 4,8,16,32,64]
[--blocks 64,128,256] [--warmup 2] [--repeats 5] [--pi 0.95] [--f64] [--out FILE]

Synthetic centred 0/1/2 genotypes: `--unique` distinct columns drawn on the host and tiled to p (what a sweep costs does not depend
on the values; tiling keeps the host's share of the run short).  T phenotypes with 0.1 % causal markers each, pi fixed (0.95: a
sparse chain; 0: RR-BLUP, every marker changes in every sweep).  Per (T, block): `warmup` sweeps, then the median device time
(jwas_mega_stats.step_ms, HIP events on the context's stream) of `repeats` sweeps, and from the shapes
    x_bytes = element bytes * ld * p * ceil(T / 8)   (every trait tile of 8 reads the block's genotypes; + one column per change)
    flops   = 2 * ld * p * T                         (the block right-hand sides X_b'R)
The yardstick is the parent capability, not the new code: the existing sweep with method MegaBayesC, 4 traits, at the block size
the chain driver picks for that prior (512 sparse, 128 dense), its median sweep_ms times T / 4.  ratio = that / the session's time
(> 1: the session is faster).  One JSON line on stdout, and --out FILE."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--traits", default="4,8,16,32,64")
ap.add_argument("--blocks", default="64,128,256")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pi", type=float, default=0.95)
ap.add_argument("--unique", type=int, default=2048)
ap.add_argument("--f64", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p = args.n, args.p
traits = [int(v) for v in args.traits.split(",")]
blocks = [int(v) for v in args.blocks.split(",")]
Tmax = max(traits + [4])
rng = np.random.default_rng(2026)
nu = min(args.unique, p)
base = rng.binomial(2, rng.uniform(0.1, 0.4, nu), size=(n, nu)).astype(np.float64)
base -= base.mean(axis=0)
cols = np.arange(p) % nu
Y = np.empty((Tmax, n))
for k in range(Tmax):
    causal = rng.choice(p, max(p // 1000, 1), replace=False)
    u = base[:, cols[causal]] @ (0.3 * rng.standard_normal(causal.size))
    Y[k] = u / max(u.std(), 1e-9) * np.sqrt(0.5) + rng.standard_normal(n) * np.sqrt(0.5)
ld = (n + 255) // 256 * 256
dtype = np.float64 if args.f64 else np.float32
esize = np.dtype(dtype).itemsize
X = np.empty((n, p), dtype=dtype, order="F")
for j0 in range(0, p, nu):
    j1 = min(p, j0 + nu)
    X[:, j0:j1] = base[:, :j1 - j0]
vare = 0.5
var_effect = 0.5 / (0.001 * p * 0.4)

eng = J.HipEngine(0, precision=64 if args.f64 else 32)
eng.load_dense(X)
del X
results = {"n": n, "p": p, "pi": args.pi, "storage": "Float64" if args.f64 else "Float32", "warmup": args.warmup, "repeats": args.repeats, "unique_columns": nu}

# ---- the yardstick: the existing 4-trait MegaBayesC sweep (a Float32 context only: constraint=true is not in the Float64 path)
old = None
if not args.f64:
    bs_old = 512 if args.pi >= 0.5 else 128
    t0 = time.perf_counter()
    eng.setup_blocks(bs_old)
    setup_ms = (time.perf_counter() - t0) * 1e3
    eng.init_state("MegaBayesC", 4)
    for k in range(4):
        eng.set_residual(Y[k].astype(np.float32), k)
    ms = []
    for it in range(1, args.warmup + args.repeats + 1):
        st = eng.sweep(iteration=it, seed=3, vare=np.eye(4) * vare, var_effect=np.eye(4) * var_effect, pi=np.full(4, args.pi))
        ms.append(st["sweep_ms"])
    old = {"block": bs_old, "setup_blocks_ms": setup_ms, "sweep_ms": ms, "steady_sweep_ms": float(np.median(ms[args.warmup:])),
           "x_gbps": esize * ld * p / float(np.median(ms[args.warmup:])) / 1e6}
    results["megabayesc_4_traits"] = old

rows = []
for bs in blocks:
    for T in traits:
        t0 = time.perf_counter()
        eng.mega_begin(T, bs, 0)
        setup_ms = (time.perf_counter() - t0) * 1e3
        eng.mega_set_residual(Y[:T])
        ms, changed = [], []
        for it in range(1, args.warmup + args.repeats + 1):
            st = eng.mega_sweep(iteration=it, seed=3, vare=np.full(T, vare), var_effect=np.full(T, var_effect), pi=np.full(T, args.pi))
            ms.append(st["step_ms"])
            changed.append(float(st["n_changed"].sum()))
        eng.mega_end()
        med = float(np.median(ms[args.warmup:]))
        row = {"T": T, "block": bs, "setup_ms": setup_ms, "step_ms": ms, "steady_step_ms": med, "ms_per_trait_sweep": med / T,
               "changed_per_sweep": float(np.median(changed[args.warmup:])), "x_bytes": esize * ld * p * ((T + 7) // 8), "flops": 2 * ld * p * T,
               "x_gbps": esize * ld * p * ((T + 7) // 8) / med / 1e6, "gflops": 2 * ld * p * T / med / 1e6,
               "session_bytes": J.HipEngine.mega_estimate_bytes(n, p, T, bs)}
        if old is not None:
            row["old_path_ms"] = old["steady_sweep_ms"] * T / 4
            row["ratio_old_over_new"] = row["old_path_ms"] / med
        rows.append(row)
        print(f"# T={T} block={bs}: {med:.2f} ms per sweep, {med / T:.3f} per trait-sweep"
              + (f", old path x T/4 {row['old_path_ms']:.2f} ms, ratio {row['ratio_old_over_new']:.2f}" if old else ""), file=sys.stderr, flush=True)
results["mega"] = rows
eng.close()
line = json.dumps(results)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
