"""The random-regression sweep (csrc/rrm.hpp) on one MI355X: ms per sweep, genotype bytes over time and the set-up time of the Gram
tensor.  python scripts/rrm_bench.py [--n 20000] [--p 50000] [--T 10] [--c 3] [--block 64] [--sweeps 8] [--skip-mt2] [--out FILE]

Synthetic centred 0/1/2 genotypes: `--unique` distinct columns drawn on the host and tiled to p (what a sweep costs does not depend
on the values; tiling keeps the host's share of the run short).  Records: T time points, Legendre Phi, a phenotype with 0.1 % causal
markers; run once with every record present and once with `--missing` of them absent.  The prior puts 0.95 on the empty state, so
the first sweep starts from every marker in the model (delta = 1: every marker changes) and the later ones are sparse; every sweep's
device time (jwas_rrm_stats.step_ms), wall clock and number of changed markers are reported, and
    x_gbps = element bytes * ld * p / step time      (X is read once per sweep, plus once per changed column)
    setup_ms = the wall clock of rrm_begin           (O, M_j and the block Gram tensor: O(p b n c (c + 1) / 2))
Float32 storage by default (`--f64`: a Float64 context).  Unless --skip-mt2, the nearest existing path on the same build follows: the
Float64 multi-trait sampler-II sweep (csrc/f64_path.hpp) at the same n, p and t = c -- the same state count, Float64 genotypes.
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
from jwas_jl_amd.rrm import generatefullPhi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000)
ap.add_argument("--p", type=int, default=50000)
ap.add_argument("--T", type=int, default=10)
ap.add_argument("--c", type=int, default=3)
ap.add_argument("--block", type=int, default=64)
ap.add_argument("--sweeps", type=int, default=8)
ap.add_argument("--missing", type=float, default=0.2)
ap.add_argument("--unique", type=int, default=2048)
ap.add_argument("--f64", action="store_true")
ap.add_argument("--skip-mt2", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
n, p, T, c = args.n, args.p, args.T, args.c
rng = np.random.default_rng(2026)
nu = min(args.unique, p)
f = rng.uniform(0.1, 0.4, nu)
base = rng.binomial(2, f, size=(n, nu)).astype(np.float64)
base -= base.mean(axis=0)
cols = np.arange(p) % nu
Phi = generatefullPhi(np.arange(T), c)
causal = rng.choice(p, max(p // 1000, 1), replace=False)
a_true = 0.3 * rng.standard_normal((causal.size, c))
u = np.zeros((n, T))
for k, j in enumerate(causal):
    u += np.outer(base[:, cols[j]], Phi @ a_true[k])
y = (u / max(u.std(), 1e-9) * np.sqrt(0.5) + rng.standard_normal((n, T)) * np.sqrt(0.5)).T      # T x n
ld = (n + 255) // 256 * 256


def tiled(dtype):
    X = np.empty((n, p), dtype=dtype, order="F")
    for j0 in range(0, p, nu):
        j1 = min(p, j0 + nu)
        X[:, j0:j1] = base[:, :j1 - j0]
    return X


def rrm_run(eng, missing, esize):
    obs = np.random.default_rng(5).random((T, n)) >= missing
    obs[0, ~obs.any(axis=0)] = True
    t0 = time.perf_counter()
    eng.rrm_begin(Phi, obs, args.block)
    setup_ms = (time.perf_counter() - t0) * 1e3
    eng.rrm_set_residual(np.where(obs, y, 0.0))
    G = (0.5 / (0.001 * p * 0.4)) * (0.8 * np.eye(c) + 0.2)
    lp = np.log(np.full(1 << c, 0.05 / ((1 << c) - 1)))
    lp[0] = np.log(0.95)
    rows = []
    for it in range(1, args.sweeps + 1):
        t0 = time.perf_counter()
        st = eng.rrm_sweep(iteration=it, seed=3, vare=0.5, G=G, log_pi=lp)
        wall = (time.perf_counter() - t0) * 1e3
        rows.append({"step_ms": st["step_ms"], "wall_ms": wall, "n_changed": st["n_changed"], "x_gbps": esize * ld * p / st["step_ms"] / 1e6})
    eng.rrm_end()
    tail = rows[len(rows) // 2:]
    return {"missing": missing, "records": int(obs.sum()), "setup_ms": setup_ms, "sweeps": rows,
            "steady_step_ms": float(np.median([r["step_ms"] for r in tail])), "steady_x_gbps": float(np.median([r["x_gbps"] for r in tail])),
            "gram_bytes": 8 * ((p + args.block - 1) // args.block) * args.block ** 2 * c * (c + 1) // 2,
            "session_bytes": J.HipEngine.rrm_estimate_bytes(n, p, T, c, args.block)}


results = {"n": n, "p": p, "T": T, "c": c, "block": args.block, "storage": "Float64" if args.f64 else "Float32", "unique_columns": nu}
dtype = np.float64 if args.f64 else np.float32
eng = J.HipEngine(0, precision=64 if args.f64 else 32)
X = tiled(dtype)
eng.load_dense(X)
del X
results["rrm"] = [rrm_run(eng, m, np.dtype(dtype).itemsize) for m in (0.0, args.missing)]
eng.close()

if not args.skip_mt2:
    bs = min(512, 2048 // c)
    e = J.HipEngine(0, precision=64)
    X = tiled(np.float64)
    e.load_dense(X)
    del X
    t0 = time.perf_counter()
    e.setup_blocks(bs)
    mt_setup = (time.perf_counter() - t0) * 1e3
    e.init_state("MTBayesC_II", c)
    for k in range(c):
        e.set_residual(y[min(k, T - 1)], k)
        e.set_state(k, delta=np.ones(p))
    R = 0.5 * np.eye(c) + 0.1
    G = (0.5 / (0.001 * p * 0.4)) * (0.8 * np.eye(c) + 0.2)
    lp = np.log(np.full(1 << c, 0.05 / ((1 << c) - 1)))
    lp[0] = np.log(0.95)
    rows = []
    for it in range(1, args.sweeps + 1):
        t0 = time.perf_counter()
        st = e.sweep(iteration=it, seed=3, vare=R, var_effect=G, log_prior_states=lp)
        rows.append({"sweep_ms": st["sweep_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3, "n_events": st["n_events"],
                     "x_gbps": 8 * ld * p / st["sweep_ms"] / 1e6})
    e.close()
    tail = rows[len(rows) // 2:]
    results["f64_sampler2"] = {"traits": c, "block": bs, "setup_blocks_ms": mt_setup, "sweeps": rows,
                               "steady_sweep_ms": float(np.median([r["sweep_ms"] for r in tail])),
                               "steady_x_gbps": float(np.median([r["x_gbps"] for r in tail]))}

line = json.dumps(results)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
