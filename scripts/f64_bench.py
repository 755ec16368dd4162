"""Throughput of the Float64 context (runMCMC(double_precision=true)) on one MI355X: sweeps over a synthetic n x p matrix of
doubles.  python scripts/f64_bench.py [n] [p] [--method M[,M...]] [--traits T[,T...]] [--sweeps K]
  --method BayesC (default; Float64 against Float32), or the multi-trait kinds, Float64 only:
           MT1 (BayesC, sampler I), MT2 (BayesC, sampler II), MTB1 / MTB2 (BayesB, sampler I / II: one covariance per marker,
           redrawn on the device every sweep -- wall_ms includes that draw)
           outputs: the output side of a Float64 run, ms per saved sample and trait at ~1 % and at 100 % nonzero effects:
           (a) the host product X_out @ alpha (numpy / BLAS on the cores this process may use), (b) k64_mul_alpha, the loop
           over all p markers (reached through residual_sub_xalpha + a residual read-back of n doubles), (c) compact + list:
           mul_alpha on the training matrix and mul_alpha_output on n/2 output rows; and the sample readout, sparse against
           get_state + flatnonzero.  Medians of --reps calls after 3 warm-up calls, one process, one device."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import jwas_jl_amd as J

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int, nargs="?", default=20000)
ap.add_argument("p", type=int, nargs="?", default=20000)
ap.add_argument("--method", default="BayesC")
ap.add_argument("--traits", default="2")
ap.add_argument("--sweeps", type=int, default=20)
ap.add_argument("--reps", type=int, default=11)
args = ap.parse_args()
n, p = args.n, args.p
rng = np.random.default_rng(1)
f = rng.uniform(0.1, 0.4, p)
X = np.empty((n, p), dtype=np.float64, order="F")
for j0 in range(0, p, 2000):
    j1 = min(p, j0 + 2000)
    X[:, j0:j1] = rng.binomial(2, f[j0:j1], size=(n, j1 - j0))
X -= X.mean(axis=0)
beta = np.zeros(p); q = rng.choice(p, p // 1000, replace=False); beta[q] = rng.standard_normal(q.size)
g = X @ beta
y = g / g.std() * np.sqrt(0.5) + rng.standard_normal(n) * np.sqrt(0.5)
MT_KINDS = {"MT1": "MTBayesC", "MT2": "MTBayesC_II", "MTB1": "MTBayesB", "MTB2": "MTBayesB_II"}


def bench_mt(kind, t):
    """ms per sweep of a t-trait Float64 chain (blocks of JWAS_F64_BLOCK markers, default 512)."""
    bs = int(os.environ.get("JWAS_F64_BLOCK", "0")) or min(512, 2048 // t)
    e = J.HipEngine(0, precision=64)
    e.load_dense(X)
    e.setup_blocks(bs)
    e.init_state(MT_KINDS[kind], t)
    rng_t = np.random.default_rng(7)
    for k in range(t):
        e.set_residual((1 + 0.2 * k) * (y - y.mean()) + 0.5 * rng_t.standard_normal(n), k)
        e.set_state(k, delta=np.ones(p))
    R = 0.5 * np.eye(t) + 0.1
    G = (0.5 / (0.05 * (2 * f * (1 - f)).sum())) * (0.8 * np.eye(t) + 0.2)
    lp = np.log(np.full(1 << t, 0.05 / ((1 << t) - 1))); lp[0] = np.log(0.95)
    ms, wall = [], []
    for it in range(1, args.sweeps + 1):
        kw = dict(iteration=it, seed=3, vare=R, var_effect=G, log_prior_states=lp)
        t0 = time.time()
        if kind.startswith("MTB"):
            if it == 1:
                kw["var_effect_matrix"] = np.tile(G, (p, 1, 1))
            else:
                e.sample_marker_covariances(t + 4.0, G * 4.0, seed=3, iteration=it - 1)
        st = e.sweep(**kw)
        wall.append(1e3 * (time.time() - t0))
        ms.append(st["sweep_ms"])
    e.close()
    return {"block": bs, "sweep_ms_last10": float(np.mean(ms[-10:])), "wall_ms_last10": float(np.mean(wall[-10:])),
            "state_counts": [float(v) for v in st["state_counts"]]}


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def bench_outputs():
    rows = np.random.default_rng(5).permutation(n)[:n // 2]
    X_out_host = np.asarray(X[rows, :], dtype=np.float64)          # what run_chain kept on the host before the output rows were resident
    e = J.HipEngine(0, precision=64)
    e.load_dense(X)
    e.init_state("BayesC", 1)
    res = {"n_out": int(rows.size), "reps": args.reps, "blas_threads": os.environ.get("OMP_NUM_THREADS", "unset")}
    e.load_output_dense(X_out_host)
    rng_a = np.random.default_rng(11)
    for tag, nnz in (("1pct", max(1, p // 100)), ("100pct", p)):
        a = np.zeros(p)
        a[rng_a.choice(p, nnz, replace=False)] = rng_a.standard_normal(nnz) * 0.01
        e.set_state(alpha=a)
        r = {"nnz": nnz}
        r["a_host_product_ms"] = median_ms(lambda: X_out_host @ e.get_state()[0], args.reps)
        e.set_residual(np.zeros(n))
        r["b_all_markers_loop_ms"] = median_ms(lambda: (e.sub_xalpha(), e.get_residual()), args.reps)
        r["c_list_training_ms"] = median_ms(lambda: e.mul_alpha(), args.reps)
        r["c_list_output_ms"] = median_ms(lambda: e.mul_alpha_output(), args.reps)
        r["sparse_readout_ms"] = median_ms(lambda: e.alpha_sparse(), args.reps)
        assert np.array_equal(e.mul_alpha_output(), e.mul_alpha()[rows])
        r["dense_readout_ms"] = median_ms(lambda: np.flatnonzero(e.get_state()[0]), args.reps)
        res[tag] = r
        print(json.dumps({tag: r}), flush=True)
    e.close()
    return res


out = {}
if args.method == "outputs":
    X = np.asfortranarray(X)
    print(json.dumps({"n": n, "p": p, "outputs [median, min, max] ms": bench_outputs()}))
    sys.exit(0)
if args.method != "BayesC":
    X = np.asfortranarray(X)
    for kind in args.method.split(","):
        for t in (int(v) for v in args.traits.split(",")):
            out[f"{kind}_t{t}"] = bench_mt(kind, t)
            print(json.dumps({f"{kind}_t{t}": out[f"{kind}_t{t}"]}), flush=True)
    print(json.dumps({"n": n, "p": p, **out}))
    sys.exit(0)
for prec in (64, 32):
    e = J.HipEngine(0, precision=prec)
    dt = np.float64 if prec == 64 else np.float32
    e.load_dense(np.asfortranarray(X, dtype=dt))
    t0 = time.time(); e.setup_blocks(int(os.environ.get("JWAS_F64_BLOCK", "512")) if prec == 64 else 512, "mfma"); setup = time.time() - t0
    e.init_state("BayesC", 1); e.set_residual((y - y.mean()).astype(dt))
    pi, ms = 0.95, []
    for it in range(1, 41):
        st = e.sweep(iteration=it, seed=3, vare=dt(0.5), var_effect=dt(0.5 / (0.05 * (2 * f * (1 - f)).sum())), pi=pi)
        pi = float(np.clip(1.0 - (st["sum_delta"][0] + 1.0) / (p + 2.0), 0.5, 0.9999))
        ms.append(st["sweep_ms"])
    out[f"f{prec}"] = {"sweep_ms_last10": float(np.mean(ms[-10:])), "setup_s": setup, "in_model": float(st["sum_delta"][0]),
                       "GBps_last10": (8 if prec == 64 else 4) * n * p / 1e6 / float(np.mean(ms[-10:]))}
    e.close()
print(json.dumps({"n": n, "p": p, **out}))
