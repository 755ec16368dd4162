"""GBLUP on one MI355X (csrc/gblup.hpp): the relationship matrix, the eigendecomposition and the pseudo-marker step.
python scripts/gblup_bench.py [--grm-n 20000] [--grm-p 100000] [--eigen 5000] [--steps 5000,20000,40000] [--traits 1,4]
[--warmup 2] [--repeats 5] [--rounds 2] [--pause 5] [--f64] [--skip grm,eigen,step,cpu] [--out FILE]

GRM: genotypes synthesised on the device (what the kernel costs does not depend on the values), divisor 0.65.  jwas_hip_grm returns K
on the host, so a call is timed by the wall clock and includes the n x n copy; the same call with p = 1024 markers carries the same
copy and allocation, and the difference of the two medians over the difference in work, 2 n (n + tile) (p - 1024) / 2 flop on the
tiles on or below the diagonal, is the kernel's rate -- against the 155 TF/s measured f32-MFMA peak.
Eigendecomposition: numpy.linalg.eigh on the 16 usable cores against gblup.eigh_device (torch.linalg.eigh in a child process, solved
in Float64; its wall time includes starting that process and the two transfers) on a random relationship matrix.
Step: L = a column-tiled random matrix with entries N(0, 1 / n) (not orthogonal: the time does not depend on it; alpha and the residual
are reset before every repeat so nothing overflows).  step_ms (HIP events around the six launches) against the byte model
3 n^2 sizeof(real) at 6.6 TB/s (the streaming rate of the README's headline) and against the numpy restatement of the same step
(three gemv-shaped products, T columns) on the machine's 16 usable cores.
Every figure: `warmup` calls first, the median and the spread (min .. max) of `repeats`, the whole measurement repeated `rounds` times
with `pause` seconds between.  One JSON line on stdout, and --out FILE."""
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
from jwas_jl_amd import gblup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grm-n", type=int, default=20000)
ap.add_argument("--grm-p", type=int, default=100000)
ap.add_argument("--eigen", default="5000")
ap.add_argument("--steps", default="5000,20000,40000")
ap.add_argument("--traits", default="1,4")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--pause", type=float, default=5.0)
ap.add_argument("--f64", action="store_true")
ap.add_argument("--skip", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
skip = set(v for v in args.skip.split(",") if v)
dtype = np.float64 if args.f64 else np.float32
esize = np.dtype(dtype).itemsize
precision = 64 if args.f64 else 32
STREAM_TBS, MFMA_PEAK_TF = 6.6, 155.0


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


res = {"precision": precision, "rounds": args.rounds, "grm": "not measured", "eigen": "not measured", "step": "not measured"}

if "grm" not in skip:
    n, p, p0 = args.grm_n, args.grm_p, 1024
    tile = 64 if args.f64 else 128
    rounds = []
    for rd in range(args.rounds):
        one = {}
        for pp in (p0, p):
            e = J.HipEngine(0, precision=precision)
            if args.f64:
                rng = np.random.default_rng(1)
                base = rng.binomial(2, 0.3, size=(n, 256)).astype(np.float64)
                e.load_dense(np.asfortranarray(np.tile(base - base.mean(axis=0), (1, -(-pp // 256)))[:, :pp]))
            else:
                e.alloc_dense(n, pp)
                e.synth(7)
            d = np.full(pp, 0.65, dtype=dtype)
            one[pp] = stats(timed(lambda: e.grm(d), 1, args.repeats))
            e.close()
        flop = 2.0 * n * (n + tile) / 2 * (p - p0)
        dt_ = one[p]["median"] - one[p0]["median"]
        rounds.append({"wall_s": one[p], "wall_s_p1024": one[p0], "kernel_s_by_difference": dt_, "tflops": flop / dt_ / 1e12,
                       "of_mfma_peak": flop / dt_ / 1e12 / MFMA_PEAK_TF})
        time.sleep(args.pause)
    res["grm"] = {"n": n, "p": p, "rounds": rounds}

if "eigen" not in skip:
    out = []
    for n in [int(v) for v in args.eigen.split(",") if v]:
        rng = np.random.default_rng(n)
        Z = rng.standard_normal((n, 2 * n)).astype(dtype)
        K = ((Z @ Z.T) / dtype(2 * n) + np.eye(n, dtype=dtype) * dtype(1e-5)).astype(dtype)
        K = ((K + K.T) / dtype(2)).astype(dtype)
        host = stats(timed(lambda: gblup.eigh_host(K), 0, max(1, args.repeats // 2)))
        try:
            dev = stats(timed(lambda: gblup.eigh_device(K, 0), 1, max(1, args.repeats // 2)))
        except RuntimeError as ex:
            dev = f"not measured ({ex})"
        out.append({"n": n, "host_s": host, "device_s": dev})
    res["eigen"] = out

if "step" not in skip:
    out = []
    for n in [int(v) for v in args.steps.split(",") if v]:
        rng = np.random.default_rng(n)
        nu = min(512, n)
        base = (rng.standard_normal((n, nu)) / np.sqrt(n)).astype(dtype)
        L = np.empty((n, n), dtype=dtype, order="F")
        for j0 in range(0, n, nu):
            L[:, j0:min(n, j0 + nu)] = base[:, :min(n, j0 + nu) - j0]
        D = np.linspace(1e-3, 3.0, n)
        for T in [int(v) for v in args.traits.split(",")]:
            vare = np.eye(T) * 0.5 + 0.1
            G = np.eye(T) * 0.4 + 0.05
            r0 = rng.standard_normal((T, n)).astype(dtype)
            e = J.HipEngine(0, precision=precision)
            e.load_dense(L)
            e.init_state("BayesC" if T == 1 else "MTBayesC", T)
            e.gblup_begin(D)

            def one(it):
                for k in range(T):
                    e.set_residual(r0[k], k)
                    e.set_state(k, alpha=np.zeros(n, dtype=dtype))
                e.gblup_step(iteration=it, seed=1, vare=vare, G=G, diagonal=False)       # (alpha = 0 costs what any alpha costs)
                return e.gblup_step(iteration=it + 1, seed=1, vare=vare, G=G, diagonal=False)["step_ms"]
            rounds = []
            for rd in range(args.rounds):
                for w in range(args.warmup):
                    one(1)
                rounds.append(stats([one(3 + 2 * i) for i in range(args.repeats)]))
                time.sleep(args.pause)
            e.close()
            model_ms = 3.0 * n * n * esize / (STREAM_TBS * 1e12) * 1e3
            row = {"n": n, "traits": T, "step_ms": rounds, "byte_model_ms": model_ms, "of_byte_model": model_ms / rounds[0]["median"]}
            if "cpu" not in skip:
                L64 = L            # (the reference's BLAS calls run in the element type)
                A0, R0 = np.zeros((T, n), dtype=dtype), r0.copy()

                def cpu():
                    rp = R0 + A0 @ L64.T
                    s = rp @ L64
                    a = (s / (1.0 + 1.0 / D)).astype(dtype)
                    return rp - a @ L64.T
                row["numpy_16_cores_ms"] = stats([1e3 * v for v in timed(cpu, 1, max(2, args.repeats // 2))])
                row["speedup_over_numpy"] = row["numpy_16_cores_ms"]["median"] / rounds[0]["median"]
            out.append(row)
        del L
    res["step"] = out

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
