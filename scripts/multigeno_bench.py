"""What the residual hand-over costs a model with two genotype categories (jwas.jl_amd/multigeno.py) on one MI355X: per-iteration time
of two dense BayesC categories of p / 2 markers each -- hand-over, sweep, hand-over, sweep, as the driver runs them -- against the
single-category sweep on the concatenated n x p matrix with the same fixed block size and hyper-parameters.
    python scripts/multigeno_bench.py [n] [p] [--block B] [--iters K] [--reps R] [--warmup W]
The matrices are generated on the device (column j of the concatenation is column j - p/2 of category 2: synth's marker_offset), so
both arms sweep the same genotypes.  Every sweep ends synchronised with the device, so a host clock around an iteration measures it;
the two arms alternate inside every repeat (R repeats of K iterations each after W warm-up iterations of both), medians and the
range over the repeats are printed as one JSON line.  The hand-over alone: 200 copies back and forth behind one read-back."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import jwas_jl_amd as J

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int, nargs="?", default=20000)
ap.add_argument("p", type=int, nargs="?", default=40000)
ap.add_argument("--block", type=int, default=512)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
n, p, bs = args.n, args.p, args.block
assert p % 2 == 0
h = p // 2
y = np.random.default_rng(1).standard_normal(n).astype(np.float32)
kw = dict(seed=3, vare=np.float32(0.9), var_effect=np.float32(1.0 / (0.05 * 0.4 * p)), pi=0.95)


def engine(ncols, offset):
    e = J.HipEngine(0)
    e.alloc_dense(n, ncols)
    e.synth(11, kind=0, center=True, marker_offset=offset)
    e.setup_blocks(bs, "mfma")
    e.init_state("BayesC")
    return e


one, c1, c2 = engine(p, 0), engine(h, 0), engine(h, h)
assert np.array_equal(one.get_columns(h, 2), c2.get_columns(0, 2))        # the same genotypes in both arms
one.set_residual(y)
c1.set_residual(y)
state = {"owner": c1}


def iter_one(it):
    return one.sweep(iteration=it, **kw)["sweep_ms"]


def iter_two(it):
    ms = 0.0
    for e, off in ((c1, 0), (c2, h)):
        if e is not state["owner"]:
            e.residual_handover(state["owner"])
            state["owner"] = e
        ms += e.sweep(iteration=it, marker_offset=off, **kw)["sweep_ms"]
    return ms


def timed(fn, it0, k):
    dev = 0.0
    t0 = time.perf_counter()
    for it in range(it0, it0 + k):
        dev += fn(it)
    return 1e3 * (time.perf_counter() - t0) / k, dev / k


it = 1
for _ in range(args.warmup):
    iter_one(it); iter_two(it); it += 1
rows = {"one": [], "two": []}
for _ in range(args.reps):
    rows["one"].append(timed(iter_one, it, args.iters))
    rows["two"].append(timed(iter_two, it, args.iters))
    it += args.iters


def summary(v):
    w, d = np.array(v).T
    return {"wall_ms_per_iteration": [float(np.median(w)), float(w.min()), float(w.max())],
            "device_sweep_ms_per_iteration": [float(np.median(d)), float(d.min()), float(d.max())]}


c1.get_residual()
t0 = time.perf_counter()
for _ in range(100):
    c1.residual_handover(c2)
    c2.residual_handover(c1)
c2.get_residual()
hand_us = 1e6 * (time.perf_counter() - t0) / 200
print(json.dumps({"n": n, "p": p, "block": bs, "iters": args.iters, "reps": args.reps, "[median, min, max]": True,
                  "one_category": summary(rows["one"]), "two_categories": summary(rows["two"]),
                  "handover_us": hand_us, "handover_bytes": 4 * ((n + 255) // 256 * 256),
                  "in_model": [float(one.get_state()[2].sum()), float(c1.get_state()[2].sum() + c2.get_state()[2].sum())]}))
for e in (one, c1, c2):
    e.close()
