"""The step of a pedigree random effect on one MI355X (csrc/locpar.hpp, k_locpar_draw_structured) against the same step with an
i.i.d. random term of as many levels, in the same run on the same build.
python scripts/locpar_ped_bench.py [--n 50000] [--steps 50] [--out profiles/locpar_ped.json]

n records; a generated pedigree (500 founders, 6 generations of (n - 1500) / 6 + ... animals, 20 sires per generation, 10 % unknown
dams, parents drawn from all earlier animals so that inbreeding occurs); per trait an intercept and the animal term.
  structured   set_random(model, "animal", ped, G): A-inverse uploaded with locpar_set_group_structure, sampled colour by colour
  iid          the same levels as an i.i.d. random term (the yardstick)
One trait and three, Float32 and Float64 contexts.  jwas_locpar_stats.step_ms (HIP events on the context's stream around the
launches of one step): `steps` steps after 5 warm-up steps, median / min / max, for the whole step and for the animal terms alone.
One JSON line on stdout, and --out FILE (merged into an existing file's other keys)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import jwas_jl_amd as J  # noqa: E402
from jwas_jl_amd import api  # noqa: E402
from jwas_jl_amd.single_step import Pedigree  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.n
rng = np.random.default_rng(n)
founders, gens, sires = 500, 6, 20
per_gen = max(1, (n - 1500) // gens)
sire, dam = [-1] * founders, [-1] * founders
for _ in range(gens):
    born = len(sire)
    pool = rng.choice(born, size=sires, replace=False)
    sire += [int(v) for v in rng.choice(pool, size=per_gen)]
    dam += [int(v) for v in np.where(rng.random(per_gen) < 0.1, -1, rng.integers(0, born, per_gen))]
ped = Pedigree([f"a{i}" for i in range(len(sire))], sire, dam)
V = api.pedigree_structure(ped)
q = V.shape[0]
level = rng.integers(0, q, n).astype(np.int32)
X = np.asfortranarray(rng.integers(0, 3, (n, 64)).astype(np.float32))
rows = np.diff(V.indptr)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}


results = {}
ncolors = None
for t in (1, 3):
    for precision in (32, 64):
        row = {}
        for kind in ("structured", "iid"):
            e = J.HipEngine(0, precision=precision)
            e.load_dense(X.astype(e.dtype))
            e.setup_blocks(64, "f64")
            e.init_state("BayesC" if t == 1 else "MTBayesC", t)
            for k in range(t):
                e.set_residual(rng.standard_normal(n).astype(e.dtype), k)
            e.locpar_begin(t)
            if kind == "structured":
                e.locpar_set_group_structure(0, V.indptr, V.indices, V.data)
                ncolors = int(e.locpar_group_colors(0).max()) + 1
            for k in range(t):
                e.locpar_add_covariate(k, None)
                e.locpar_add_factor(k, level, q, 0)
            kw = dict(vare=1.0) if t == 1 else dict(Rinv=np.eye(t))
            Gi = [np.eye(t) * 2.0]
            whole = [e.locpar_step(iteration=it, seed=1, Gi=Gi, **kw)["step_ms"] for it in range(1, args.steps + 6)][5:]
            terms = []                                     # the animal terms alone: every second term of the scan
            for it in range(args.steps + 6, 2 * args.steps + 11):
                terms.append(sum(e.locpar_step(iteration=it, seed=1, Gi=Gi, first_term=2 * k + 1, last_term=2 * k + 2, **kw)["step_ms"] for k in range(t)))
            row[kind] = {"whole_step": stats(whole), "animal_terms_alone": stats(terms[5:])}
            e.close()
        row["structured_over_iid_whole_step"] = row["structured"]["whole_step"]["median_ms"] / row["iid"]["whole_step"]["median_ms"]
        results[f"t{t}_f{precision}"] = row
        print(json.dumps({f"t{t}_f{precision}": row}), file=sys.stderr, flush=True)
out = {"bench": "pedigree random effect step", "steps": args.steps, "n": n, "animals": q, "nnz": int(V.nnz), "colours": ncolors,
       "longest_row": int(rows.max()), "mean_row": float(rows.mean()), "rows_longer_than_32": int((rows > 32).sum()), "results": results}
print(json.dumps(out))
if args.out:
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            merged = json.load(fh)
    merged.update(out)
    with open(args.out, "w") as fh:
        json.dump(merged, fh, indent=1)
