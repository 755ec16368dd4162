"""Single-step analysis on one MI355X: the imputation on the device (csrc/ssbr.hpp) against the path the package had before it, and one
iteration of the single-step chain against the same chain without the ϵ and J terms.
python scripts/ssbr_bench.py [--founders 1000] [--generations 5] [--per-generation 2200] [--genotyped 3000] [--records 8000]
[--p 20000] [--iterations 30] [--out FILE]

A synthetic pedigree from the generator of the pedigree tests (tests/locpar_ped_reference.py::generate_pedigree: 20 sires per
generation, 10 % unknown dams, parents drawn from all earlier animals), `genotyped` random members with centred 0/1/2 genotypes,
`records` phenotyped members (genotyped or not).
  imputation  single_step.impute_genotypes(geno, ped, ids, engine=...) with solver="host" -- SuperLU solves 1000 markers at a time on
              the host, every imputed chunk is uploaded -- against solver="device": one factorisation goes up, then only the
              g x chunk blocks.  Same inputs, same machine, wall time of the whole call (A-inverse and the factorisation included:
              `setup_s` is their share, measured apart).
  iteration   runMCMC(single_step_analysis=True, pedigree=ped) against runMCMC on the SAME resident imputed matrix with the model
              y = intercept + geno, both with the location parameters on the device: the median wall time of an iteration.
One JSON line on stdout, and --out FILE."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import jwas_jl_amd as J  # noqa: E402
from jwas_jl_amd import api, ssbr  # noqa: E402
from jwas_jl_amd import single_step as SS  # noqa: E402
from locpar_ped_reference import generate_pedigree  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--founders", type=int, default=1000)
ap.add_argument("--generations", type=int, default=5)
ap.add_argument("--per-generation", type=int, default=2200)
ap.add_argument("--genotyped", type=int, default=3000)
ap.add_argument("--records", type=int, default=8000)
ap.add_argument("--p", type=int, default=20000)
ap.add_argument("--iterations", type=int, default=30)
ap.add_argument("--out", default="")
args = ap.parse_args()

rng = np.random.default_rng(2026)
t0 = time.perf_counter()
ped = SS.Pedigree(*generate_pedigree(args.founders, args.generations, args.per_generation, 20, 0.1, seed=2026))
gen_ids = sorted(rng.choice(ped.ids, args.genotyped, replace=False).tolist(), key=ped.index.get)
rec_ids = rng.choice(ped.ids, args.records, replace=False).tolist()
p = args.p
G = rng.binomial(2, rng.uniform(0.1, 0.5, p), size=(len(gen_ids), p)).astype(np.float32)
with contextlib.redirect_stdout(io.StringIO()):
    geno = api.get_genotypes(G, 1.0, method="BayesC", Pi=0.99, quality_control=False)
geno.obsID = list(gen_ids)
t_data = time.perf_counter() - t0
t0 = time.perf_counter()
non, gen, Ai_nn, Ai_ng = ssbr.pedigree_blocks(ped, gen_ids)
lu = ssbr.factorize(Ai_nn)
setup_s = time.perf_counter() - t0
nnz_lu = int(lu.L.nnz + lu.U.nnz)

times = {}
hip = J.HipEngine(0)
for solver in ("host", "device"):
    t0 = time.perf_counter()
    imputed = SS.impute_genotypes(geno, ped, rec_ids, engine=hip, solver=solver, **({} if solver == "host" else dict(markers_per_chunk=8192)))
    times[solver] = time.perf_counter() - t0
    if solver == "host":
        check = hip.get_columns(0, 64)
d = float(np.abs(hip.get_columns(0, 64) - check).max())          # the two paths agree to Float32 rounding

# one iteration: the chain on the resident matrix without ϵ and J, then the single-step analysis itself
ph = pd.DataFrame({"ID": rec_ids, "y": rng.standard_normal(len(rec_ids))})
kw = dict(chain_length=args.iterations, burnin=0, seed=1, output_samples_frequency=args.iterations, printout_model_info=False)


def per_iteration(out):
    ends = np.asarray(out["_timing"]["iteration_end_s"])
    return float(np.median(np.diff(ends)))


with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
    model = api.build_model("y = intercept + geno", genotypes={"geno": imputed})
    plain = per_iteration(api.runMCMC(model, ph, location_parameters="device", output_folder=os.path.join(tmp, "plain"), **kw))
    hip.close()
    model = api.build_model("y = intercept + geno", genotypes={"geno": geno})
    t0 = time.perf_counter()
    out = api.runMCMC(model, ph, single_step_analysis=True, pedigree=ped, output_folder=os.path.join(tmp, "ss"), **kw)
    ss_total = time.perf_counter() - t0
    single = per_iteration(out)

res = {"bench": "single-step analysis", "pedigree": len(ped.ids), "non_genotyped": len(non), "genotyped": len(gen), "records": len(rec_ids), "p": p,
       "nnz_L_plus_U": nnz_lu, "nnz_Ai_nn": int(Ai_nn.nnz), "setup_s": round(setup_s, 3), "impute_host_s": round(times["host"], 3),
       "impute_device_s": round(times["device"], 3), "impute_speedup": round(times["host"] / times["device"], 2), "max_abs_difference": d,
       "iteration_plain_ms": round(1e3 * plain, 3), "iteration_single_step_ms": round(1e3 * single, 3), "single_step_run_s": round(ss_total, 2),
       "data_s": round(t_data, 2)}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
