"""The runs of tests/test_chain_output_golden.py: small runMCMC calls on the CPU stand-in engines that together open every kind of
sample file and build every kind of table the four chain drivers know (mcmc.run_chain, multigeno.run_multigeno,
megatrait.run_megatrait, rrm.run_rrm).  tests/golden/make_chain_output_golden.py records what a commit writes for them; the test
replays them and requires equality.

A case is a function of the scratch folder that returns (inputs, run): the generated inputs, whose digest the fixture stores beside
the outputs, and a callable that performs the run and returns runMCMC's dict.  Every case is at most 250 records x 200 markers and at
most 20 iterations, with burnin >= 2 so that unsaved and saved iterations both occur; the shapes are a few dozen records and one or
two dozen markers, since the output layer does nothing that depends on their number."""
import builtins
import contextlib
import hashlib
import io
import os
import sys

import numpy as np
import pandas as pd

from conftest import make_dataset
from jwas_jl_amd import api

VALUE_COLUMNS = ("Estimate", "SD", "EBV", "PEV", "Model_Frequency")
FULL_VALUES = 8


# ---- data of the run_chain cases that have no helper of their own -----------------------------------------------------------------------
def _frames(n=24, p=12, seed=23, missing=False):
    """(genotype frame, phenotype frame): y1, y2, a covariate x1 and a three-level factor herd; `missing` blanks some cells of y2."""
    d = make_dataset(n=n, p=p, ncausal=4, seed=seed, center=False)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(d["raw"], columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    rng = np.random.default_rng(seed + 1)
    ph = pd.DataFrame({"ID": ids, "y1": d["y"], "y2": (0.6 * d["y"] + rng.standard_normal(n)).astype(np.float32),
                       "x1": rng.standard_normal(n), "herd": rng.choice(["a", "b", "c"], n)})
    if missing:
        ph.loc[rng.random(n) < 0.2, "y2"] = np.nan
    return gdf, ph


def _single_trait(tmp, name, engine, *, geno_kw, double=False, ids_out=None, **kw):
    gdf, ph = _frames()
    if ids_out is not None:
        ph = ph.iloc[:20]                                # (the last 4 genotyped individuals have no record)

    def run():
        geno = api.get_genotypes(gdf, double_precision=double, **geno_kw)      # noqa: F841 (build_model finds it)
        model = api.build_model("y1 = intercept + x1 + herd + geno")
        api.set_covariate(model, "x1")
        api.outputMCMCsamples(model, "herd")
        if ids_out is not None:
            api.outputEBV(model, ids_out)
        args = dict(chain_length=14, burnin=2, output_samples_frequency=2, seed=7, double_precision=double,
                    output_folder=str(tmp / name), _engine=engine, block_size=8)
        args.update(kw)
        return api.runMCMC(model, ph, **args)
    return [gdf, ph], run


def _two_traits(tmp, name, *, constraint):
    from oracle_engine import OracleEngine
    gdf, ph = _frames(missing=not constraint)

    def run():
        geno = api.get_genotypes(gdf, method="BayesC", constraint=constraint)      # noqa: F841
        model = api.build_model("y1 = intercept + x1 + geno\ny2 = intercept + geno", constraint=constraint)
        api.set_covariate(model, "x1")
        return api.runMCMC(model, ph, chain_length=14, burnin=2, output_samples_frequency=2, seed=7, output_folder=str(tmp / name),
                           _engine=OracleEngine("block"), block_size=8)
    return [gdf, ph], run


def bayesc(tmp):
    from oracle_engine import OracleEngine
    return _single_trait(tmp, "bayesc", OracleEngine("block"), geno_kw=dict(method="BayesC", Pi=0.8))


def bayesr(tmp):
    from oracle_engine import OracleEngine
    return _single_trait(tmp, "bayesr", OracleEngine("block"), geno_kw=dict(method="BayesR"))


def bayesb(tmp):
    from oracle_engine import OracleEngine
    return _single_trait(tmp, "bayesb", OracleEngine("block"), geno_kw=dict(method="BayesB", Pi=0.8))


def estimate_scale(tmp):
    from oracle_engine import OracleEngine
    return _single_trait(tmp, "scale", OracleEngine("block"), geno_kw=dict(method="BayesC", Pi=0.8, estimate_scale=True))


def two_traits_missing(tmp):
    return _two_traits(tmp, "mt_missing", constraint=False)


def two_traits_constraint(tmp):
    return _two_traits(tmp, "mt_constraint", constraint=True)


IDS_OUT = ["i7", "i21", "i3", "i23", "nobody", "i12"]      # i21 and i23 have no record; nobody has no genotype


def ebv_ids_output_rows(tmp):
    from test_f64_outputs_host import CountingEngine64
    return _single_trait(tmp, "ids_dev", CountingEngine64(), geno_kw=dict(method="BayesC", Pi=0.8), double=True, ids_out=IDS_OUT)


def ebv_ids_host_product(tmp):
    from oracle_engine import OracleEngine64             # (no load_output_dense: the host forms X_out alpha)
    return _single_trait(tmp, "ids_host", OracleEngine64(), geno_kw=dict(method="BayesC", Pi=0.8), double=True, ids_out=IDS_OUT)


def double_precision(tmp):
    from oracle_engine import OracleEngine64
    return _single_trait(tmp, "f64", OracleEngine64(), geno_kw=dict(method="BayesC", Pi=0.8), double=True)


def random_and_pedigree(tmp):
    import test_locpar_ped_host as T
    from locpar_ped_reference import PedOracleEngine
    ped = T._demo_ped()
    model, ph = T._model("y1 = intercept + x1 + x2 + ID + geno")

    def run():
        api.set_covariate(model, "x1")
        api.set_random(model, "x2", 0.6)
        api.set_random(model, "ID", ped, 0.6)
        api.outputMCMCsamples(model, "ID")
        return T._run(model, ph, tmp / "ped", PedOracleEngine("block"), chain_length=16, burnin=4, output_samples_frequency=2)
    return [ph, list(ped.ids), os.path.join(T.DEMO, "genotypes.txt")], run


def categorical(tmp):
    import test_liability_host as T
    from liability_reference import LiabilityOracleEngine
    gdf, ids, g, liab = T._simulate(30, 12, 2, ncausal=6)
    ph = pd.DataFrame({"ID": ids, "y": np.digitize(liab, [-0.6, 0.1, 0.9]) + 1.0})

    def run():
        return T._run(gdf, ph, "y = intercept + geno", tmp / "cat", LiabilityOracleEngine("block"), chain_length=12, burnin=3,
                      categorical_trait=["y"])[1]
    return [gdf, ph], run


def _sem_data():
    return make_dataset(n=24, p=8, ncausal=4, seed=11)


def causal_structure(tmp):
    import sem_reference as SR
    import test_sem_host as T
    data = _sem_data()

    def run():
        return T._run(data, tmp, "sem", chain_length=12, burnin=4, output_samples_frequency=2)[0]
    return list(SR.sem_phenotypes(data, ["a", "b", "c"])), run


def _annotated(tmp, where):
    import test_annot_host as T
    from annot_reference import AnnotOracleEngine
    gdf, ph, ann = T.annotated_data(p=24, n=24)

    def run():
        geno = api.get_genotypes(gdf, method="BayesC", annotations=ann, Pi=0.7)      # noqa: F841
        model = api.build_model("y1 = intercept + geno")
        return api.runMCMC(model, ph, chain_length=14, burnin=2, output_samples_frequency=2, seed=7, output_folder=str(tmp / ("annot_" + where)),
                           _engine=AnnotOracleEngine("block"), block_size=8, annotation_priors=where)
    return [gdf, ph, ann], run


def annotated_host(tmp):
    return _annotated(tmp, "host")


def annotated_device(tmp):
    return _annotated(tmp, "device")


def single_step(tmp):
    import ssbr_reference as SR
    import test_ssbr_host as T
    case = SR.small_case(markers=12, traits=("y",))

    def run():
        return T._run(case, tmp / "ss", traits=["y"], engine=SR.SsOracleEngine(), output_samples_frequency=2)[0]
    return [case["gdf"], case["ph"], list(case["ped"].ids)], run


def _multigeno(tmp, name, traits, build, ph_edit=None, **kw):
    import test_multigeno_host as T
    from multigeno_reference import MultiOracleEngine
    _, g1, g2, ph = T._frames(n=24, p1=8, p2=6, traits=traits)
    if ph_edit is not None:
        ph = ph_edit(ph)

    def run():
        args = dict(chain_length=14, burnin=2, output_samples_frequency=2, seed=6, output_folder=str(tmp / name),
                    _engine=[MultiOracleEngine("block"), MultiOracleEngine("block")], block_size=8)
        args.update(kw)
        return api.runMCMC(build(T, g1, g2), ph, **args)
    return [g1, g2, ph], run


def multigeno_mixed(tmp):
    return _multigeno(tmp, "mg_mixed", 1, lambda T, g1, g2: T.mixed_model(g1, g2))


def multigeno_three_traits(tmp):
    def build(T, g1, g2):
        geno1, geno2 = T._two(g1, g2, dict(method="BayesC"), dict(method="RR-BLUP"))
        geno1.multi_trait_sampler = "II"
        model = api.build_model("y1 = intercept + x1 + geno1 + geno2\ny2 = intercept + geno1 + geno2\ny3 = intercept + geno1 + geno2")
        api.set_covariate(model, "x1")
        return model
    return _multigeno(tmp, "mg_t3", 3, build)


def multigeno_ebv_ids(tmp):
    def build(T, g1, g2):
        geno1, geno2 = T._two(g1, g2, dict(method="BayesC", Pi=0.8))      # noqa: F841 (build_model finds them)
        model = api.build_model("y1 = intercept + geno1 + geno2")
        api.outputEBV(model, ["i7", "i3", "i22", "nobody"])
        return model

    def ph_edit(ph):
        return pd.concat([ph.iloc[:20], pd.DataFrame({"ID": ["nobody"], "y1": [0.3], "x1": [0.0]})], ignore_index=True)
    return _multigeno(tmp, "mg_ids", 1, build, ph_edit, output_samples_frequency=1)


def _megatrait(tmp, name, double):
    import test_megatrait_host as T
    data = T.mega_data(n=16, p=8)

    def run():
        return T.run_mega(tmp, name, data=data, double=double, output_samples_frequency=2,
                          model_edit=lambda model, api_: api_.outputMCMCsamples(model, "age"))
    return list(data), run


def megatrait_f64(tmp):
    return _megatrait(tmp, "mega64", True)


def megatrait_f32(tmp):
    return _megatrait(tmp, "mega32", False)


def _rrm(tmp, name, **kw):
    import test_rrm_host as T
    data = T.rrm_data(n=16, p=8)

    def run():
        return T.run_rrm(tmp, name, data=data, output_samples_frequency=2, **kw)
    return list(data), run


def rrm_default(tmp):
    return _rrm(tmp, "rrm")


def rrm_fixed_pi_no_ebv(tmp):
    return _rrm(tmp, "rrm_fixed", geno_kw=dict(estimatePi=False), outputEBV=False)


CASES = {f.__name__: f for f in (
    bayesc, bayesr, bayesb, estimate_scale, two_traits_missing, two_traits_constraint, ebv_ids_output_rows, ebv_ids_host_product,
    random_and_pedigree, categorical, causal_structure, annotated_host, annotated_device, single_step, double_precision,
    multigeno_mixed, multigeno_three_traits, multigeno_ebv_ids, megatrait_f64, megatrait_f32, rrm_default, rrm_fixed_pi_no_ebv)}


# ---- the drivers of the block sessions (tests/golden/session_driver_golden.json): run_mtjoint, run_chains, and the output rows of
# run_megatrait -------------------------------------------------------------------------------------------------------------------------
IDS_OUT_16 = [f"i{i}" for i in range(9, 16)]             # (with nph = 12: i12 .. i15 have no record)


def _mtjoint(tmp, name, double, data=None, **kw):
    import test_mtj_host as T
    from test_megatrait_host import mega_data
    data = data or mega_data(n=16, p=8, t=5, missing=0.0)

    def run():
        return T.run_joint(tmp, name, data=data, double=double, output_samples_frequency=2, **kw)
    return list(data), run


def mtjoint_f64(tmp):
    return _mtjoint(tmp, "mtj64", True, model_edit=lambda model, api_: api_.outputMCMCsamples(model, "age"))


def mtjoint_f32(tmp):
    return _mtjoint(tmp, "mtj32", False)


def mtjoint_rrblup_ids(tmp):
    from test_megatrait_host import mega_data
    return _mtjoint(tmp, "mtj_rr", True, data=mega_data(n=16, p=8, t=5, nph=12, missing=0.0), geno_kw=dict(method="RR-BLUP"),
                    model_edit=lambda model, api_: api_.outputEBV(model, IDS_OUT_16))


def megatrait_ids_missing(tmp):
    import test_megatrait_host as T
    data = T.mega_data(n=16, p=8, nph=12)

    def run():
        return T.run_mega(tmp, "mega_ids", data=data, output_samples_frequency=2,
                          model_edit=lambda model, api_: api_.outputEBV(model, IDS_OUT_16))
    return list(data), run


def _chains(tmp, name, method, **kw):
    import test_chains_host as T
    data = T.chain_data(n=16, p=8)

    def run():
        return T.run_k(tmp, name, data=data, method=method, output_samples_frequency=2, **kw)
    return list(data), run


def chains_bayesc(tmp):
    return _chains(tmp, "chains_c", "BayesC", chains=3)


def chains_bayesr(tmp):
    return _chains(tmp, "chains_r", "BayesR", chains=2, first_chain=2)


SESSION_DRIVER_CASES = {f.__name__: f for f in (mtjoint_f64, mtjoint_f32, mtjoint_rrblup_ids, megatrait_ids_missing, chains_bayesc, chains_bayesr)}


# ---- recording ---------------------------------------------------------------------------------------------------------------------------
def _sha(data):
    return hashlib.sha256(data).hexdigest()


def inputs_digest(inputs):
    h = hashlib.sha256()
    for obj in inputs:
        if isinstance(obj, pd.DataFrame):
            h.update(obj.to_csv(index=False, float_format="%.17g").encode())
        elif isinstance(obj, np.ndarray):
            h.update(repr((obj.dtype.str, obj.shape)).encode() + np.ascontiguousarray(obj).tobytes())
        elif isinstance(obj, str) and os.path.isfile(obj):
            h.update(open(obj, "rb").read())
        else:
            h.update(repr(obj).encode())
    return h.hexdigest()


@contextlib.contextmanager
def _recorded_prints(chunks):
    """Everything print() sends to standard output, also when a helper redirects standard output for the run."""
    real = builtins.print

    def tee(*args, **kw):
        if kw.get("file") in (None, sys.stdout):
            buf = io.StringIO()
            real(*args, **{**kw, "file": buf})
            chunks.append(buf.getvalue())
        real(*args, **kw)
    builtins.print = tee
    try:
        yield
    finally:
        builtins.print = real


def _table(tab):
    """The columns, and of every value column its dtype and the shortest repr of every value in that dtype -- in full up to
    FULL_VALUES values, else their number and the SHA-256 of the reprs joined by commas (equality of the digest is equality of
    every repr; the fixture stays small enough to be read)."""
    rec = {"columns": [str(c) for c in tab.columns]}
    for col in tab.columns:
        if col in VALUE_COLUMNS:
            values = [str(v) for v in tab[col].to_numpy()]
            rec[col] = [str(tab[col].dtype)] + (values if len(values) <= FULL_VALUES else [len(values), _sha(",".join(values).encode())])
    return rec


def _files_below(folder):
    """Every file of the output folder, those of the per-chain folders of run_chains as chain/name."""
    return sorted(os.path.relpath(os.path.join(d, f), folder).replace(os.sep, "/") for d, _, fs in os.walk(folder) for f in fs)


def run_case(name, tmp, cases=CASES):
    """What one case (of `cases`: CASES or SESSION_DRIVER_CASES) read and wrote: the record the fixture holds."""
    inputs, run = cases[name](tmp)
    before = set(os.listdir(tmp))
    chunks = []
    with _recorded_prints(chunks), contextlib.redirect_stdout(io.StringIO()):
        out = run()
    (folder,) = sorted(set(os.listdir(tmp)) - before)
    folder = os.path.join(str(tmp), folder)
    return {"inputs": inputs_digest(inputs),
            "sha256": {f: _sha(open(os.path.join(folder, f), "rb").read()) for f in _files_below(folder)},
            "tables": {key: _table(tab) for key, tab in out.items() if isinstance(tab, pd.DataFrame)},
            "timing_keys": sorted(out["_timing"]),
            "stdout": "".join(chunks).replace(str(tmp), "<tmp>")}
