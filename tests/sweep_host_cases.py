"""Chains of tests/test_gpu_sweep_host_golden.py and its fixture's maker (tests/golden/make_sweep_host_golden.py).

Every case drives the host side of the sweep (csrc/jwas_hip.hip: sweep_enqueue and f64_sweep, csrc/sweep_plan.hpp) down one of its
paths and records, per sweep, n_events, the schedule word and every returned statistic but the milliseconds, and after the last sweep
a SHA-256 of alpha, beta, delta and the residual of every trait.  The shapes are the schedule worker's (tests/_schedule_worker.py):
n = 2300 individuals (two row groups), three to five blocks with a ragged last one, 4 to 12 sweeps, default switches.
"""
import functools
import hashlib

import numpy as np

import _schedule_worker as W
from conftest import make_dataset

N = W.N
TIMING_FIELDS = ("sweep_ms", "update_kernel_ms", "event_overhead_ms")       # never pinned


def _c(method, bs, t=1, nblocks=3, nsweeps=6, prec=32, prior="mid", **kw):
    return dict(method=method, bs=bs, t=t, p=nblocks * bs + 40 - 23 * (t > 1), nsweeps=nsweeps, prec=prec, prior=prior, **kw)


CASES = {f"worker/{k}": dict(worker=k) for k in W.CASES}
CASES.update({
    "indep/BayesC-256": _c("BayesC", 256, independent=True),
    "indep/BayesR-128": _c("BayesR", 128, independent=True),
    "indep/MTBayesC-128-t2": _c("MTBayesC", 128, t=2, independent=True),
    "indep/MTBayesC_II-t2": _c("MTBayesC_II", 128, t=2, independent=True),
    "indep/MegaBayesC-t2": _c("MegaBayesC", 128, t=2, independent=True),
    "solve/MTBayesC-256-t2": _c("MTBayesC", 256, t=2, section_solve=True, prior="DDDSDD"),
    "solve/MTBayesC-256-t3": _c("MTBayesC", 256, t=3, section_solve=True, prior="DDDSDD"),
    "solve/MTBayesC-256-t4": _c("MTBayesC", 256, t=4, section_solve=True, prior="DDDS", nsweeps=4),
    "cov/MTBayesB-t2": _c("MTBayesB", 128, t=2, resident_cov=True),
    "cov/MTBayesB_II-t2": _c("MTBayesB_II", 128, t=2, resident_cov=True),
    "cov/MegaBayesB-t3": _c("MegaBayesB", 128, t=3, nsweeps=4),
    "prior/BayesB": _c("BayesB", 256),
    "prior/BayesC-pi_vec": _c("BayesC", 256, prior="pi_vec"),
    "prior/BayesR-pi_matrix": _c("BayesR", 256, prior="pi_matrix"),
    "prior/MTBayesC-lpr-t2": _c("MTBayesC", 128, t=2, prior="lpr"),
    "explicit/BayesC": _c("BayesC", 256, starts=[0, 100, 356, 600]),
    "nreps2/BayesC-128": _c("BayesC", 128, nreps=2),
    "timing/lookahead-BayesC-512": dict(worker="lookahead-BayesC-512", timing=2),
    "timing/grouped-BayesC-m2": dict(worker="grouped-BayesC-m2", timing=2),
    "sharded/BayesC-256": _c("BayesC", 256, sharded=True),
    "rows/BayesC-256": _c("BayesC", 256, rows=True),
    "f64/BayesC": _c("BayesC", 256, prec=64),
    "f64/BayesR": _c("BayesR", 256, prec=64),
    "f64/BayesB": _c("BayesB", 256, prec=64),
    "f64/MTBayesC-t2": _c("MTBayesC", 128, t=2, prec=64),
    "f64/MTBayesC_II-t2": _c("MTBayesC_II", 128, t=2, prec=64),
    "f64/MTBayesB-t2": _c("MTBayesB", 128, t=2, prec=64, resident_cov=True),
    "f64/MTBayesC-lpr-t2": _c("MTBayesC", 128, t=2, prec=64, prior="lpr"),
    "f64/indep-BayesC": _c("BayesC", 256, prec=64, independent=True),
    "f64/indep-MTBayesC-t2": _c("MTBayesC", 128, t=2, prec=64, independent=True),
})


@functools.lru_cache(maxsize=4)
def _data(p):
    return make_dataset(n=N, p=p, ncausal=6, seed=1000 + p)


def _mt_prior(t, ch):
    """log pi over the 2^t joint states: D = nearly every marker in the model for every trait, S = sparse, M = in between."""
    ns = 1 << t
    if ch == "D":
        pr = np.full(ns, W.MT_LEAK); pr[-1] = 1.0
    elif ch == "S":
        pr = np.full(ns, (1 - W.MT_SPARSE) / (ns - 1)); pr[0] = W.MT_SPARSE
    else:
        pr = np.full(ns, 0.3 / (ns - 1)); pr[0] = 0.7
    return np.log(pr / pr.sum())


def _own_chain(name, c):
    """Data and per-sweep keyword arguments of a case that is not one of the schedule worker's."""
    d = _data(c["p"])
    p, t, method = c["p"], c["t"], c["method"]
    rng = np.random.default_rng(sum(name.encode()))
    y = (d["y"] - d["y"].mean()).astype(np.float32)
    vare = np.float32(0.5 * y.var())
    varg = np.float32(0.5 * y.var() / (0.05 * float((2 * d["freq"] * (1 - d["freq"])).sum())))
    out = dict(c, name=name, X=d["X"], y=y)
    base = dict(nreps=c.get("nreps", 1), independent_blocks=c.get("independent", False), section_solve=c.get("section_solve", False))
    prior = c["prior"]
    pis = [0.4, 0.4, 0.9, 0.999, 0.999, 0.4, 0.9, 0.9][:c["nsweeps"]]           # (turnover above and below the host's thresholds)
    if t > 1:
        v, g = np.float32(max(float(np.var(y)), 0.1)), np.float32(0.02)
        Rm = (v * (np.eye(t) * (1 + 0.25 * np.arange(t)) + 0.2 * (1 - np.eye(t)))).astype(np.float32)
        Gm = (g * (np.eye(t) + 0.3 * (1 - np.eye(t)))).astype(np.float32)
        if method.startswith("Mega"):
            kws = [dict(base, vare=Rm, var_effect=Gm, pi=np.full(t, pi)) for pi in pis]
            if method == "MegaBayesB":
                vm = np.stack([np.diag(g * rng.uniform(0.5, 2.0, t)) for _ in range(p)]).astype(np.float32)
                kws = [dict(kw, var_effect_matrix=vm) for kw in kws]
        elif prior == "lpr":
            lpm = np.log(rng.dirichlet(np.ones(1 << t) * 2, size=p))
            kws = [dict(base, vare=Rm, var_effect=Gm, log_prior_states=lpm) for _ in pis]
        else:
            pattern = prior if prior != "mid" else "MDMSMD"
            kws = [dict(base, vare=Rm, var_effect=Gm, log_prior_states=_mt_prior(t, ch)) for ch in pattern[:c["nsweeps"]]]
        if c.get("resident_cov"):
            # the first sweep uploads the covariances; before every later one they are drawn on the device and stay resident
            out["vm0"] = np.stack([Gm.astype(np.float64) * rng.uniform(0.5, 2.0) + np.diag(rng.uniform(0, 0.002, t)) for _ in range(p)])
            out["iw"] = (t + 3.0, Gm.astype(np.float64) * 3.0)
    elif method == "BayesR":
        if prior == "pi_matrix":
            pm = rng.dirichlet(np.array([40.0, 3.0, 1.5, 0.5]), size=p)
            kws = [dict(base, vare=vare, var_effect=np.float32(20 * varg), pi_classes=pm) for _ in pis]
        else:
            kws = [dict(base, vare=vare, var_effect=np.float32(20 * varg), pi_classes=W._pi_classes(pi)) for pi in pis]
    else:
        kws = [dict(base, vare=vare, var_effect=varg, pi=pi) for pi in pis]
        if prior == "pi_vec":
            pv = rng.uniform(0.5, 0.999, p)
            kws = [dict(kw, pi=0.0, pi_vec=pv) for kw in kws]
        if method == "BayesB":
            vv = (varg * rng.uniform(0.5, 1.5, p)).astype(np.float64)
            kws = [dict(kw, var_effect_vec=vv) for kw in kws]
    out["kws"] = kws
    out["chain_seed"] = 4321
    return out


def chain(name):
    c = CASES[name]
    if "worker" in c:
        w = W.chain(c["worker"])
        w["kws"] = [dict(kw, group_launch=w["grouped"]) for kw in w["kws"]]
        w.update(prec=32, timing=c.get("timing", 0))
        return w
    return _own_chain(name, c)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _stats(st, flags):
    rec = {"schedule": int(flags)}
    for k, v in st.items():
        if k not in TIMING_FIELDS:
            rec[k] = np.asarray(v, dtype=np.float64).reshape(-1).tolist()
    return rec


def run_case(name):
    """Runs the chain on a fresh engine.  Returns {"sweeps": [per-sweep records], "final": {"alpha0": sha256, ...}}."""
    import jwas_jl_amd as J
    from jwas_jl_amd import streaming as S
    c = chain(name)
    t, prec = c["t"], c["prec"]
    dtype = np.float64 if prec == 64 else np.float32
    hip = J.HipEngine(0, precision=prec)
    try:
        if c.get("kind") == "grouped_packed":
            hip.load_packed2bit(S.pack_2bit(c["codes"]), N, c["means"], centered=True)
        else:
            hip.load_dense(np.asfortranarray(c["X"].astype(dtype)))
        if c.get("sharded"):
            hip.comm_init_loopback(0, 0, 1)
        if c.get("rows"):
            hip.comm_init_loopback(2, 0, 1)
            hip.comm_row_shards(True)
        if c.get("starts"):
            hip.setup_blocks_explicit(np.asarray(c["starts"]), *(() if prec == 64 else ("f64",)))
        else:
            hip.setup_blocks(c["bs"], *(() if prec == 64 else ("f64",)))
        if c.get("grouped"):
            hip.setup_groups(c["m"], "f64")
        hip.init_state(c["method"], t)
        for k in range(t):
            hip.set_residual(((1 + 0.3 * k) * c["y"]).astype(dtype), k)
        if c["method"] == "BayesR":
            hip.set_state(0, delta=np.ones(c["p"], dtype=np.int32))
        elif t > 1:
            for k in range(t):
                hip.set_state(k, delta=np.ones(c["p"], dtype=dtype))
        if c.get("timing"):
            hip.set_kernel_timing(c["timing"])
        sweep = hip.sweep_sharded if c.get("sharded") else hip.sweep
        recs = []
        for it, kw in enumerate(c["kws"], 1):
            if "vm0" in c:
                if it == 1:
                    kw = dict(kw, var_effect_matrix=c["vm0"])
                else:
                    hip.sample_marker_covariances(c["iw"][0], c["iw"][1], seed=c["chain_seed"], iteration=it - 1)
            st = sweep(iteration=it, seed=c["chain_seed"], **kw)
            recs.append(_stats(st, hip.last_sweep_schedule()))
        final = {}
        for k in range(t):
            a, b, d = hip.get_state(k)
            final.update({f"alpha{k}": _sha(a), f"beta{k}": _sha(b), f"delta{k}": _sha(d), f"r{k}": _sha(hip.get_residual(k))})
    finally:
        hip.close()
    return {"sweeps": recs, "final": final}
