"""Chains of tests/test_gpu_schedule_variants.py, and the worker that runs them in a fresh process.

sweep_enqueue (csrc/jwas_hip.hip) picks a kernel instantiation and a placement per sweep from the block size, the previous sweep's
number of effect changes and JWAS_HIP_* switches, most of which are read ONCE per process.  The chains here are built so that the
thresholds are crossed in both directions along one chain (the prior changes between sweeps); run as a program, this file runs a
list of them under whatever switches its environment carries and writes, per chain, the final state, the per-sweep n_events and
the per-sweep schedule flags (HipEngine.last_sweep_schedule) to an .npz:

    python _schedule_worker.py OUT.npz PRE.npz CASE [CASE ...]      (PRE.npz: the oracle's inner products, see oracle_for)

All chains: n = 2300 individuals (dense storage: 9 slices of 256 rows = 2 row groups; packed: three 1024-row slices, the last ragged).
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import make_dataset  # noqa: E402

N = 2300
H, L = 0.9, 0.999               # grouped chains: pi of the high- / low-turnover sweeps
# Grouped chains, 12 sweeps.  A sweep's schedule follows the PREVIOUS sweep's n_events (threshold 1.25 % of p), and the first low
# sweep after a high one still counts the departures, so: sweeps 1-3 and 8-10 run the ping-pong / cooperative instantiation,
# sweeps 4-7 and 11-12 the steady-state one.
GROUPED_PI = [H, L, L, L, L, L, H, H, L, L, L, L]
# One block per launch, 12 sweeps: cooperative apply from 25 % turnover on, quiet XCD from 1.25 % on.
LOOKAHEAD_PI = [0.4, 0.4, 0.9, 0.9, 0.999, 0.999, 0.999, 0.999, 0.999, 0.4, 0.4, 0.4]
# Multi-trait sampler I, 12 sweeps: D = nearly every marker in the model for both traits, S = sparse.
MT_PRIOR = "DDDSSSSSDDDD"
MT_SPARSE = 0.99
MT_LEAK = 1e-3


def _grouped(method, m, packed=False):
    return dict(kind="grouped_packed" if packed else "grouped", method=method, t=1, bs=1024, m=m, p=1024 * (2 * m + 1) + 24,
                ncausal=5, seed=40 + m, chain_seed=77, nsweeps=12)


def _plain(kind, method, bs, p, nsweeps, t=1, ncausal=6, seed=0, vscale=1.0):
    return dict(vscale=vscale, kind=kind, method=method, t=t, bs=bs, m=0, p=p, ncausal=ncausal, seed=seed or bs + p, chain_seed=1234, nsweeps=nsweeps)


CASES = {
    "grouped-BayesC-m2": _grouped("BayesC", 2), "grouped-BayesC-m4": _grouped("BayesC", 4),
    "grouped-BayesR-m2": _grouped("BayesR", 2), "grouped-BayesR-m4": _grouped("BayesR", 4),
    "packed-BayesC-m2": _grouped("BayesC", 2, packed=True),
    "lookahead-BayesC-512": _plain("lookahead", "BayesC", 512, 5 * 512 + 40, 12, vscale=0.25),
    "dense-BayesC-256": _plain("dense", "BayesC", 256, 3 * 256 + 40, 10), "dense-BayesC-512": _plain("dense", "BayesC", 512, 3 * 512 + 40, 10),
    "dense-control-BayesC-256": _plain("dense", "BayesC", 256, 2 * 256 + 40, 10),
    "dense-control-BayesC-512": _plain("dense", "BayesC", 512, 2 * 512 + 40, 10),
    "mt-MTBayesC-128": _plain("mt", "MTBayesC", 128, 3 * 128 + 17, 12, t=2), "mt-MTBayesC-256": _plain("mt", "MTBayesC", 256, 3 * 256 + 17, 12, t=2),
    # (worker only: the compact candidate chain of sampler_st.hpp under JWAS_HIP_COMPACT_OFF)
    "sparse-BayesC-512": _plain("sparse", "BayesC", 512, 5 * 512 + 40, 10, ncausal=12),
    "sparse-BayesR-512": _plain("sparse", "BayesR", 512, 5 * 512 + 40, 10, ncausal=12),
}
NATURAL = [k for k in CASES if not k.startswith("sparse")]


def _pi_classes(pi):
    return np.array([pi, 0.6 * (1 - pi), 0.3 * (1 - pi), 0.1 * (1 - pi)])


def chain(name):
    """Data and the per-sweep keyword arguments of chain `name` (deterministic)."""
    c = dict(CASES[name])
    c["name"] = name
    packed = c["kind"] == "grouped_packed"
    d = make_dataset(n=N, p=c["p"], ncausal=c["ncausal"], seed=c["seed"], center=not packed)
    y = (d["y"] - d["y"].mean()).astype(np.float32)
    if packed:                                       # missing codes as in test_gpu_packed.py
        raw = d["raw"].astype(np.float64)
        rng = np.random.default_rng(c["seed"])
        raw[rng.integers(0, N, 40), rng.integers(0, c["p"], 40)] = 9
        miss = raw == 9
        c["codes"] = np.where(miss, 3, raw).astype(np.uint8)
        c["means"] = np.array([raw[~miss[:, j], j].mean(dtype=np.float32) for j in range(c["p"])], dtype=np.float32)
        v = np.where(miss, c["means"][None, :], raw.astype(np.float32)).astype(np.float32)
        c["X"] = np.asfortranarray(v - c["means"][None, :])
        freq = c["means"] / 2.0
    else:
        c["X"] = d["X"]
        freq = d["freq"]
    c["y"] = y
    vare = np.float32(0.5 * y.var())
    sum2pq = float((2 * freq * (1 - freq)).sum())
    varg = np.float32(c.get("vscale", 1.0) * 0.5 * y.var() / (0.05 * sum2pq))      # (the effect variance of a chain with pi = 0.95, kept along the chain)
    kind, method = c["kind"], c["method"]
    if kind in ("grouped", "grouped_packed"):
        pis = GROUPED_PI
    elif kind == "lookahead":
        pis = LOOKAHEAD_PI
    elif kind == "dense":
        pis = [0.0] * c["nsweeps"]
    elif kind == "sparse":
        pis = [0.95] * c["nsweeps"]
    if kind == "mt":
        v, g = np.float32(max(float(np.var(y)), 0.1)), np.float32(0.02)
        Rm = np.array([[v, 0.2 * v], [0.2 * v, 1.5 * v]], dtype=np.float32)
        Gm = np.array([[g, 0.3 * g], [0.3 * g, g]], dtype=np.float32)
        dense = np.array([MT_LEAK, MT_LEAK, MT_LEAK, 1.0]); dense /= dense.sum()
        sparse = np.array([MT_SPARSE] + [(1 - MT_SPARSE) / 3] * 3)
        c["kws"] = [dict(vare=Rm, var_effect=Gm, log_prior_states=np.log(dense if ch == "D" else sparse)) for ch in MT_PRIOR]
    elif method == "BayesR":
        c["kws"] = [dict(vare=vare, var_effect=np.float32(20 * varg), pi_classes=_pi_classes(pi)) for pi in pis]
    else:
        c["kws"] = [dict(vare=vare, var_effect=varg, pi=pi) for pi in pis]
    assert len(c["kws"]) == c["nsweeps"]
    c["grouped"] = kind in ("grouped", "grouped_packed")
    return c


SPG = 8      # slices per row group of the update role at n = 2300, dense storage (jwas_hip_update_geometry; the tests assert it)


def _init(e, c):
    e.init_state(c["method"], c["t"])
    for k in range(c["t"]):
        e.set_residual(((1 + 0.3 * k) * c["y"]).astype(np.float32), k)
    if c["method"] == "BayesR":
        e.set_state(0, delta=np.ones(c["p"], dtype=np.int32))
    elif c["t"] > 1:
        for k in range(c["t"]):
            e.set_state(k, delta=np.ones(c["p"], dtype=np.float32))


def oracle_for(c):
    """The OracleEngine of chain c, ready to sweep, and -- for the chains with one block per launch -- the inner products the device
    takes from it (`pre`: x'x, Grams and cross-Grams summed in the device's order; the harness of
    test_random_configurations_against_the_oracle, which makes the comparison bit for bit)."""
    import oracle as O
    from oracle_engine import OracleEngine
    pre = None
    if c["grouped"]:
        orc = OracleEngine("lookahead")
        orc.load_dense(c["X"])
        orc.setup_blocks(c["bs"], "f64")
        orc.setup_groups(c["m"], "f64")
    else:
        O.set_device_order(SPG)
        try:
            orc = OracleEngine("lookahead", acc=O.ACC_DEVICE)
            orc.load_dense(c["X"])
            orc.setup_blocks(c["bs"], "f64")
            st = list(orc._bs) + [c["p"]]
            pre = {"xpx": orc._xpx, "grams": orc._grams}
            for kb in range(1, len(st) - 1):
                pre[f"cross{kb}"] = O.cross_gram(c["X"], st[kb - 1], st[kb] - st[kb - 1], st[kb], st[kb + 1] - st[kb], O.ACC_DEVICE)
        finally:
            O.set_device_order(8)
    _init(orc, c)
    return orc, pre


def setup_device(hip, c, pre):
    """Puts chain c on the engine (pre: see oracle_for).  Returns update_geometry()."""
    from jwas_jl_amd import streaming as S
    if c["kind"] == "grouped_packed":
        hip.load_packed2bit(S.pack_2bit(c["codes"]), N, c["means"], centered=True)
    else:
        hip.load_dense(c["X"])
    hip.set_weights(None)
    geom = hip.update_geometry()
    hip.setup_blocks(c["bs"], "f64")
    if c["grouped"]:
        hip.setup_groups(c["m"], "f64")
    else:
        hip.set_xpx(pre["xpx"]); hip.set_grams_packed(pre["grams"])
        for kb in range(1, hip.nblocks):
            hip.set_cross_gram(kb, pre[f"cross{kb}"])
    _init(hip, c)
    return geom


def run_oracle(orc, c):
    """The chain on the oracle: final state and per-sweep n_events."""
    import oracle as O
    ev = []
    try:
        if c["kind"] == "grouped_packed":
            orc.set_packed_source(c["codes"], c["means"], centered=True)
        if not c["grouped"]:
            O.set_device_order(SPG)
        for it, kw in enumerate(c["kws"], 1):
            ev.append(int(orc.sweep(iteration=it, seed=c["chain_seed"], group_launch=c["grouped"], **kw)["n_events"]))
    finally:
        O.set_device_order(8)
        if c["kind"] == "grouped_packed":
            orc.set_packed_source(None, None)
    return _final(orc, c, ev, None, None)


def run_device(hip, c):
    """The chain on the device: final state, per-sweep n_events, schedule flags and hand-over timeouts (counter 24)."""
    ev, flags, timeouts = [], [], []
    for it, kw in enumerate(c["kws"], 1):
        ev.append(int(hip.sweep(iteration=it, seed=c["chain_seed"], group_launch=c["grouped"], **kw)["n_events"]))
        flags.append(hip.last_sweep_schedule())
        timeouts.append(hip.last_sweep_counters()[24])
    return _final(hip, c, ev, flags, timeouts)


def _final(e, c, ev, flags, timeouts):
    out = {"n_events": np.array(ev, dtype=np.int64)}
    if flags is not None:
        out["flags"] = np.array(flags, dtype=np.int64)
        out["timeouts"] = np.array(timeouts, dtype=np.int64)
    for k in range(c["t"]):
        a, b, d = e.get_state(k)
        out[f"alpha{k}"], out[f"beta{k}"], out[f"delta{k}"], out[f"r{k}"] = a, b, d, e.get_residual(k)
    return out


def main(argv):
    out_path, pre_path, names = argv[1], argv[2], argv[3:]
    import jwas_jl_amd as J
    pre_all = np.load(pre_path)
    hip = J.HipEngine(0)
    res = {}
    for name in names:
        c = chain(name)
        pre = None if c["grouped"] else {k.split("/", 1)[1]: pre_all[k] for k in pre_all.files if k.startswith(name + "/")}
        geom = setup_device(hip, c, pre)
        r = run_device(hip, c)
        r["geometry"] = np.array(geom, dtype=np.int64)
        for k, v in r.items():
            res[f"{name}/{k}"] = v
    hip.close()
    np.savez(out_path, **res)
    print("SCHEDULE_WORKER_OK")


if __name__ == "__main__":
    main(sys.argv)
