"""Every schedule variant sweep_enqueue (csrc/jwas_hip.hip) can pick, pinned against the oracle -- and PROVEN to have run.

A sweep does not run one schedule: from the block size, the previous sweep's number of effect changes and JWAS_HIP_* switches the
host picks among kernel instantiations and placements (k_group_step<.., true | false>: ping-pong samplers and cooperative apply of
the merged list, or the steady state bench.py times; the quiet-XCD work-item mapping or all eight XCDs; the cooperative apply of
k_block_step; the dense-walk-only multi-trait sampler; the helper workgroup of the dense single-trait sweeps; the compact candidate
chain).  "The same chain, the same bits", say the comments.  HipEngine.last_sweep_schedule() reports the decisions a sweep took, so:

  1. variants chosen NATURALLY: chains whose prior changes between sweeps so that the turnover crosses every threshold in both
     directions (tests/_schedule_worker.py); the flags must show at least three sweeps on either side and a transition each way,
     and the chain is held to the project's bars against the oracle:
       one block per launch   the oracle's inner products on the device, its sums in the device's order: BIT FOR BIT
                              (test_random_configurations_against_the_oracle);
       grouped, dense         equal delta, equal n_events in every sweep, alpha within 2e-6, r within 2e-5 (test_gpu_groups._same_state);
       grouped, packed        5e-6 and 3e-5 (test_packed_grouped_launches_match_the_oracle);
  2. variants FORCED: most switches are read once per process, so one fresh child process per environment runs the same chains
     (plus a sparse one for the compact candidate chain); the flags must show that the forced variant ran, and the state must be
     BIT FOR BIT the default child's, which itself is compared with the oracle at the bars above.

The prior schedules were chosen on the CPU with the oracle alone; its n_events per sweep, as % of p, against the thresholds
(n_events is asserted identical on the device, so the flags below follow from these numbers):

  grouped BayesC m=2 (p 5144)   8.26 8.32 0.23 0.23 0.25 0.19 5.73 10.81 6.12 0.27 0.17 0.17     threshold 1.25 %
  grouped BayesC m=4 (p 9240)   8.63 8.71 0.32 0.24 0.21 0.18 6.56 12.65 7.15 0.22 0.21 0.19     (low < 0.4, high > 5.7:
  grouped BayesR m=2            8.13 8.15 0.25 0.39 0.31 0.21 7.15 13.22 6.98 0.23 0.25 0.25      under a third of / over four
  grouped BayesR m=4            8.50 8.58 0.21 0.21 0.24 0.23 7.87 14.27 7.39 0.19 0.22 0.18      times the threshold)
  packed  BayesC m=2            as grouped BayesC m=2 (the same trajectory)
     -> sweeps 1-3 and 8-10 run k_group_step<.., true>, sweeps 4-7 and 11-12 k_group_step<.., false> on all eight XCDs
  lookahead BayesC 512 (p 2600) 52.1 73.9 54.2 16.2 8.27 0.50 0.42 0.42 0.42 46.9 71.1 72.8      thresholds 25 % and 1.25 %
     -> cooperative apply in sweeps 2-4 and 11-12 (the first sweep of a chain has no count: off), quiet XCD off in sweeps 7-10
  MTBayesC 128 (p 401)          100 100 100 100 25.9 4.49 2.74 2.00 44.6 65.8 77.6 86.3          threshold 60 %
  MTBayesC 256 (p 785)          100 100 100 100 28.0 3.69 1.53 1.02 44.7 68.2 80.4 87.8          threshold 10 %
     -> dense walk in sweeps 2-5 and 11-12 (128) / 2-6 and 10-12 (256)
  dense BayesC (pi = 0)         100 in every sweep: dense_big and the helper workgroup in every sweep
  (the high phase of the cooperative apply cannot be "twice the threshold" with a prior near 0.5 -- 47 % is the lowest high sweep --
  and a dense multi-trait sweep cannot exceed 100 %; 65.8 % against 60 % is the thinnest margin.  The counts are exact, not noisy.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _schedule_worker as W
from jwas_jl_amd._lib import SCHEDULE_COMPACT_OFF_MASK, SCHEDULE_COMPACT_OFF_SHIFT, SCHEDULE_FLAGS as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import jwas_jl_amd as J
    e = J.HipEngine(0)
    yield e
    e.close()


_REF = {}


def _setup(name):
    """(chain, oracle engine ready to sweep, the inner products the device takes from the oracle): once per chain."""
    if name not in _REF:
        c = W.chain(name)
        orc, pre = W.oracle_for(c)
        _REF[name] = [c, orc, pre]
    return _REF[name]


def _reference(name):
    """(chain, the oracle's run of it, the inner products): the oracle runs a chain once, whoever asks first."""
    ref = _setup(name)
    if not isinstance(ref[1], dict):
        ref[1] = W.run_oracle(ref[1], ref[0])
    return tuple(ref)


def _names(mask):
    s = "+".join(k for k, bit in F.items() if mask & bit)
    co = (mask & SCHEDULE_COMPACT_OFF_MASK) >> SCHEDULE_COMPACT_OFF_SHIFT
    return (s or "-") + (f"+COMPACT_OFF={co}" if co else "")


def _report(tag, name, flags):
    pat = {}
    for f in flags:
        pat[_names(int(f))] = pat.get(_names(int(f)), 0) + 1
    print(f"[schedule] {tag} {name}: " + ", ".join(f"{n} x {k}" for k, n in pat.items()))


def _set_and_clear(name, flags, flag):
    """At least three sweeps with the flag set, three with it clear, and a transition in each direction."""
    on = [bool(int(f) & F[flag]) for f in flags]
    up = sum(1 for a, b in zip(on, on[1:]) if not a and b)
    down = sum(1 for a, b in zip(on, on[1:]) if a and not b)
    assert sum(on) >= 3 and len(on) - sum(on) >= 3 and up >= 1 and down >= 1, f"{name}: {flag} per sweep {on}"


def _every(name, flags, flag, want=True):
    on = [bool(int(f) & F[flag]) for f in flags]
    assert all(v == want for v in on), f"{name}: {flag} per sweep {on}, expected {want} in every sweep"


def _natural_flags(c, flags, geom):
    """What the device's flags must show for chain c under the default switches."""
    name, kind = c["name"], c["kind"]
    if kind in ("grouped", "grouped_packed"):
        _every(name, flags, "GROUPED")
        _set_and_clear(name, flags, "GROUP_PP_KERNEL")            # clear: k_group_step<.., false>, the instantiation bench.py times
        _set_and_clear(name, flags, "GROUP_PINGPONG")
        _set_and_clear(name, flags, "QUIET_XCD")                  # clear: grid 1 + nwork, every XCD streams
        if kind == "grouped":
            _set_and_clear(name, flags, "GROUP_COOP")
        else:
            _every(name, flags, "GROUP_COOP", False)              # (the wide update role of packed storage has no cooperative apply)
    elif kind == "lookahead":
        _set_and_clear(name, flags, "COOP_APPLY")
        _set_and_clear(name, flags, "QUIET_XCD")
    elif kind == "dense":
        _every(name, flags, "DENSE_BIG")
        _every(name, flags, "CORR_HELPER")
        _every(name, flags, "COOP_APPLY")
    elif kind == "mt":
        _set_and_clear(name, flags, "DENSE_MT")
    if kind != "grouped_packed":
        # dense storage: 9 slices of 256 rows in 2 row groups (the second one ragged) x 32 column groups
        assert geom[0] == W.SPG and geom[1] >= 2 and geom[2] >= 2, geom
    else:
        # packed storage streams 1024-row slices: 2300 rows are three of them, the last ragged.  A row group holds 4..8 slices
        # (alloc_storage), so they form ONE row group -- two or more do not exist at n = 2300
        assert geom[1] >= 1 and geom[2] >= 2, geom


def _against_oracle(c, dev, ref):
    name = c["name"]
    assert list(dev["n_events"]) == list(ref["n_events"]), f"{name}: n_events per sweep {list(dev['n_events'])} vs oracle {list(ref['n_events'])}"
    assert not np.any(dev["timeouts"]), f"{name}: hand-over timeouts per sweep {list(dev['timeouts'])}"
    for k in range(c["t"]):
        do, dh = ref[f"delta{k}"], dev[f"delta{k}"]
        assert np.array_equal(do, dh), f"{name}: trajectories diverged at {np.flatnonzero(do != dh)[:5]}"
        if not c["grouped"]:
            for v in ("alpha", "beta", "r"):
                assert np.array_equal(dev[f"{v}{k}"], ref[f"{v}{k}"]), f"{name}: {v} differs by {np.abs(dev[f'{v}{k}'] - ref[f'{v}{k}']).max()}"
        else:
            atol_a, atol_r = (5e-6, 3e-5) if c["kind"] == "grouped_packed" else (2e-6, 2e-5)
            np.testing.assert_allclose(dev[f"alpha{k}"], ref[f"alpha{k}"], rtol=0, atol=atol_a, err_msg=name)
            np.testing.assert_allclose(dev[f"r{k}"], ref[f"r{k}"], rtol=0, atol=atol_r, err_msg=name)


# ---- 1. variants chosen naturally ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.NATURAL)
def test_naturally_chosen_variants_against_the_oracle(hip, name):
    """One chain whose turnover crosses the host's thresholds in both directions: the flags prove which instantiations ran (at least
    three sweeps each, a transition each way), no hand-over timed out, and the chain is the oracle's at the project's bar."""
    c, ref, pre = _reference(name)
    geom = W.setup_device(hip, c, pre)
    dev = W.run_device(hip, c)
    _report("in-process", name, dev["flags"])
    _natural_flags(c, dev["flags"], geom)
    _against_oracle(c, dev, ref)


def test_init_state_starts_a_chain_with_no_previous_sweep(hip):
    """jwas_hip_init_state forgets the previous chain's change count: after a low-turnover chain (whose next sweep would stream on
    all eight XCDs) the first sweep of a new chain runs what a first sweep runs -- the quiet XCD, like a fresh context."""
    c, _, pre = _setup("lookahead-BayesC-512")
    W.setup_device(hip, c, pre)
    low = dict(c["kws"][0], pi=0.999)
    for it in range(1, 5):
        ev = hip.sweep(iteration=it, seed=3, **low)["n_events"]
    assert ev < 0.0125 * c["p"]
    assert not hip.last_sweep_schedule() & F["QUIET_XCD"]             # (the chain did reach the steady-state placement)
    assert hip.last_sweep_schedule(names=True)["QUIET_XCD"] is False
    hip.init_state("BayesC")
    assert hip.last_sweep_schedule() == 0
    hip.set_residual(c["y"])
    hip.sweep(iteration=1, seed=3, **low)
    assert hip.last_sweep_schedule() & F["QUIET_XCD"]


# ---- 2. variants forced: one fresh child process per environment --------------------------------------------------------------------

_SWITCHES = ("JWAS_HIP_PINGPONG", "JWAS_HIP_GROUP_COOP", "JWAS_HIP_QUIET_XCD", "JWAS_HIP_CORR_HELPER", "JWAS_HIP_GROUPS",
             "JWAS_HIP_DENSE_MT_FRACTION", "JWAS_HIP_COMPACT_OFF", "JWAS_HIP_MAX_NCG", "JWAS_HIP_DENSE_MT", "JWAS_HIP_DENSE_BIG_OFF",
             "JWAS_HIP_COOP_APPLY", "JWAS_HIP_SPG", "JWAS_HIP_WG_BUDGET")
ENVS = [("default", {})]
ENVS += [(f"pp{a}-coop{b}-quiet{q}", {"JWAS_HIP_PINGPONG": str(a), "JWAS_HIP_GROUP_COOP": str(b), "JWAS_HIP_QUIET_XCD": str(q)})
         for a in (0, 1) for b in (0, 1) for q in (0, 1)]
ENVS += [("corr-helper0", {"JWAS_HIP_CORR_HELPER": "0"}), ("groups0", {"JWAS_HIP_GROUPS": "0"}),
         ("compact-off1", {"JWAS_HIP_COMPACT_OFF": "1"}), ("compact-off2", {"JWAS_HIP_COMPACT_OFF": "2"}),
         ("max-ncg1", {"JWAS_HIP_MAX_NCG": "1"}), ("max-ncg3", {"JWAS_HIP_MAX_NCG": "3"})]

# One child runs all 14 chains (import, context, uploads, 160 sweeps): 2.0 - 2.7 s measured on an MI355X, the slowest of the 15
# environments; the limit is four times that.
CHILD_SECONDS_MEASURED = 2.7
CHILD_TIMEOUT = 4 * CHILD_SECONDS_MEASURED           # 10.8 s
_CHILD = {}
_FAILED = {}
_STOP = []          # set once a child ends abnormally: nothing more is started on the GPU by this module


def _child(env_id, tmp_path_factory):
    """The result of the worker under environment env_id (run once; children never overlap: pytest runs these tests in turn)."""
    if env_id in _CHILD:
        return _CHILD[env_id]
    if env_id in _FAILED:                                             # (no second attempt)
        pytest.fail(_FAILED[env_id])
    if _STOP:
        pytest.skip(f"no further child processes on the GPU: {_STOP[0]}")
    names = list(W.CASES)
    if "pre" not in _CHILD:
        path = str(tmp_path_factory.mktemp("schedule") / "pre.npz")
        np.savez(path, **{f"{n}/{k}": v for n in names for k, v in (_setup(n)[2] or {}).items()})
        _CHILD["pre"] = path
    out = str(tmp_path_factory.mktemp("schedule") / f"{env_id}.npz")
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(dict(ENVS)[env_id])
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(W.__file__)), "_schedule_worker.py"), out, _CHILD["pre"]] + names
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"the child under {env_id} did not finish within {CHILD_TIMEOUT:.1f} s")
        _FAILED[env_id] = _STOP[0]
        pytest.fail(_STOP[0])
    text = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in text:
        _STOP.append(f"the child under {env_id} ended abnormally (exit status {r.returncode})")
        _FAILED[env_id] = _STOP[0] + "\n" + text[-3000:]
        pytest.fail(_FAILED[env_id])
    if r.returncode != 0 or "SCHEDULE_WORKER_OK" not in r.stdout:
        _FAILED[env_id] = f"child under {env_id}: exit status {r.returncode}\n{text[-3000:]}"
        pytest.fail(_FAILED[env_id])
    z = np.load(out)
    res = {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in names}
    _CHILD[env_id] = res
    return res


def _forced_flags(env, name, c, flags, default_flags):
    """The flags must show that the switch took effect in every sweep it governs."""
    grouped, packed = c["grouped"], c["kind"] == "grouped_packed"
    if "JWAS_HIP_GROUPS" in env:
        _every(name, flags, "GROUPED", False)
        return
    if grouped and "JWAS_HIP_PINGPONG" in env:
        pp, co, qx = (env[k] == "1" for k in ("JWAS_HIP_PINGPONG", "JWAS_HIP_GROUP_COOP", "JWAS_HIP_QUIET_XCD"))
        _every(name, flags, "GROUPED")
        _every(name, flags, "GROUP_PINGPONG", pp)
        _every(name, flags, "GROUP_COOP", co and not packed)
        _every(name, flags, "GROUP_PP_KERNEL", pp or (co and not packed))          # pp0-coop0: the steady-state instantiation in EVERY sweep
        _every(name, flags, "QUIET_XCD", qx or pp)                                 # (ping-pong launches carry the quiet XCD)
    if c["kind"] in ("lookahead", "sparse", "mt") and "JWAS_HIP_QUIET_XCD" in env:
        _every(name, flags, "QUIET_XCD", env["JWAS_HIP_QUIET_XCD"] == "1")
    if "JWAS_HIP_CORR_HELPER" in env:
        _every(name, flags, "CORR_HELPER", False)
    co = int(env.get("JWAS_HIP_COMPACT_OFF", "0"))
    assert all(((int(f) & SCHEDULE_COMPACT_OFF_MASK) >> SCHEDULE_COMPACT_OFF_SHIFT) == co for f in flags), name
    if not set(env) & {"JWAS_HIP_PINGPONG", "JWAS_HIP_CORR_HELPER"}:
        assert list(flags & ~SCHEDULE_COMPACT_OFF_MASK) == list(default_flags), f"{name}: the switch changed other decisions"


@pytest.mark.parametrize("env_id", [e for e, _ in ENVS])
def test_forced_variants_are_the_default_chain_bit_for_bit(env_id, tmp_path_factory):
    """A fresh process per environment (the switches are read once per process).  Default: every chain against the oracle at its bar,
    with the flags of the natural selection.  Every other environment: the flags show the forced variant in every sweep, the geometry's
    summation order is unchanged, and final state and n_events of every chain are BIT FOR BIT the default child's."""
    env = dict(ENVS)[env_id]
    base = _child("default", tmp_path_factory)
    res = base if env_id == "default" else _child(env_id, tmp_path_factory)
    for name, dev in res.items():
        c = _setup(name)[0]
        _report(env_id, name, dev["flags"])
        assert not np.any(dev["timeouts"]), f"{name}: hand-over timeouts per sweep {list(dev['timeouts'])}"
        if env_id == "default":
            if name in W.NATURAL:
                _natural_flags(c, dev["flags"], dev["geometry"])
            _against_oracle(c, dev, _reference(name)[1])
            continue
        b = base[name]
        _forced_flags(env, name, c, dev["flags"], b["flags"])
        assert dev["geometry"][0] == b["geometry"][0], f"{name}: slices per row group {dev['geometry']} vs {b['geometry']}"
        if "JWAS_HIP_MAX_NCG" in env:
            assert dev["geometry"][2] <= int(env["JWAS_HIP_MAX_NCG"]) and dev["geometry"][1] == b["geometry"][1], dev["geometry"]
        else:
            assert list(dev["geometry"]) == list(b["geometry"])
        if "JWAS_HIP_GROUPS" in env and c["grouped"]:
            # NOT a bit-identity claim: with the groups off these chains run one block per launch, whose corrections are summed in another
            # order (the grouped schedule adds cG + cP + cW, the plain one a single cross-Gram product).  Held to the oracle's bar instead.
            print(f"[schedule] {env_id} {name}: one block per launch vs grouped default child: max |d alpha| "
                  f"{np.abs(dev['alpha0'] - b['alpha0']).max():.3g}, max |d r| {np.abs(dev['r0'] - b['r0']).max():.3g}")
            _against_oracle(c, dev, _reference(name)[1])
            continue
        assert list(dev["n_events"]) == list(b["n_events"]), f"{name}: n_events {list(dev['n_events'])} vs default {list(b['n_events'])}"
        for k in sorted(dev):
            if k[:-1] in ("alpha", "beta", "delta", "r"):
                assert np.array_equal(dev[k], b[k]), f"{name} under {env_id}: {k} differs from the default child's by {np.abs(dev[k].astype(np.float64) - b[k]).max()}"
