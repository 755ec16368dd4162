"""Differential fuzz of the Float64 device context (csrc/f64_path.hpp; f64_sweep / f64_launch_block in csrc/jwas_hip.hip):
ragged shapes down to n = 1, tall shapes whose column groups walk several batches of eight columns, a seeded sample of the
configuration space, and ONE context reused by every case -- its buffers regrow and its partitions and weights are replaced
from case to case, which is part of the test.

References: single-trait BayesA/B/C the C oracle (OracleEngine64), BayesR the block restatement of f64_bayesr_reference.py
(pinned to the C chain by test_f64_bayesr_host.py), the multi-trait kinds the restatement of f64_mt_reference.py.  Bars: those
of test_gpu_f64._compare (indicators / classes identical, effects rtol 1e-9 / atol 1e-12, residual atol 1e-9), event and
class / state counts equal after every sweep, r'R^-1 r within rtol 1e-9.  Both sides compute in double; only the association
of the sums differs (~1e-13), so no case is excused for a near-threshold decision.

Every case prints its largest ratio to each bar and its time ("f64fuzz ..." lines; NOTES.md records a run's summary)."""
import os
import time

import numpy as np
import pytest

from conftest import make_dataset
from oracle_engine import OracleEngine64
from f64_bayesr_reference import BayesROracleEngine64
from f64_mt_reference import RestatementEngine64
from test_gpu_f64 import _compare

pytestmark = pytest.mark.gpu

MT_METHODS = ("MTBayesC", "MTBayesC_II", "MTBayesB", "MTBayesB_II")
SWEEP_SEED = 99


@pytest.fixture(scope="module")
def hip():
    import jwas_jl_amd as J
    e = J.HipEngine(0, precision=64)
    yield e
    e.close()


def reference_for(method):
    if method == "BayesR":
        return BayesROracleEngine64()
    return RestatementEngine64() if method in MT_METHODS else OracleEngine64()


def family(method):
    return "BayesR" if method == "BayesR" else ("multi-trait" if method in MT_METHODS else "BayesABC")


def update_geometry(n, b):
    """(nslices, ncg, cpg) of k64_update_partial for a block of b markers on n records: the rule of f64_launch_block."""
    nslices = (n + 255) // 256
    ncg = max(1, min((b + 7) // 8, (512 + nslices - 1) // nslices))
    cpg = ((b + ncg - 1) // ncg + 7) // 8 * 8
    return nslices, (b + cpg - 1) // cpg, cpg


def _data(n, p, seed):
    d = make_dataset(n=max(n, 2), p=p, ncausal=min(6, p), seed=seed)
    X = np.asfortranarray(d["X"][:n].astype(np.float64))
    y = d["y"][:n].astype(np.float64)
    return X, (y - y.mean() if n > 1 else y)


def _prepare(e, c, X, y):
    """Load case c into engine e: matrix, weights, partition, state, residuals."""
    t, p = c["t"], c["p"]
    e.load_dense(X)
    e.set_weights(c.get("w"))
    if c["part"][0] == "explicit":
        e.setup_blocks_explicit(c["part"][1])
    else:
        e.setup_blocks(c["part"][1])
    e.init_state(c["method"], t)
    for k in range(t):
        e.set_residual((1 + 0.3 * k) * y + c["noise"][k], k)
        if c["method"] == "BayesR":
            e.set_state(0, delta=np.ones(p, dtype=np.int32))
        elif t > 1:
            e.set_state(k, delta=np.ones(p))


def _figures(ref, hip, t, so, sh):
    """The largest ratio of a difference to its bar: (effects, residual, r'R^-1 r)."""
    eff = res = 0.0
    for k in range(t):
        ao, bo, _ = ref.get_state(k)
        ah, bh, _ = hip.get_state(k)
        for got, want in ((ah, ao), (bh, bo)):
            eff = max(eff, float(np.max(np.abs(got - want) / (1e-12 + 1e-9 * np.abs(want)))))
        res = max(res, float(np.max(np.abs(hip.get_residual(k) - ref.get_residual(k))) / 1e-9))
    rss = float(np.max(np.abs(sh["resid_ss"] - so["resid_ss"]) / (1e-9 * np.abs(so["resid_ss"]))))
    return eff, res, rss


def _run_pair(hip, c, X, y, sweeps, tag):
    t0 = time.perf_counter()
    ref = reference_for(c["method"])
    for e in (ref, hip):
        _prepare(e, c, X, y)
    t = c["t"]
    so = sh = None
    for it in range(1, sweeps + 1):
        so = ref.sweep(iteration=it, seed=SWEEP_SEED, **c["kw"])
        sh = hip.sweep(iteration=it, seed=SWEEP_SEED, **c["kw"])
        assert so["n_events"] == sh["n_events"], f"{tag} iteration {it}: events {so['n_events']} vs {sh['n_events']}"
        key = "class_counts" if c["method"] == "BayesR" else "state_counts"
        assert np.array_equal(so[key], sh[key]), f"{tag} iteration {it}: {key} {so[key]} vs {sh[key]}"
    eff, res, rss = _figures(ref, hip, t, so, sh)
    print(f"f64fuzz {tag} family={family(c['method'])} method={c['method']} t={t} n={c['n']} p={c['p']} effects={eff:.3e} "
          f"residual={res:.3e} resid_ss={rss:.3e} events={so['n_events']:.0f} seconds={time.perf_counter() - t0:.2f}")
    _compare(ref, hip, t)
    np.testing.assert_allclose(sh["resid_ss"], so["resid_ss"], rtol=1e-9, atol=0)


def _device_result(e, c, X, y, sweeps):
    _prepare(e, c, X, y)
    for it in range(1, sweeps + 1):
        e.sweep(iteration=it, seed=SWEEP_SEED, **c["kw"])
    return [e.get_state(k) for k in range(c["t"])], [e.get_residual(k) for k in range(c["t"])]


def _sweep_kw(rng, method, t, p, y, sparsity, marker_prior=False):
    v = max(float(np.var(y)), 0.1)
    g = 0.02
    sp = sparsity
    A = rng.standard_normal((t, t)); Rm = (A @ A.T / t + np.eye(t)) * v
    Bm = rng.standard_normal((t, t)); Gm = (Bm @ Bm.T / t + np.eye(t)) * g
    if method in ("BayesC", "BayesB"):
        kw = dict(vare=v, var_effect=g, pi=sp)
        if method == "BayesB":
            kw["var_effect_vec"] = rng.uniform(0.005, 0.04, p)
        if marker_prior:
            kw["pi_vec"] = np.clip(sp + rng.uniform(-0.2, 0.2, p), 0.0, 0.999)
    elif method == "BayesR":
        kw = dict(vare=v, var_effect=0.1, pi_classes=np.concatenate([[sp], np.array([0.5, 0.3, 0.2]) * (1 - sp)]))
        if marker_prior:
            pm = rng.dirichlet(np.ones(4), size=p) * 0.5 + 0.5 * kw["pi_classes"]
            kw["pi_matrix"] = pm / pm.sum(axis=1, keepdims=True)
    else:
        prior = np.full(1 << t, (1 - sp) / ((1 << t) - 1)); prior[0] = sp
        if sp == 0.0:
            prior = np.full(1 << t, 1e-3); prior[-1] = 1.0
        prior /= prior.sum()
        kw = dict(vare=Rm, var_effect=Gm, log_prior_states=np.log(prior))
        if marker_prior:                                                 # marker-specific joint priors (t = 2)
            pm = rng.dirichlet(np.ones(1 << t), size=p) * 0.5 + 0.5 * prior
            kw["log_prior_states"] = np.log(pm / pm.sum(axis=1, keepdims=True))
        if method in ("MTBayesB", "MTBayesB_II"):
            Wm = rng.standard_normal((p, t, t))
            kw["var_effect_matrix"] = (Wm @ Wm.transpose(0, 2, 1) / t + np.eye(t)) * (g * np.exp(rng.uniform(-1, 1, p)))[:, None, None]
    return kw


# ---- ragged and tall shapes ------------------------------------------------------------------------------------------------
# Tall cases, from the rule of f64_launch_block (ncg = min(ceil(b/8), ceil(512/nslices)), cpg = round_up(ceil(b/ncg), 8)):
#   n = 10 240 (40 slices), b = 512: ncg = 13, cpg = 40 -- five full batches of 8 columns per group, the last group 32 columns
#   n = 10 240 (40 slices), b = 500: ncg = 13, cpg = 40 -- the last group holds 20 columns: batches of 8, 8 and a ragged 4
#   n =  5 200 (21 slices), b = 256: ncg = 16, cpg = 16 -- two batches per group, three traits
RAGGED = [
    # (n, p, block, method, t, cpg of the first block or None where the shape is not about the batches)
    (1, 70, 64, "BayesC", 1, None), (3, 5, 64, "BayesC", 1, None), (255, 65, 64, "BayesR", 1, None),
    (256, 9, 8, "BayesC", 1, None),                     # ncg == 1
    (257, 129, 128, "BayesB", 1, None),
    (300, 23, 7, "BayesR", 1, None),                    # block not a multiple of 8 (bstride 8); the last block has 2 markers
    (1023, 300, 223, "MTBayesC", 2, None), (77, 200, 128, "MTBayesC_II", 2, None),
    (10_240, 600, 512, "BayesC", 1, 40), (10_240, 600, 500, "BayesR", 1, 40), (5_200, 300, 256, "MTBayesC", 3, 16),
]


@pytest.mark.parametrize("n,p,bs,method,t,cpg", RAGGED)
def test_f64_ragged_and_tall_shapes(hip, n, p, bs, method, t, cpg):
    if cpg is not None:
        nslices, ncg, got = update_geometry(n, min(bs, p))
        assert got == cpg and got > 8 and ncg > 1, f"the case no longer walks several batches per column group: ncg {ncg}, cpg {got}"
    if (n, p, bs) == (256, 9, 8):
        assert update_geometry(n, 8)[1] == 1 and update_geometry(n, 1)[1] == 1
    rng = np.random.default_rng(n * 1000 + p)
    X, y = _data(n, p, n + p)
    c = dict(method=method, t=t, n=n, p=p, part=("uniform", bs), noise=[0.3 * rng.standard_normal(n) * (k > 0) for k in range(t)],
             kw=_sweep_kw(rng, method, t, p, y, 0.8))
    _run_pair(hip, c, X, y, 6, f"ragged n={n} p={p} block={bs}")


# ---- random configurations ---------------------------------------------------------------------------------------------------
# Estimated microseconds of the Python references per marker update; a case whose repetitions would take the reference past
# BUDGET_US per sweep gets fewer markers (the partition is cut at the new p), never fewer cases.
def _reference_cost_us(method, t):
    if method == "BayesR":
        return 12.0
    if method in ("MTBayesC", "MTBayesB"):
        return 10.0 + 6.0 * t * t
    if method in ("MTBayesC_II", "MTBayesB_II"):
        return (1 << t) * (12.0 + 5.0 * t * t)
    return 0.0                                                          # (the C oracle)


BUDGET_US = 0.4e6


def _split(starts, p, limit):
    while np.diff(np.append(starts, p)).max() > limit:
        sizes = np.diff(np.append(starts, p))
        big = int(np.argmax(sizes))
        starts = np.sort(np.append(starts, starts[big] + sizes[big] // 2))
    return starts.astype(np.int64)


def _random_case(seed):
    """One random configuration: sampler, traits, shape, partition (uniform of any size 1..512, or explicit ragged starts),
    repetitions (1, a few, 0 = the block's size), prior sparsity, Float64 weights, independent blocks, per-marker priors."""
    rng = np.random.default_rng(seed)
    method = str(rng.choice(["BayesC", "BayesB", "BayesR", "MTBayesC", "MTBayesC_II", "MTBayesB", "MTBayesB_II"]))
    t = int(rng.integers(2, 5)) if method in MT_METHODS else 1
    tall = int(seed) % 7 == 3
    n = int(rng.integers(4000, 11001)) if tall else int(rng.integers(40, 701))
    p = int(rng.integers(30, 401)) if tall else int(rng.integers(30, 901))
    nreps = int(rng.choice([1, 1, 1, 2, 5, 0]))
    cost = _reference_cost_us(method, t)
    limit = 128 if nreps == 0 else 300
    if cost and nreps == 0:                                             # (a block repeated its own size must fit the budget alone)
        limit = max(4, min(limit, int(np.sqrt(BUDGET_US / cost))))
    explicit = rng.random() < 0.4
    if explicit:
        cuts = np.unique(rng.integers(1, p, size=int(rng.integers(1, 12))))
        starts = _split(np.concatenate([[0], cuts]), p, limit)
    else:
        bs = int(rng.integers(1, 513)) if rng.random() < 0.5 else int(round(2.0 ** rng.uniform(0, 9)))
        if nreps == 0:
            bs = min(bs, limit)
        starts = np.arange(0, p, bs, dtype=np.int64)
    # the Python references' patience: cut the markers (and with them the partition) when the repetitions ask for too much
    sizes = np.diff(np.append(starts, p))
    updates = np.cumsum(sizes * (sizes if nreps == 0 else nreps))
    if cost and updates[-1] * cost > BUDGET_US:
        if nreps == 0:                                                  # whole blocks (a block's size is its repetition count)
            keep = max(1, int(np.searchsorted(updates * cost, BUDGET_US, side="right")))
            p_new = int(starts[keep]) if keep < len(starts) else p
        else:
            p_new = int(BUDGET_US / (cost * nreps))
        p = min(p, max(p_new, 30))
        starts = starts[starts < p]
    part = ("explicit", starts) if explicit else ("uniform", bs)
    sparsity = float(rng.choice([0.0, 0.3, 0.9, 0.99]))
    weights = rng.random() < 0.25
    pervar = method in ("MTBayesB", "MTBayesB_II")
    indep = (not pervar) and rng.random() < 0.2
    marker_prior = rng.random() < 0.25 and (t == 1 or (t == 2 and not pervar))
    return dict(method=method, t=t, n=n, p=p, part=part, nreps=nreps, sparsity=sparsity, seed=int(seed), weights=weights,
                indep=indep, marker_prior=marker_prior, nblocks=len(starts))


def _materialise(c):
    """The arrays of a random case (data, weights, sweep arguments), all from the case's seed."""
    rng = np.random.default_rng(c["seed"] + 10_000)
    X, y = _data(c["n"], c["p"], c["seed"] % 1000)
    c = dict(c)
    c["noise"] = [0.3 * rng.standard_normal(c["n"]) * (k > 0) for k in range(c["t"])]
    c["w"] = None
    if c["weights"]:
        c["w"] = rng.uniform(0.3, 3.0, c["n"])                          # Float64 weights that no Float32 holds
        assert (c["w"] != c["w"].astype(np.float32)).any()
    c["kw"] = _sweep_kw(rng, c["method"], c["t"], c["p"], y, c["sparsity"], c["marker_prior"])
    c["kw"]["nreps"] = c["nreps"]
    if c["indep"]:
        c["kw"]["independent_blocks"] = True
    return c, X, y


N_CASES = int(os.environ.get("JWAS_F64_FUZZ_CASES", "120"))             # JWAS_F64_FUZZ_CASES=2000 for a long run
FUZZ_BASE = 5000
SHARED_RESULTS = {}                                                     # seed -> what the shared context produced


@pytest.mark.parametrize("seed", list(range(N_CASES)))
def test_f64_random_configurations_against_the_references(hip, seed):
    c, X, y = _materialise(_random_case(FUZZ_BASE + seed))
    assert c["part"][0] == "explicit" or 1 <= c["part"][1] <= 512
    _run_pair(hip, c, X, y, 4, f"seed={seed}")
    SHARED_RESULTS[seed] = ([hip.get_state(k) for k in range(c["t"])], [hip.get_residual(k) for k in range(c["t"])])


# ---- one context, many problems -----------------------------------------------------------------------------------------------
def _reuse_seeds():
    """(sequential case, (sequential case with more blocks, the independent case after it), (weighted case, the unweighted
    case after it)) among the default 120 seeds, in their order."""
    cases = [_random_case(FUZZ_BASE + s) for s in range(120)]
    seq = next(s for s in range(120) if not cases[s]["indep"] and cases[s]["nblocks"] > 1)
    ind = next(s for s in range(1, 120) if cases[s]["indep"] and not cases[s - 1]["indep"] and cases[s - 1]["nblocks"] > cases[s]["nblocks"] > 1)
    unw = next(s for s in range(1, 120) if cases[s - 1]["weights"] and not cases[s]["weights"])
    return seq, ind, unw


def test_f64_shared_context_equals_a_fresh_one_bit_for_bit(hip):
    """Three fuzz cases on a fresh context each, against the shared context that ran other problems first: a sequential
    sweep; an independent sweep right after a sequential one with MORE blocks (the partial-sum and change-list buffers regrow
    with the independent sweep, sized by the new partition); an unweighted case right after a weighted one.  State and
    residual must be equal bit for bit (and equal to what the fuzz above recorded, when it ran in this session)."""
    import jwas_jl_amd as J
    seq, ind, unw = _reuse_seeds()
    shared = {}
    for s in (seq, ind - 1, ind, unw - 1, unw):                         # the shared context, in the fuzz's order
        c, X, y = _materialise(_random_case(FUZZ_BASE + s))
        shared[s] = _device_result(hip, c, X, y, 4)
    for s in (seq, ind, unw):
        c, X, y = _materialise(_random_case(FUZZ_BASE + s))
        fresh = J.HipEngine(0, precision=64)
        try:
            got = _device_result(fresh, c, X, y, 4)
        finally:
            fresh.close()
        for want in [shared[s]] + ([SHARED_RESULTS[s]] if s in SHARED_RESULTS else []):
            for k in range(c["t"]):
                for a, b in zip(got[0][k], want[0][k]):
                    assert np.array_equal(a, b), f"seed {s} trait {k}: the shared context's state differs from a fresh context's"
                assert np.array_equal(got[1][k], want[1][k]), f"seed {s} trait {k}: residual differs"


@pytest.mark.parametrize("method,t", [("BayesC", 1), ("BayesR", 1), ("MTBayesC", 2)])
def test_f64_per_marker_priors_after_a_matrix_with_fewer_markers(method, t):
    """Pins what the fuzz found: a Float64 context kept its per-marker prior tables (pi_vec, pi_matrix, the p x 2^t joint
    priors) across jwas_hip_load_dense_f64, sized by the OLD number of markers, so a sweep with per-marker priors on a later
    matrix with more markers failed its upload ("invalid argument").  One context: 60 markers, then 200, each against its
    reference."""
    import jwas_jl_amd as J
    own = J.HipEngine(0, precision=64)
    try:
        for p in (60, 200):
            rng = np.random.default_rng(p)
            X, y = _data(150, p, 300 + p)
            c = dict(method=method, t=t, n=150, p=p, part=("uniform", 64), noise=[0.3 * rng.standard_normal(150) * (k > 0) for k in range(t)],
                     kw=_sweep_kw(rng, method, t, p, y, 0.8, marker_prior=True))
            _run_pair(own, c, X, y, 3, f"priors after a smaller matrix: {method} p={p}")
    finally:
        own.close()


def test_f64_one_matrix_reconfigured(hip):
    """One loaded matrix, reconfigured in place: weights + an explicit partition (sequential), then set_weights(None) +
    setup_blocks (uniform, more and smaller blocks) with independent blocks, then weights again on the uniform partition --
    each stage against the C oracle given the same calls."""
    n, p = 700, 420
    X, y = _data(n, p, 77)
    rng = np.random.default_rng(8)
    w = rng.uniform(0.3, 3.0, n)
    ref = OracleEngine64()
    for e in (ref, hip):
        e.load_dense(X)
    kw = dict(vare=max(float(np.var(y)), 0.1), var_effect=0.02, pi=0.8)
    stages = [(w, ("explicit", np.array([0, 3, 150, 151, 300])), dict(nreps=2)),
              (None, ("uniform", 24), dict(nreps=1, independent_blocks=True)),
              (w * 0.5, ("uniform", 24), dict(nreps=3, independent_blocks=True)),
              (None, ("explicit", np.array([0, 200])), dict(nreps=1))]
    for stage, (wt, part, extra) in enumerate(stages):
        for e in (ref, hip):
            e.set_weights(wt)
            if part[0] == "explicit":
                e.setup_blocks_explicit(part[1])
            else:
                e.setup_blocks(part[1])
            e.init_state("BayesC", 1)
            e.set_residual(y)
        ww = np.ones(n) if wt is None else wt
        np.testing.assert_allclose(hip.xpx(), (X * X * ww[:, None]).sum(axis=0), rtol=1e-13)
        for it in range(1, 4):
            so = ref.sweep(iteration=it, seed=5 + stage, **kw, **extra)
            sh = hip.sweep(iteration=it, seed=5 + stage, **kw, **extra)
            assert so["n_events"] == sh["n_events"] and np.array_equal(so["state_counts"], sh["state_counts"]), f"stage {stage} iteration {it}"
        _compare(ref, hip, 1)
        np.testing.assert_allclose(sh["resid_ss"], so["resid_ss"], rtol=1e-9, atol=0)
