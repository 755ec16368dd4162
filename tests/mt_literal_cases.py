"""Multi-trait sweeps against the LITERAL chain: the case table and the builder shared by tests/test_mt_literal_host.py (the
lookahead oracle against the literal one, on the CPU) and tests/test_gpu_mt_literal.py (the device against the literal one).

The literal chain is the non-block form of MTBayesABC.jl:57-127 -- per marker one dot product per trait, the t conditionals
(sampler I) / the joint state (sampler II) / t independent single-trait draws (mega-trait), one axpy per trait -- i.e.
OracleEngine(form="dense") with the per-marker arithmetic in the reference's own order (orc_set_mt_linear_form(0)).  It forms no
Gram, knows no block and no lookahead correction: nothing of the block algebra that sampler_mt.hpp and the oracle's lookahead form
share can hide in it.

Geometry: n = 5 200 (five full 1024-row slices and a ragged one); every p is two full blocks and a ragged tail at the case's block
size (three at 256 / 512 markers).  These are the geometries `bench.py --workload config4` runs through: the 256-marker dense start and
its mixed-state transition, 512- and 1024-marker skip and verify.
"""
import contextlib
from collections import namedtuple

import numpy as np

import oracle as O
from conftest import make_dataset
from oracle_engine import OracleEngine

N = 5200
SWEEP_SEED = 23

# levels: resident block sizes 256 / 512 / 1024, switched between sweeps (mcmc.pick_block_size_mt's three levels)
Case = namedtuple("Case", "id method t bs p prior dup sweeps seed levels sweep_seed", defaults=(SWEEP_SEED,))
CASES = [
    Case("s1-512-dup", "MTBayesC", 3, 512, 3 * 512 + 150, "sparse", True, 12, 1425, False),
    Case("s1-1024-dup", "MTBayesC", 3, 1024, 2 * 1024 + 150, "sparse", True, 12, 1938, False),
    Case("s1-1024-t4", "MTBayesC", 4, 1024, 2 * 1024 + 150, "sparse", False, 10, 1941, False),
    Case("s1-256-mixed-t3", "MTBayesC", 3, 256, 3 * 256 + 77, "mixed", False, 8, 77, False),
    Case("s1-256-mixed-t2", "MTBayesC", 2, 256, 3 * 256 + 77, "mixed", False, 8, 78, False),
    Case("s2-512-dup", "MTBayesC_II", 3, 512, 3 * 512 + 150, "sparse", True, 12, 1425, False),
    Case("s2-256-mixed", "MTBayesC_II", 2, 256, 3 * 256 + 77, "mixed", False, 8, 79, False),
    Case("mega-512-dup", "MegaBayesC", 3, 512, 3 * 512 + 150, "sparse", True, 12, 1425, False),
    Case("mega-256-mixed", "MegaBayesC", 4, 256, 3 * 256 + 77, "mixed", False, 8, 80, False),
    Case("b1-512", "MTBayesB", 3, 512, 3 * 512 + 150, "sparse", False, 12, 1425, False),
    Case("levels", "MTBayesC", 3, 256, 2 * 1024 + 200, "sparse", False, 12, 1937, True),
]
# The same two geometries under four more sweep seeds (other draws at every marker; the table's rows keep sweep seed 23).  The take-over
# condition of the dup rows is asked of the table's rows only: whether a copy enters from a skipped sub-block depends on the draws.
EXTRA_SWEEP_SEEDS = (29, 31, 37, 41)
CASES += [c._replace(id=f"{c.id}-seed{s}", sweep_seed=s) for c in (CASES[0], CASES[3]) for s in EXTRA_SWEEP_SEEDS]
CASE_IDS = [c.id for c in CASES]


def is_table_row(case):
    return case.sweep_seed == SWEEP_SEED


# The bars (the docstring of tests/test_gpu_literal.py: the reference's own stream-against-dense bar).
REL_BAR = 1e-4
ALPHA_FLOOR = 1e-3


def level_of_sweep(it):
    """The `levels` row: the resident block size of sweep `it` (1-based), the switches of test_mt_three_resident_block_sizes_mid_chain."""
    return (256, 512, 1024, 1024, 512, 1024)[(it // 2) % 6]


def build_inputs(case, n=N):
    """X, the t residuals, the sweep's keyword arguments and the starting delta of a case."""
    t = case.t
    data = make_dataset(n=n, p=case.p, ncausal=24, h2=0.7, seed=case.seed)
    X = data["X"]
    if case.dup:
        X = X.copy()
        causal = set(int(j) for j in data["causal"])
        for j in data["causal"]:
            for off in (64, 130, 200):
                k = int(j) + off
                if k // case.bs == int(j) // case.bs and k < X.shape[1] and k not in causal:      # (same block, a later sub-block)
                    X[:, k] = X[:, j]
        X = np.asfortranarray(X)
    rng = np.random.default_rng(17 + t)
    yc = data["y"] - data["y"].mean()
    Y = np.stack([(1 + 0.2 * k) * yc + 0.3 * rng.standard_normal(n).astype(np.float32) for k in range(t)]).astype(np.float32)
    A = rng.standard_normal((t, t)); B = rng.standard_normal((t, t))
    vare = ((A @ A.T / t + np.eye(t)) * 0.5).astype(np.float32)
    varg = ((B @ B.T / t + np.eye(t)) * (0.01 if case.prior == "sparse" else 0.003)).astype(np.float32)
    kw = dict(vare=vare, var_effect=varg)
    if case.method == "MegaBayesC":
        kw = dict(vare=np.diag(np.diag(vare)).astype(np.float32), var_effect=np.diag(np.diag(varg)).astype(np.float32),
                  pi=np.full(t, 0.99 if case.prior == "sparse" else 0.5))
    else:
        if case.prior == "sparse":
            prior = np.full(1 << t, 0.03 / ((1 << t) - 1)); prior[0] = 0.97
        else:
            prior = np.random.default_rng(5).dirichlet(np.ones(1 << t))
        kw["log_prior_states"] = np.log(prior)
        if case.method == "MTBayesB":                        # a covariance per marker (the helper waves use the marker's own constants)
            Bm = rng.standard_normal((case.p, t, t))
            kw["var_effect_matrix"] = ((Bm @ Bm.transpose(0, 2, 1) / t + np.eye(t)) * 0.01).astype(np.float32)
    delta0 = np.full(case.p, 0.0 if case.prior == "sparse" else 1.0, dtype=np.float32)
    return dict(X=X, Y=Y, kw=kw, delta0=delta0, causal=data["causal"])


def literal(X, method, t):
    """The literal non-block oracle on X (no Grams are formed: the dense form only needs x'x)."""
    orc = OracleEngine(form="dense")
    orc.load_dense(X)
    orc._xpx = O.xpx(orc.X, orc.acc)
    orc._groups = {}
    orc.block_size = 0
    orc.init_state(method, t)
    return orc


@contextlib.contextmanager
def literal_order():
    """The oracle's per-marker arithmetic in the reference's conditional-by-conditional order (Rule L's linear form off)."""
    O.lib().orc_set_mt_linear_form(0)
    try:
        yield
    finally:
        O.lib().orc_set_mt_linear_form(1)


def start(engine, inp, t):
    for k in range(t):
        engine.set_residual(inp["Y"][k], k)
        engine.set_state(k, delta=inp["delta0"])


def joint_state(engine, t):
    s = np.zeros(engine.p, dtype=np.int64)
    for k in range(t):
        s |= (engine.get_state(k)[2] != 0).astype(np.int64) << k
    return s


def first_difference(lit, other, t):
    """(trait, markers) of the first trait whose delta arrays differ, or None."""
    for k in range(t):
        dl, do = lit.get_state(k)[2], other.get_state(k)[2]
        if not np.array_equal(dl, do):
            return k, np.flatnonzero(dl != do)[:8]
    return None


def relative_gaps(lit, other, t):
    """Per trait: (max |alpha - alpha_lit| / max(|alpha_lit|.max(), 1e-3), max |r - r_lit| / |r_lit|.max())."""
    out = []
    for k in range(t):
        al, ao = lit.get_state(k)[0], other.get_state(k)[0]
        rl, ro = lit.get_residual(k), other.get_residual(k)
        out.append((float(np.abs(ao - al).max()) / max(float(np.abs(al).max()), ALPHA_FLOOR),
                    float(np.abs(ro - rl).max()) / float(np.abs(rl).max())))
    return out


def literal_probabilities(lit, before, kw, j, t):
    """Sampler I: [(probDelta1, uniform)] for every trait of marker j in the literal chain -- mt1_update of oracle/jwas_oracle.c restated
    operation for operation -- from `before` = dict(alpha, beta, delta, r), the literal engine's arrays before the sweep with keyword
    arguments kw; the markers in front of j are swept by the literal oracle itself on X[:, :j].  For the report that a diverged
    trajectory needs: a rounding tie is a draw whose probability and uniform differ by less than 1e-6."""
    f = np.float32
    X = lit.X
    r = before["r"].copy()
    if j > 0:
        sub = OracleEngine(form="dense")
        sub.load_dense(X[:, :j]); sub._xpx = lit._xpx[:j].copy(); sub._groups = {}; sub.block_size = 0
        sub.init_state(lit.method, t)
        sub.alpha = np.ascontiguousarray(before["alpha"][:, :j]); sub.beta = np.ascontiguousarray(before["beta"][:, :j])
        sub.delta = np.ascontiguousarray(before["delta"][:, :j]); sub.r = r
        kws = {k: v for k, v in kw.items() if k not in ("section_solve", "group_launch", "independent_blocks")}
        with literal_order():
            sub.sweep(**kws)
        r = sub.r
    Rinv = np.linalg.inv(np.asarray(kw["vare"], dtype=np.float32).reshape(t, t).astype(np.float64)).astype(f)
    Ginv = np.linalg.inv(np.asarray(kw["var_effect"], dtype=np.float32).reshape(t, t).astype(np.float64)).astype(f)
    lp = np.asarray(kw["log_prior_states"], dtype=np.float64)
    d = f(lit._xpx[j])
    x = X[:, j].astype(np.float64)
    b = before["beta"][:, j].astype(f).copy(); dl = before["delta"][:, j].astype(f).copy(); al = before["alpha"][:, j].astype(f)
    w = np.array([f(f(x @ r[k].astype(np.float64)) + d * al[k]) for k in range(t)], dtype=f)
    out = []
    L_ = O.lib()
    for k in range(t):
        G11 = Ginv[k, k]; C11 = f(G11 + f(Rinv[k, k] * d))
        rhs0, c12b, wR = f(0), f(0), f(0)
        for m in range(t):
            wR = f(wR + f(w[m] * Rinv[m, k]))
            if m == k:
                continue
            C12m = f(Ginv[k, m] + f(f(d * dl[m]) * Rinv[k, m]))
            rhs0 = f(rhs0 + f(Ginv[k, m] * b[m])); c12b = f(c12b + f(C12m * b[m]))
        rhs0 = f(-rhs0)
        inv0 = f(f(1) / G11); g0 = f(rhs0 * inv0); inv1 = f(f(1) / C11); rhs1 = f(wR - c12b); g1 = f(rhs1 * inv1)
        s0 = sum((1 << m) for m in range(t) if m != k and dl[m] != 0); s1 = s0 | (1 << k)
        in0 = f(f(np.log(np.float64(G11))) - f(f(g0 * g0) * G11)); in1 = f(f(np.log(np.float64(C11))) - f(f(g1 * g1) * C11))
        l0 = -0.5 * float(in0) + lp[s0]; l1 = -0.5 * float(in1) + lp[s1]
        prob = 1.0 / (1.0 + np.exp(l0 - l1))
        u = float(L_.orc_uniform(int(kw["seed"]), j, int(kw["iteration"]), 0, k))
        z = float(L_.orc_normal(int(kw["seed"]), j, int(kw["iteration"]), 0, k))
        if u < prob:
            dl[k] = f(1); b[k] = f(float(g1) + z * float(np.sqrt(inv1)))
        else:
            dl[k] = f(0); b[k] = f(float(g0) + z * float(np.sqrt(inv0)))
        out.append((float(prob), u))
    return out
