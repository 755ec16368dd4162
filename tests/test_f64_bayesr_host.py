"""The Float64 BayesR block restatement (tests/f64_bayesr_reference.py) pinned to the literal C chain (oracle.bayesr_sweep64)
where the two must agree: one pass per block, no weights, a uniform partition.  No GPU.  The restatement is what the device's
BayesR Float64 path is judged by beyond the plain pass (repetitions, weights, ragged partitions, independent blocks), so it is
held to the existing reference first."""
import numpy as np
import pytest

from conftest import make_dataset
from oracle_engine import OracleEngine64
from f64_bayesr_reference import BayesROracleEngine64, bayesr_block_sweep
from test_gpu_f64 import _compare


def _engines(n, p, bs, seed):
    d = make_dataset(n=n, p=p, ncausal=8, seed=seed)
    X = np.asfortranarray(d["X"].astype(np.float64))
    lit, ref = OracleEngine64(), BayesROracleEngine64()
    for e in (lit, ref):
        e.load_dense(X); e.setup_blocks(bs); e.init_state("BayesR", 1)
        e.set_residual(d["y"] - d["y"].mean())
        e.set_state(0, delta=np.ones(p, dtype=np.int32))
    return lit, ref


@pytest.mark.parametrize("n,p,bs,prior_matrix", [(300, 64 * 3 + 17, 64, False), (257, 223 + 90, 223, True)])
def test_block_restatement_reproduces_the_literal_chain(n, p, bs, prior_matrix):
    lit, ref = _engines(n, p, bs, seed=3 + bs)
    kw = dict(vare=0.5, var_effect=0.05, pi_classes=np.array([0.9, 0.05, 0.03, 0.02]))
    if prior_matrix:
        kw["pi_matrix"] = np.random.default_rng(1).dirichlet([20, 2, 1, 1], size=p)
    for it in range(1, 13):
        so = lit.sweep(iteration=it, seed=9, **kw)
        sr = ref.sweep(iteration=it, seed=9, **kw)
        assert np.array_equal(lit.delta, ref.delta), f"iteration {it}: classes differ at {np.flatnonzero(lit.delta[0] != ref.delta[0])[:5]}"
        assert np.array_equal(so["class_counts"], sr["class_counts"]) and so["n_events"] == sr["n_events"]
        assert so["bayesr_nnz"] == sr["bayesr_nnz"]
        np.testing.assert_allclose(sr["bayesr_ssq"], so["bayesr_ssq"], rtol=1e-9)
        np.testing.assert_allclose(sr["resid_ss"], so["resid_ss"], rtol=1e-9)
    assert (ref.delta > 1).any() and (ref.delta == 1).any()          # (the chain moves between the classes)
    _compare(lit, ref, 1)


@pytest.mark.parametrize("nreps,weighted", [(1, False), (3, True)])
def test_independent_single_block_equals_the_sequential_form_bit_for_bit(nreps, weighted):
    """One block holds every marker: its right-hand sides come from the residual at the start of the sweep either way."""
    n, p = 120, 90
    d = make_dataset(n=n, p=p, ncausal=5, seed=11)
    X = np.asfortranarray(d["X"].astype(np.float64))
    rng = np.random.default_rng(4)
    w = 1.0 + rng.uniform(0, 1.5, n) if weighted else None
    ww = np.ones(n) if w is None else w
    xpx = (X * X * ww[:, None]).sum(axis=0)
    pi = rng.dirichlet([10, 2, 1, 1], size=p)
    out = []
    for independent in (False, True):
        r = d["y"] - d["y"].mean()
        alpha, delta = np.zeros(p), np.ones(p, dtype=np.int32)
        for it in range(1, 6):
            bayesr_block_sweep(X, xpx, r, alpha, delta, 0.5, 0.05, pi, 7, it, np.array([0]), nreps=nreps, independent=independent,
                               w=w, marker0=1000)
        out.append((r, alpha, delta))
    assert (out[0][2] > 1).any()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_repetitions_use_their_own_draws():
    """The repetition is part of the draw's counter: a second pass over a block is not a replay of the first."""
    lit, ref = _engines(200, 70, 64, seed=5)
    one, two = BayesROracleEngine64(), ref
    one.load_dense(ref.X); one.setup_blocks(64); one.init_state("BayesR", 1)
    one.set_residual(ref.get_residual(0)); one.set_state(0, delta=np.ones(70, dtype=np.int32))
    kw = dict(iteration=1, seed=9, vare=0.5, var_effect=0.05, pi_classes=np.array([0.5, 0.2, 0.2, 0.1]))
    one.sweep(nreps=1, **kw)
    two.sweep(nreps=2, **kw)
    assert not np.array_equal(one.alpha, two.alpha)
