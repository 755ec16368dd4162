"""The output side of a Float64 device context (jwas_hip_set_precision(ctx, 64)): the sparse sample readout
(jwas_hip_get_alpha_sparse_f64), EBVs over the nonzero effects for the training rows and for a second resident matrix
(jwas_hip_mul_alpha_f64, jwas_hip_load_output_dense_f64 / jwas_hip_mul_alpha_output_f64) and the window sums of the GWAS
(jwas_hip_window_sums_f64 / _sums2_f64), all through the C ABI on a HipEngine(0, precision=64).

Stated contracts: the compacted lists are exact; X*alpha is ONE fused multiply-add per nonzero effect in marker order, so it is
checked bit for bit against an exact (rational) restatement of that chain, and the output rows give the bits of the training rows
they were copied from; the window sums differ from numpy only in the association of fp64 sums."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from f64_mt_reference import RestatementEngine64
from test_f64_outputs_host import _run as run_subset_case

pytestmark = pytest.mark.gpu

ESTATE, EUNSUP = -3, -4


def _engine(n, p, t=1, method="BayesC", seed=0, real=True, bs=64):
    import jwas_jl_amd as J
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, size=(n, p)).astype(np.float64)
    if real:
        X += 0.3 * rng.standard_normal((n, p))                  # real-valued genotypes: every product rounds
    X = np.asfortranarray(X - X.mean(0))
    hip = J.HipEngine(0, precision=64)
    hip.load_dense(X); hip.setup_blocks(bs); hip.init_state(method, t)
    return hip, X, rng


def _sparse_vec(rng, p, nnz):
    a = np.zeros(p)
    a[rng.choice(p, size=nnz, replace=False)] = rng.standard_normal(nnz)
    return a


def _fma_chain(X, a):
    """per row, over the nonzero effects in marker order: acc = fl(a_j * x_ij + acc), one rounding per term (CPython rounds
    Fraction -> float correctly) -- the arithmetic of k64_mul_alpha / k64_mul_alpha_list"""
    nz = np.flatnonzero(a)
    out = np.zeros(X.shape[0])
    for i in range(X.shape[0]):
        acc = 0.0
        for j in nz:
            acc = float(Fraction(float(a[j])) * Fraction(float(X[i, j])) + Fraction(acc))
        out[i] = acc
    return out


def test_sparse_readout_is_exact():
    hip, X, rng = _engine(500, 900, seed=1)
    try:
        y = X[:, :6] @ rng.standard_normal(6) + rng.standard_normal(500)
        hip.set_residual(y - y.mean())
        for it in range(1, 5):
            hip.sweep(iteration=it, seed=3, vare=1.0, var_effect=0.05, pi=0.95)
        a = hip.get_state()[0]
        assert 0 < np.count_nonzero(a) < 900
        idx, val = hip.alpha_sparse()
        assert idx.dtype == np.int32 and val.dtype == np.float64
        assert np.array_equal(idx, np.flatnonzero(a)) and np.array_equal(val, a[idx])
        # no nonzero effect at all
        hip.set_state(alpha=np.zeros(900))
        idx, val = hip.alpha_sparse()
        assert idx.size == 0 and val.size == 0
        # more nonzero effects than the first capacity: the call reports the count, the engine grows and asks again
        a = _sparse_vec(rng, 900, 333)
        hip.set_state(alpha=a)
        hip._sparse_cap = 4
        idx, val = hip.alpha_sparse()
        assert hip._sparse_cap >= 333
        assert np.array_equal(idx, np.flatnonzero(a)) and np.array_equal(val, a[idx])
        nnz = C.c_int64(-1)
        rc = hip._L.jwas_hip_get_alpha_sparse_f64(hip._h, 0, 4, idx[:4].ctypes.data_as(C.c_void_p), val[:4].ctypes.data_as(C.c_void_p), C.byref(nnz))
        assert rc != 0 and nnz.value == 333
        a = rng.standard_normal(900)                            # every effect nonzero
        hip.set_state(alpha=a)
        idx, val = hip.alpha_sparse()
        assert np.array_equal(idx, np.arange(900)) and np.array_equal(val, a)
    finally:
        hip.close()


@pytest.mark.parametrize("nnz", [0, 1, 37, 100])
def test_mul_alpha_is_the_fma_chain_bit_for_bit(nnz):
    """(passes before and after the move to compact + list: it pins that the move changes no bit)"""
    hip, X, rng = _engine(300, 2000, seed=10 + nnz)
    try:
        a = _sparse_vec(rng, 2000, nnz)
        hip.set_state(alpha=a)
        got = hip.mul_alpha()
        want = _fma_chain(X, a)
        assert got.dtype == np.float64
        if nnz:
            assert np.abs(want).max() > 0.1
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of 300 rows differ, max {np.abs(got - want).max():.3e}"
    finally:
        hip.close()


def test_output_rows_give_the_bits_of_the_training_rows():
    n, p, t = 700, 1200, 2
    hip, X, rng = _engine(n, p, t=t, method="MTBayesC", seed=4)
    try:
        for k in range(t):
            hip.set_state(k, alpha=_sparse_vec(rng, p, 40 + 150 * k))
        full = [hip.mul_alpha(k) for k in range(t)]
        for k in range(t):
            np.testing.assert_allclose(full[k], X @ hip.get_state(k)[0], rtol=0, atol=1e-11)
        with pytest.raises(TypeError, match="float64"):
            hip.load_output_dense(X[:10].astype(np.float32))
        for n_out in (300, 256, 7):                            # each load replaces the one before; 300 and 7 are no multiples of 256
            rows = rng.permutation(n)[:n_out]
            hip.load_output_dense(X[rows])
            for k in range(t):
                got = hip.mul_alpha_output(k)
                assert got.shape == (n_out,) and got.dtype == np.float64
                assert np.array_equal(got, full[k][rows])
        hip.set_state(1, alpha=np.zeros(p))                     # the state changes, the resident rows stay
        assert np.array_equal(hip.mul_alpha_output(1), np.zeros(7))
        assert np.array_equal(hip.mul_alpha_output(0), full[0][rows])
    finally:
        hip.close()


def _windows(rng, p, nz):
    """CSR description as GWAS() builds it: window 0 = all nonzero effects, then disjoint windows, one of them empty"""
    edges = [0, p // 5, p // 5, p // 2, p]                      # (the second window holds no marker at all)
    parts = [nz] + [nz[(nz >= lo) & (nz < hi)] for lo, hi in zip(edges[:-1], edges[1:])]
    wptr = np.concatenate([[0], np.cumsum([len(q) for q in parts])]).astype(np.int32)
    return wptr, np.concatenate(parts).astype(np.int32)


def _numpy_sums(X, wptr, idx, v1, v2=None):
    nw = len(wptr) - 1
    outs = np.zeros((5, nw)); mass = np.zeros((2, nw))
    for w in range(nw):
        sl = slice(wptr[w], wptr[w + 1])
        cols = X[:, idx[sl]]
        b1 = cols @ v1[sl]
        b2 = cols @ v2[sl] if v2 is not None else np.zeros_like(b1)
        outs[:, w] = b1.sum(), (b1 * b1).sum(), b2.sum(), (b2 * b2).sum(), (b1 * b2).sum()
        mass[:, w] = np.abs(b1).sum(), np.abs(b2).sum()
    return outs, mass


@pytest.mark.parametrize("use_output_rows", [False, True])
def test_window_sums_against_numpy(use_output_rows):
    n, p = 900, 1500
    hip, X, rng = _engine(n, p, seed=6)
    try:
        Xr = X
        if use_output_rows:
            rows = rng.permutation(n)[:333]
            Xr = X[rows]
            Xr = Xr - Xr.mean(0)                               # (centred like the training rows, so the raw sums cancel here too)
            hip.load_output_dense(Xr)
        m = Xr.shape[0]
        a1, a2 = _sparse_vec(rng, p, 120), _sparse_vec(rng, p, 90)
        nz = np.flatnonzero(a1)
        wptr, idx = _windows(rng, p, nz)
        assert wptr[2] == wptr[1] + np.count_nonzero(nz < p // 5) and wptr[3] == wptr[2]          # window 2 is empty
        s, q = hip.window_sums(wptr, idx, a1[idx], use_output_rows=use_output_rows)
        want, mass = _numpy_sums(Xr, wptr, idx, a1[idx])
        var = lambda q_, s_: (q_ - s_ * s_ / m) / (m - 1)
        assert np.all(np.abs(s - want[0]) <= 1e-12 * mass[0])          # (sums of centred genotypes cancel: bounded by sum |BV|)
        np.testing.assert_allclose(var(q, s), var(want[1], want[0]), rtol=1e-10)
        assert s[2] == 0.0 and q[2] == 0.0 and var(q, s)[0] > 0
        # two effect vectors over the union of their nonzero effects
        nz2 = np.flatnonzero((a1 != 0) | (a2 != 0))
        wptr, idx = _windows(rng, p, nz2)
        got = hip.window_sums2(wptr, idx, a1[idx], a2[idx], use_output_rows=use_output_rows)
        want, mass = _numpy_sums(Xr, wptr, idx, a1[idx], a2[idx])
        for g, w_, ms in ((got[0], want[0], mass[0]), (got[2], want[2], mass[1])):
            assert np.all(np.abs(g - w_) <= 1e-12 * ms)
        np.testing.assert_allclose(var(got[1], got[0]), var(want[1], want[0]), rtol=1e-10)
        np.testing.assert_allclose(var(got[3], got[2]), var(want[3], want[2]), rtol=1e-10)
        cov = lambda c_, s1_, s2_: (c_ - s1_ * s2_ / m) / (m - 1)
        np.testing.assert_allclose(cov(got[4], got[0], got[2]), cov(want[4], want[0], want[2]), rtol=1e-10)
        assert np.all(np.asarray(got)[:, 2] == 0.0)
    finally:
        hip.close()


def test_runmcmc_double_precision_id_subset_gpu_vs_restatement(tmp_path):
    """runMCMC(double_precision=true) with outputEBV(model, IDs) naming a permuted strict subset: the device (output rows resident,
    samples read out sparse) against the same host loop on the restatement engine (host product), same seed."""
    rng = np.random.default_rng(9)
    ids_out = [f"id{i}" for i in rng.permutation(180)[:70]]
    out_ref = run_subset_case(RestatementEngine64(), tmp_path, "ref", ids_out)
    out_hip = run_subset_case(None, tmp_path, "hip", ids_out)
    eo, eh = out_ref["marker effects geno"], out_hip["marker effects geno"]
    np.testing.assert_allclose(eh["Estimate"].to_numpy(dtype=np.float64), eo["Estimate"].to_numpy(dtype=np.float64), atol=1e-8)
    np.testing.assert_allclose(eh["Model_Frequency"].to_numpy(dtype=np.float64), eo["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)
    for k in ("y1", "y2"):
        assert list(out_hip[f"EBV_{k}"]["ID"]) == ids_out
        np.testing.assert_allclose(out_hip[f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64), out_ref[f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64), atol=1e-7)


def test_precision_guards_name_the_twin():
    import jwas_jl_amd as J
    hip, X, rng = _engine(300, 200, seed=2)
    f32 = J.HipEngine(0)
    try:
        f32.load_dense(np.asfortranarray(X.astype(np.float32))); f32.setup_blocks(64); f32.init_state("BayesC")
        L = hip._L
        buf = np.zeros(4096)                                    # (large enough for every out-array below, whatever its element type)
        ib = np.zeros(4096, dtype=np.int32)
        wptr = np.array([0, 1], dtype=np.int32)
        nnz = C.c_int64(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        f32_calls = {
            "jwas_hip_get_alpha_sparse": lambda h: L.jwas_hip_get_alpha_sparse(h, 0, 4096, vp(ib), vp(buf), C.byref(nnz)),
            "jwas_hip_load_output_dense_f32": lambda h: L.jwas_hip_load_output_dense_f32(h, vp(buf), 4, 200, 4),
            "jwas_hip_mul_alpha_output": lambda h: L.jwas_hip_mul_alpha_output(h, 0, vp(buf)),
            "jwas_hip_window_sums": lambda h: L.jwas_hip_window_sums(h, 0, 1, vp(wptr), vp(ib), vp(buf), vp(buf), vp(buf)),
            "jwas_hip_window_sums2": lambda h: L.jwas_hip_window_sums2(h, 0, 1, vp(wptr), vp(ib), vp(buf), vp(buf), *[vp(buf)] * 5),
        }
        twin = {"jwas_hip_load_output_dense_f32": "jwas_hip_load_output_dense_f64"}
        for name, call in f32_calls.items():
            assert call(hip._h) == EUNSUP, name
            msg = L.jwas_hip_last_error(hip._h).decode()
            assert twin.get(name, name + "_f64") in msg and "Float64 context" in msg, (name, msg)
        f64_calls = {
            "jwas_hip_get_alpha_sparse_f64": lambda h: L.jwas_hip_get_alpha_sparse_f64(h, 0, 4096, vp(ib), vp(buf), C.byref(nnz)),
            "jwas_hip_load_output_dense_f64": lambda h: L.jwas_hip_load_output_dense_f64(h, vp(buf), 4, 200, 4),
            "jwas_hip_mul_alpha_output_f64": lambda h: L.jwas_hip_mul_alpha_output_f64(h, 0, vp(buf)),
            "jwas_hip_window_sums_f64": lambda h: L.jwas_hip_window_sums_f64(h, 0, 1, vp(wptr), vp(ib), vp(buf), vp(buf), vp(buf)),
            "jwas_hip_window_sums2_f64": lambda h: L.jwas_hip_window_sums2_f64(h, 0, 1, vp(wptr), vp(ib), vp(buf), vp(buf), *[vp(buf)] * 5),
        }
        for name, call in f64_calls.items():
            assert call(f32._h) == ESTATE, name
            assert "Float64 context" in L.jwas_hip_last_error(f32._h).decode()
        # a Float64 context without output rows says which call is missing
        with pytest.raises(J.JwasHipError, match="jwas_hip_load_output_dense_f64") as ei:
            hip.mul_alpha_output()
        assert ei.value.code == ESTATE
    finally:
        hip.close(); f32.close()
