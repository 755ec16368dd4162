"""The GWAS session of the C ABI (jwas_hip_gwas_begin / _sample / _local_ebv / _end; src/3.GWAS/src/GWAS.jl:149-173) on the
device: window sums bit-identical to jwas_hip_window_sums on the CSR description `gwas.py` builds for the same sample, local
EBVs within the derived bound of the Float64 numpy mean (gwas_session_standin.local_ebv_bound:
|device - numpy64| <= (K_w + 4 S) 2^-52 A_iw), every error code, and GWAS(..., local_EBV=true) end to end."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from gwas_session_standin import csr_of_sample, local_ebv_bound
from jwas_jl_amd import api
from jwas_jl_amd import streaming as S

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_7animals")


def _load(kind, n, p, seed):
    """(engine, the decoded matrix the device holds)"""
    import jwas_jl_amd as J
    rng = np.random.default_rng(seed)
    if kind == "f64":
        e = J.HipEngine(0, precision=64)
        X = np.asfortranarray(rng.standard_normal((n, p)))
        e.load_dense(X)
    elif kind == "dense":
        e = J.HipEngine(0)
        X = np.asfortranarray(rng.standard_normal((n, p)).astype(np.float32))
        e.load_dense(X)
    else:                                              # 2-bit packed, codes 0 / 1 / 2 and 3 = missing (as tests/test_gpu_packed.py)
        e = J.HipEngine(0)
        raw = rng.integers(0, 3, size=(n, p)).astype(np.float64)
        raw[rng.integers(0, n, 60), rng.integers(0, p, 60)] = 9
        miss = raw == 9
        codes = np.where(miss, 3, raw).astype(np.uint8)
        means = np.array([raw[~miss[:, j], j].mean(dtype=np.float32) for j in range(p)], dtype=np.float32)
        v = np.where(miss, means[None, :], raw.astype(np.float32)).astype(np.float32)
        X = np.asfortranarray(v - means[None, :])
        e.load_packed2bit(S.pack_2bit(codes), n, means, centered=True)
    return e, X


def _check_session(e, X, cs, ce, samples, use_out):
    """Feeds the samples; sums == window_sums on the CSR, local EBVs within the bound, nsamples right."""
    n, nwin = X.shape[0], len(cs)
    X64 = np.asarray(X, dtype=np.float64)
    want = np.zeros((n, nwin))
    for a in samples:
        nz = np.flatnonzero(a)
        s, q = e.gwas_sample(nz, a[nz])
        wptr, gather = csr_of_sample(nz, cs, ce)
        s0, q0 = e.window_sums(wptr, gather, a[gather], use_output_rows=use_out)
        assert s.shape == (nwin + 1,) and np.array_equal(s, s0) and np.array_equal(q, q0)
        a64 = a.astype(np.float64)
        for w in range(nwin):
            want[:, w] += X64[:, cs[w]:ce[w]] @ a64[cs[w]:ce[w]]
    want /= len(samples)
    got, ns = e.gwas_local_ebv()
    assert ns == len(samples) and got.shape == (n, nwin)
    bound = local_ebv_bound(X, samples, cs, ce)
    err = np.abs(got - want)
    print("max |err| / bound:", float((err / np.where(bound > 0, bound, 1)).max()), " max |local EBV|:", float(np.abs(want).max()))
    assert (err <= bound).all()
    return got


def _windows_40(p):
    """40 windows over p = 3000 columns: 30 disjoint ones of 80, a single-marker one, one no sample touches, 8 overlapping."""
    cs = [80 * k for k in range(30)] + [2400, 2500] + [100 + 150 * k for k in range(8)]
    ce = [80 * (k + 1) for k in range(30)] + [2401, 2600] + [100 + 150 * k + 400 for k in range(8)]
    assert len(cs) == 40 and max(ce) <= p
    return np.array(cs), np.array(ce)


@pytest.mark.parametrize("kind", ["dense", "packed", "f64"])
def test_session_sums_are_window_sums_and_local_ebvs_match_numpy(kind):
    n, p, n_out = 700, 3000, 300
    e, X = _load(kind, n, p, 21)
    try:
        rng = np.random.default_rng(5)
        cs, ce = _windows_40(p)
        samples = np.where(rng.random((12, p)) < 0.03, rng.standard_normal((12, p)), 0.0)
        samples[4] = 0.0                                        # nnz = 0
        samples[7] = rng.standard_normal(p)                     # every effect nonzero
        samples[:, 2500:2600] = 0.0                             # window 31: no nonzero effect in any sample
        samples[:, 2400] = rng.standard_normal(12)              # the single-marker window is hit
        samples[4] = 0.0
        samples = samples.astype(e.dtype)
        e.gwas_begin(cs, ce, local_ebv=True)
        assert e.gwas_geometry() == {"nslices": 3, "windows_per_chunk": 1, "nchunks": 41}
        got = _check_session(e, X, cs, ce, samples, False)
        assert not got[:, 31].any() and np.abs(got[:, 30]).max() > 0
        # a second begin restarts the session: clean accumulator, counter 0
        e.gwas_begin(cs, ce, local_ebv=True)
        z, ns = e.gwas_local_ebv()
        assert ns == 0 and not z.any()
        got2 = _check_session(e, X, cs, ce, samples[:3], False)
        assert not np.array_equal(got2, got)
        # the output rows (Mi.output_genotypes)
        rows = rng.permutation(n)[:n_out]
        Xo = np.asfortranarray(np.asarray(X)[rows, :])
        e.load_output_dense(Xo)
        e.gwas_begin(cs, ce, local_ebv=True, use_output_rows=True)
        assert e.gwas_geometry()["nslices"] == 2
        _check_session(e, Xo, cs, ce, samples, True)
        # sums only: same bits, no accumulator
        e.gwas_begin(cs, ce, local_ebv=False)
        nz = np.flatnonzero(samples[0])
        s, q = e.gwas_sample(nz, samples[0][nz])
        wptr, gather = csr_of_sample(nz, cs, ce)
        s0, q0 = e.window_sums(wptr, gather, samples[0][gather])
        assert np.array_equal(s, s0) and np.array_equal(q, q0)
        e.gwas_end()
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["dense", "f64"])
def test_many_slices_and_window_chunks(kind):
    n, p, nwin = 5200, 8000, 200
    e, X = _load(kind, n, p, 22)
    try:
        rng = np.random.default_rng(6)
        cs = np.arange(nwin) * 40
        ce = cs + 40
        ce[::7] += 60                                           # some windows reach into their neighbours
        ce = np.minimum(ce, p)
        samples = np.where(rng.random((20, p)) < 0.02, rng.standard_normal((20, p)), 0.0).astype(e.dtype)
        e.gwas_begin(cs, ce, local_ebv=True)
        g = e.gwas_geometry()
        # the documented rule: 256-row slices; windows per chunk = max(1, cld(nwin * nslices, 2048)); chunk 0 = "all markers"
        assert g["nslices"] == 21 and g["windows_per_chunk"] == -(-nwin * 21 // 2048) == 3
        assert g["nchunks"] == 1 + -(-nwin // 3) and g["nchunks"] > 2
        _check_session(e, X, cs, ce, samples, False)
        e.gwas_end()
    finally:
        e.close()


def test_every_error_is_decided_before_a_launch_and_the_context_survives():
    import jwas_jl_amd as J
    EINVAL, ESTATE, EUNSUP, ENOMEM = -1, -3, -4, -5
    n, p = 300, 500
    rng = np.random.default_rng(7)
    X = np.asfortranarray(rng.standard_normal((n, p)).astype(np.float32))
    e = J.HipEngine(0)
    L, h = e._L, e._h
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(8)
    ns = C.c_int64(0)

    def expect(code, pattern, call):
        with pytest.raises(J.JwasHipError, match=pattern) as ei:
            e._chk(call())
        assert ei.value.code == code, (ei.value.code, ei.value.message)

    cs, ce = i32([0, 100, 50]), i32([100, 200, 300])
    one_i, one_f = i32([3]), np.array([1.0], dtype=np.float32)
    try:
        expect(ESTATE, "no genotype matrix", lambda: L.jwas_hip_gwas_begin(h, 0, 3, ptr(cs), ptr(ce), 1))
        e.load_dense(X)
        expect(ESTATE, "gwas_begin has not been called", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(one_i), ptr(one_f), ptr(out), ptr(out)))
        expect(ESTATE, "gwas_begin has not been called", lambda: L.jwas_hip_gwas_local_ebv(h, ptr(out), C.byref(ns)))
        expect(ESTATE, "load_output_dense_f32 has not been called", lambda: L.jwas_hip_gwas_begin(h, 1, 3, ptr(cs), ptr(ce), 1))
        expect(EINVAL, "NULL", lambda: L.jwas_hip_gwas_begin(h, 0, 3, None, ptr(ce), 1))
        expect(EINVAL, "nwin must be >= 1", lambda: L.jwas_hip_gwas_begin(h, 0, 0, ptr(cs), ptr(ce), 1))
        expect(EINVAL, "col_start 100 > col_end 99", lambda: L.jwas_hip_gwas_begin(h, 0, 3, ptr(cs), ptr(i32([100, 99, 300])), 1))
        expect(EINVAL, r"outside \[0, 500\]", lambda: L.jwas_hip_gwas_begin(h, 0, 3, ptr(cs), ptr(i32([100, 200, 501])), 1))
        expect(EINVAL, r"outside \[0, 500\]", lambda: L.jwas_hip_gwas_begin(h, 0, 3, ptr(i32([-1, 100, 50])), ptr(ce), 1))
        # an allocation that fails: 300 -> 512 padded rows x 10^8 windows x 8 bytes = 410 GB of accumulator
        big = 100_000_000
        zs = np.zeros(big, dtype=np.int32)
        expect(ENOMEM, "x 100000000 windows x 8 bytes", lambda: L.jwas_hip_gwas_begin(h, 0, big, ptr(zs), ptr(zs), 1))
        del zs
        expect(ESTATE, "gwas_begin has not been called", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(one_i), ptr(one_f), ptr(out), ptr(out)))
        e.gwas_begin(cs, ce, local_ebv=False)
        expect(ESTATE, "without local_ebv", lambda: L.jwas_hip_gwas_local_ebv(h, ptr(out), C.byref(ns)))
        expect(EINVAL, "NULL", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(one_i), ptr(one_f), None, ptr(out)))
        expect(EINVAL, "idx / val is NULL", lambda: L.jwas_hip_gwas_sample(h, 1, None, ptr(one_f), ptr(out), ptr(out)))
        expect(EINVAL, "strictly ascending", lambda: L.jwas_hip_gwas_sample(h, 2, ptr(i32([5, 5])), ptr(np.ones(2, dtype=np.float32)), ptr(out), ptr(out)))
        expect(EINVAL, "strictly ascending", lambda: L.jwas_hip_gwas_sample(h, 2, ptr(i32([5, 4])), ptr(np.ones(2, dtype=np.float32)), ptr(out), ptr(out)))
        expect(EINVAL, "out of range", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(i32([p])), ptr(one_f), ptr(out), ptr(out)))
        expect(EINVAL, "out of range", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(i32([-2])), ptr(one_f), ptr(out), ptr(out)))
        expect(ESTATE, "Float64 context", lambda: L.jwas_hip_gwas_sample_f64(h, 1, ptr(one_i), ptr(np.ones(1)), ptr(out), ptr(out)))
        # ... and the session and the context still work
        s, q = e.gwas_sample(one_i, one_f)
        x = X[:, 3].astype(np.float64)
        np.testing.assert_allclose(s, [x.sum(), x.sum(), 0.0, 0.0], rtol=1e-12)
        # reloading the genotypes ends the session
        e.load_dense(X)
        expect(ESTATE, "gwas_begin has not been called", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(one_i), ptr(one_f), ptr(out), ptr(out)))
        wptr = i32([0, 1])
        s, q = e.window_sums(wptr, one_i, one_f)
        np.testing.assert_allclose([s[0], q[0]], [x.sum(), (x * x).sum()], rtol=1e-12)
        e.gwas_end()                                            # (no session: a no-op)
    finally:
        e.close()
    e = J.HipEngine(0, precision=64)
    try:
        e.load_dense(np.asfortranarray(X.astype(np.float64)))
        e.gwas_begin(cs, ce, local_ebv=True)
        L, h = e._L, e._h
        expect(EUNSUP, "use jwas_hip_gwas_sample_f64", lambda: L.jwas_hip_gwas_sample(h, 1, ptr(one_i), ptr(one_f), ptr(out), ptr(out)))
        s, q = e.window_sums(i32([0, 1]), one_i, np.ones(1))
        np.testing.assert_allclose(s[0], X[:, 3].astype(np.float64).sum(), rtol=1e-12)
    finally:
        e.close()


def test_local_ebv_end_to_end_on_demo_data(tmp_path):
    pheno = pd.read_csv(os.path.join(DEMO, "phenotypes.txt"), na_values=["NA"], dtype={"ID": str})
    geno = api.get_genotypes(os.path.join(DEMO, "genotypes.txt"), 1.0, separator=",", method="BayesC")
    model = api.build_model("y1 = intercept + geno", 1.0)
    api.outputEBV(model, geno.obsID)
    folder = tmp_path / "chain"
    api.runMCMC(model, pheno, chain_length=100, burnin=20, output_samples_frequency=10, outputEBV=True, output_folder=str(folder), seed=123)
    marker_file = str(folder / "MCMC_samples_marker_effects_geno_y1.txt")
    mapfile = os.path.join(DEMO, "map.txt")
    a, b = tmp_path / "off", tmp_path / "on"
    a.mkdir(); b.mkdir()
    r0 = api.GWAS(model, mapfile, marker_file, window_size="1 Mb", header=True, output_folder=str(a))
    r1 = api.GWAS(model, mapfile, marker_file, window_size="1 Mb", header=True, local_EBV=True, output_folder=str(b))
    pd.testing.assert_frame_equal(r0[0], r1[0], check_exact=True)
    assert open(a / "MCMC_samples_local_genomic_variance1.txt", "rb").read() == open(b / "MCMC_samples_local_genomic_variance1.txt", "rb").read()
    tab = pd.read_csv(b / "localEBV1.txt", dtype={"ID": str})
    Mi = model.M[0]
    rows = Mi.output_rows
    assert list(tab.columns) == ["ID", "w1", "w2", "w3"]
    assert list(tab["ID"]) == [Mi.obsID[r] for r in rows] and len(tab) == len(geno.obsID)
    smp = pd.read_csv(marker_file).to_numpy(dtype=np.float32)
    Xo = np.asarray(Mi.genotypes[rows, :], dtype=np.float32)
    cs, ce = [0, 2, 3], [2, 3, 5]                               # map.txt: chr 1 [0, 1 Mb), [1, 2 Mb); chr 2 [0, 1 Mb)
    want = np.zeros((Xo.shape[0], 3))
    for s in smp.astype(np.float64):
        for w in range(3):
            want[:, w] += Xo[:, cs[w]:ce[w]].astype(np.float64) @ s[cs[w]:ce[w]]
    want /= smp.shape[0]
    got = tab.iloc[:, 1:].to_numpy(dtype=np.float64)
    assert smp.shape[0] == 8 and (np.abs(got - want) <= local_ebv_bound(Xo, smp, cs, ce)).all()
