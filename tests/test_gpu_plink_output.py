"""EBVs for individuals of a PLINK fileset outside the training set (jwas_hip_plink_commit_output, jwas_hip_load_output_packed2bit,
jwas_hip_get_output_packed2bit, jwas_hip_ebv_output; csrc/output.hpp k_ebv_packed): the output rows as a second 2-bit packed matrix
decoded with the training set's selection, counted allele and means.  Everything is compared bit for bit -- with the host reader, with
the training-row kernels on the same individuals, with a second engine that holds the same rows dense -- and once against numpy in double.

The fileset: 1 003 individuals (n % 4 = 3), 100 markers of which ten are monomorphic; training: a shuffled 301; the output sets: 1, 5,
257, 700 individuals (more than the training ld of 512) and all 1 003 in file order (the direct transcode)."""
import contextlib
import io

import numpy as np
import pytest

import grm_packed_reference as PKR
import plink_reference as PR
from jwas_jl_amd import plink as P

pytestmark = pytest.mark.gpu

N_FILE, P_FILE, N_TRAIN = 1003, 100, 301
SETS = (1, 5, 257, 700)
EINVAL, ESTATE, EUNSUP = -1, -3, -4


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


@pytest.fixture(scope="module")
def engines():
    import jwas_jl_amd as J
    a, b = J.HipEngine(0), J.HipEngine(0)
    yield a, b
    a.close(); b.close()


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    """The fileset, the training rows, and the output rows of every set.  Marker 20 is missing for every individual outside the
    training set; markers 3, 13, .. 93 are monomorphic."""
    d = tmp_path_factory.mktemp("plink_output_gpu")
    rng = np.random.default_rng(41)
    f = rng.uniform(0.1, 0.5, P_FILE)
    G = (rng.random((N_FILE, P_FILE)) < f).astype(np.int64) + (rng.random((N_FILE, P_FILE)) < f).astype(np.int64)
    G[rng.random((N_FILE, P_FILE)) < 0.02] = 9
    G[:, 3::10] = 2
    train_rows = np.random.default_rng(5).permutation(N_FILE)[:N_TRAIN]
    outside = np.setdiff1d(np.arange(N_FILE), train_rows)
    G[outside, 20] = 9
    ids, _, _, _ = PR.write_fileset(d / "g", G)
    r9 = np.random.default_rng(9)
    sets = {k: r9.permutation(outside)[:k] for k in SETS}
    sets["all"] = np.arange(N_FILE)
    return {"prefix": str(d / "g"), "G": G, "ids": ids, "train_rows": train_rows, "sets": sets, "dir": d}


def _train(eng, fs, counted="A1", center=True):
    """The training set into `eng`; (the backend dict, the count matrix of the counted allele)."""
    b = _quiet(P.load_plink, eng, fs["prefix"], keep=[fs["ids"][i] for i in fs["train_rows"]], counted_allele=counted, center=center)
    return b, PR.read_bed(fs["prefix"] + ".bed", N_FILE, P_FILE, counted)


def _effects(p, t, seed):
    """t effect vectors with different, overlapping nonzero sets; with t >= 2 trait 1 is all zero, with t = 4 trait 3 fully dense."""
    rng = np.random.default_rng(seed)
    A = np.zeros((t, p), dtype=np.float32)
    for k in range(t):
        nz = rng.permutation(p)[:7 + 5 * k]
        A[k, nz] = rng.standard_normal(nz.size).astype(np.float32)
    if t >= 2:
        A[1] = 0
    if t == 4:
        A[3] = rng.standard_normal(p).astype(np.float32)
        A[3][A[3] == 0] = 1
    A[0, :4] = [0.5, -0.25, 0, 1.5]                                                   # (overlaps whatever trait 2 drew)
    return A


def _set_effects(eng, A):
    eng.init_state("BayesC" if A.shape[0] == 1 else "MTBayesC", A.shape[0])
    for k in range(A.shape[0]):
        eng.set_state(k, alpha=A[k])


# ---- 1. the payload --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counted", ["A1", "A2"])
def test_committed_payload_equals_the_reader(engines, fileset, counted):
    dev, _ = engines
    b, M = _train(dev, fileset, counted)
    sel, src = b["selected"], b["source"]
    assert 20 in sel and sel.size < P_FILE
    training = dev.get_packed2bit(0, dev.p)
    for name, rows in fileset["sets"].items():
        assert P.load_plink_output(dev, src, [fileset["ids"][i] for i in rows]) == rows.size == dev.n_out
        codes = PR.codes_of(M[rows][:, sel])
        assert np.array_equal(dev.get_output_packed2bit(0, dev.p), PR.pack_codes(codes)), name
        if name != "all":
            assert np.all(codes[:, list(sel).index(20)] == 3)                        # the all-missing marker
        assert np.array_equal(dev.get_output_packed2bit(3, 2), PR.pack_codes(codes)[3:5])
    assert np.array_equal(dev.get_packed2bit(0, dev.p), training) and dev.n == N_TRAIN


@pytest.mark.parametrize("n_out", [1, 5, 257, 700])
def test_pad_fields_of_a_host_payload_do_not_show(engines, fileset, n_out):
    """load_output_packed2bit of a payload whose fields at rows >= n_out hold 1 and 3, in a stride wider than cld(n_out,4): the EBVs
    are those of the clean payload, bit for bit -- the pad mask is n_out's, not the training n's."""
    dev, _ = engines
    b, M = _train(dev, fileset)
    rows = fileset["sets"][n_out]
    clean = PR.pack_codes(PR.codes_of(M[rows][:, b["selected"]]))
    width = clean.shape[1]
    A = _effects(dev.p, 2, 3)
    A[1] = np.random.default_rng(4).standard_normal(dev.p).astype(np.float32)        # (a dense trait: the loop over all markers)
    _set_effects(dev, A)
    dev.load_output_packed2bit(clean, n_out)
    want = [dev.mul_alpha_output(k) for k in range(2)]
    want_all = dev.ebv_output()
    for fill in (1, 3):
        dirty = np.full((dev.p, width + 3), 0xFF, dtype=np.uint8)
        dirty[:, :width] = clean
        for i in range(n_out, 4 * width):
            dirty[:, i >> 2] |= np.uint8(fill << ((i & 3) << 1))
        dev.load_output_packed2bit(dirty, n_out)
        assert n_out % 4 == 0 or not np.array_equal(dev.get_output_packed2bit(0, dev.p), clean)
        for k in range(2):
            assert np.array_equal(dev.mul_alpha_output(k), want[k]), (fill, k)
        assert np.array_equal(dev.ebv_output(), want_all), fill


# ---- 2. the same individuals, the same bits -----------------------------------------------------------------------------------------------
def test_training_individuals_as_output_rows(engines, fileset):
    dev, _ = engines
    b, _ = _train(dev, fileset)
    perm = np.random.default_rng(12).permutation(N_TRAIN)
    ids = [fileset["ids"][fileset["train_rows"][i]] for i in perm]
    P.load_plink_output(dev, b["source"], ids)
    sparse = _effects(dev.p, 1, 5)
    dense = np.random.default_rng(6).standard_normal((1, dev.p)).astype(np.float32)
    assert np.count_nonzero(sparse) * 4 <= dev.p < np.count_nonzero(dense) * 4      # the list kernel, the loop over all markers
    for A in (sparse, dense):
        _set_effects(dev, A)
        assert np.array_equal(dev.mul_alpha_output(0), dev.mul_alpha(0)[perm])
        assert np.array_equal(dev.ebv_output()[0], dev.mul_alpha(0)[perm])


# ---- 3. packed against dense output rows, 6. window sums ----------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [True, False])
def test_packed_output_rows_equal_dense_ones(engines, fileset, center):
    """A second engine holds the same training storage and the candidates decoded on the host (Float32 code - mean, a missing code
    at the training mean): X alpha and the window sums on output rows are bit-equal."""
    dev, ref = engines
    b, M = _train(dev, fileset, center=center)
    _train(ref, fileset, center=center)
    sel = b["selected"]
    for n_out in (5, 700):
        rows = fileset["sets"][n_out]
        P.load_plink_output(dev, b["source"], [fileset["ids"][i] for i in rows])
        Xc = PKR.decode(PR.codes_of(M[rows][:, sel]), b["marker_means"], center)
        if center:
            assert np.all(Xc[:, list(sel).index(20)] == 0)                           # missing at the training mean: 0 when centred
        ref.load_output_dense(Xc)
        for A in (_effects(dev.p, 2, 7), np.random.default_rng(8).standard_normal((2, dev.p)).astype(np.float32)):
            for e in (dev, ref):
                _set_effects(e, A)
            for k in range(2):
                assert np.array_equal(dev.mul_alpha_output(k), ref.mul_alpha_output(k)), (n_out, k)
            assert np.array_equal(dev.ebv_output(), ref.ebv_output())                # (dense output rows: the traits one by one)
        a = _effects(dev.p, 1, 9)[0]
        nz = np.flatnonzero(a)
        wptr = np.array([0, nz.size, nz.size + 3, nz.size + 3, nz.size + 8], dtype=np.int32)
        idx = np.concatenate([nz, nz[:3], nz[2:7]]).astype(np.int32)
        got, want = dev.window_sums(wptr, idx, a[idx], use_output_rows=True), ref.window_sums(wptr, idx, a[idx], use_output_rows=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.any(want[1] != 0)
        a2 = np.roll(a, 1)
        got, want = (e.window_sums2(wptr, idx, a[idx], a2[idx], use_output_rows=True) for e in (dev, ref))
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 4. the kernel of all traits, 5. against numpy in double ------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 4])
def test_ebv_output_equals_mul_alpha_output_and_numpy(engines, fileset, t):
    """ebv_output()[k] is mul_alpha_output(k) bit for bit; and against numpy in double within
    |out - ref| <= 2^-24 |ref| + 2 (K + 2) 2^-53 sum_j |alpha_j x_ij|: the cast to Float32, the fma chain of K terms."""
    dev, _ = engines
    b, M = _train(dev, fileset)
    A = _effects(dev.p, t, 20 + t)
    _set_effects(dev, A)
    worst = 0.0
    for n_out in SETS:
        rows = fileset["sets"][n_out]
        P.load_plink_output(dev, b["source"], [fileset["ids"][i] for i in rows])
        E = dev.ebv_output()
        assert E.shape == (t, n_out) and E.dtype == np.float32
        X = PKR.decode(PR.codes_of(M[rows][:, b["selected"]]), b["marker_means"], True).astype(np.float64)
        for k in range(t):
            assert np.array_equal(E[k], dev.mul_alpha_output(k)), (n_out, k)
            a = A[k].astype(np.float64)
            ref, mag, K = X @ a, np.abs(X) @ np.abs(a), int(np.count_nonzero(a))
            bound = 2.0 ** -24 * np.abs(ref) + 2 * (K + 2) * 2.0 ** -53 * mag
            err = np.abs(E[k].astype(np.float64) - ref)
            if K == 0:
                assert not E[k].any()
            else:
                worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
                print(f"t={t} n_out={n_out} trait {k}: K={K}, worst |out - ref| / bound = {np.max(err / np.where(bound > 0, bound, 1.0)):.3f}")
            assert np.all(err <= bound), (n_out, k)
    print(f"t={t}: worst |out - ref| / bound over all sets = {worst:.3f}")


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(engines, fileset):
    import jwas_jl_amd as J
    dev, ref = engines
    bed = fileset["prefix"] + ".bed"

    def refused(code, match, call):
        with pytest.raises(J.JwasHipError, match=match) as ei:
            call()
        assert ei.value.code == code

    b, M = _train(dev, fileset)
    sel = b["selected"]
    _set_effects(dev, _effects(dev.p, 1, 1))
    refused(ESTATE, "jwas_hip_plink_scan has not been called", lambda: dev.plink_commit_output(sel))
    refused(ESTATE, "no 2-bit packed output rows", lambda: dev.get_output_packed2bit(0, 1))
    refused(ESTATE, "no output rows are loaded", lambda: dev.ebv_output())
    P.load_plink_output(dev, b["source"], fileset["ids"][:5])
    kept = dev.get_output_packed2bit(0, dev.p)
    dev.plink_scan(bed, N_FILE, P_FILE, [1, 2, 3])
    refused(EINVAL, "differs from the training matrix's", lambda: dev.plink_commit_output(sel[:-1]))
    refused(EINVAL, "strictly ascending", lambda: dev.plink_commit_output(sel[::-1].copy()))
    assert np.array_equal(dev.get_output_packed2bit(0, dev.p), kept) and dev.n_out == 5      # the earlier output rows are in place
    dev.plink_commit_output(sel)                                                  # (the refused commits left the scan pending)
    assert dev.n_out == 3
    refused(ESTATE, "jwas_hip_plink_scan has not been called", lambda: dev.plink_commit_output(sel))
    refused(EINVAL, "markers, the training matrix", lambda: dev.load_output_packed2bit(np.zeros((dev.p + 1, 2), dtype=np.uint8), 5))
    refused(EINVAL, "stride_bytes", lambda: dev.load_output_packed2bit(np.zeros((dev.p, 1), dtype=np.uint8), 5))
    refused(EINVAL, "marker range", lambda: dev.get_output_packed2bit(dev.p - 1, 2))
    # a session on packed output rows is out of scope; the window sums are not
    cs, ce = np.array([0, 4], dtype=np.int32), np.array([4, 9], dtype=np.int32)
    refused(EUNSUP, "2-bit packed output rows", lambda: dev.gwas_begin(cs, ce, use_output_rows=True))
    dev.gwas_begin(cs, ce)                                                        # (on the training rows it opens)
    dev.gwas_end()
    # a dense matrix replaces the packed rows, and the reverse
    dev.load_output_dense(np.zeros((6, dev.p), dtype=np.float32, order="F"))
    refused(ESTATE, "no 2-bit packed output rows", lambda: dev.get_output_packed2bit(0, 1))
    assert dev.mul_alpha_output(0).shape == (6,)
    dev.load_output_packed2bit(kept, 5)
    assert dev.mul_alpha_output(0).shape == (5,) and np.array_equal(dev.get_output_packed2bit(0, dev.p), kept)
    # a load of genotypes frees the output rows
    _train(dev, fileset)
    _set_effects(dev, _effects(dev.p, 1, 1))
    refused(ESTATE, "has not been called", lambda: dev.mul_alpha_output(0))
    # no packed training storage
    ref.load_dense(np.zeros((8, sel.size), dtype=np.float32, order="F"))
    ref.plink_scan(bed, N_FILE, P_FILE, [1, 2, 3])
    refused(ESTATE, "need 2-bit packed training storage", lambda: ref.plink_commit_output(sel))
    ref.plink_discard()
    refused(ESTATE, "need 2-bit packed training storage", lambda: ref.load_output_packed2bit(kept, 5))
    # a Float64 context
    f64 = J.HipEngine(0, precision=64)
    try:
        buf = np.zeros(16, dtype=np.uint8)
        for call in (lambda: f64._chk(f64._L.jwas_hip_load_output_packed2bit(f64._h, buf.ctypes.data, 1, 1, 1)),
                     lambda: f64._chk(f64._L.jwas_hip_plink_commit_output(f64._h, None, 0)),
                     lambda: f64._chk(f64._L.jwas_hip_get_output_packed2bit(f64._h, 0, 1, buf.ctypes.data, 1)),
                     lambda: f64._chk(f64._L.jwas_hip_ebv_output(f64._h, buf.ctypes.data))):
            refused(EUNSUP, "not available in a Float64 context", call)
        for name, args in (("load_output_packed2bit", (kept, 5)), ("plink_commit_output", (sel,)), ("get_output_packed2bit", (0, 1)), ("ebv_output", ())):
            with pytest.raises(ValueError, match="needs a Float32 engine"):
                getattr(f64, name)(*args)
    finally:
        f64.close()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------
def test_runmcmc_reports_candidates_of_the_fileset(fileset, tmp_path):
    """runMCMC on plink_genotypes(bfile, keep=train) with outputEBV(model, train[:50] + candidates) against the run on the dense
    matrix of the same genotypes, decoded on the host with the training means: the EBV tables within 1e-4, the tolerance of
    test_gpu_packed.py between a packed and a dense chain; the 50 training IDs as in the default run."""
    import pandas as pd
    from jwas_jl_amd import api
    ids, train_rows = fileset["ids"], fileset["train_rows"]
    train = [ids[i] for i in train_rows]
    cand_rows = fileset["sets"][257]
    want = train[:50] + [ids[i] for i in cand_rows]
    G = fileset["G"]
    Xt = np.where(G[train_rows] == 9, 1.0, G[train_rows]).astype(np.float64)
    ph = pd.DataFrame({"ID": train, "y": (1.0 + Xt[:, 2] - Xt[:, 9] + np.random.default_rng(3).standard_normal(N_TRAIN)).astype(np.float32)})
    run = dict(chain_length=30, burnin=5, seed=11, block_size=64, gram_mode="mfma")      # (the block size plink_genotypes made resident)
    import jwas_jl_amd as J
    eng = J.HipEngine(0)
    try:
        b, M = _train(eng, fileset)
    finally:
        eng.close()
    outs = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for kind in ("list", "default"):
            geno = api.plink_genotypes(fileset["prefix"], keep=train, method="BayesC", Pi=0.9)
            try:
                model = api.build_model("y = intercept + geno", genotypes={"geno": geno})
                if kind == "list":
                    api.outputEBV(model, want)
                outs[kind] = api.runMCMC(model, ph, output_folder=str(tmp_path / kind), **run)
                assert kind == "default" or geno.device_backend.n_out == len(want)
            finally:
                geno.device_backend.close()
        # the dense matrix of the same genotypes: training and output individuals, Float32 code - training mean, missing codes 0
        all_rows = np.concatenate([train_rows, cand_rows])
        X = PKR.decode(PR.codes_of(M[all_rows][:, b["selected"]]), b["marker_means"], True)
        gdf = pd.DataFrame(np.asarray(X, dtype=np.float64), columns=b["markerID"])
        gdf.insert(0, "ID", [ids[i] for i in all_rows])
        dense = api.get_genotypes(gdf, method="BayesC", Pi=0.9, quality_control=False, center=False)
        dense.alleleFreq, dense.sum2pq, dense.centered = b["allele_freq"], b["sum2pq"], True
        model = api.build_model("y = intercept + geno", genotypes={"geno": dense})
        api.outputEBV(model, want)
        outs["dense"] = api.runMCMC(model, ph, output_folder=str(tmp_path / "dense"), **run)
    a, d, base = outs["list"]["EBV_y"], outs["dense"]["EBV_y"], outs["default"]["EBV_y"]
    assert [str(v) for v in a["ID"]] == want == [str(v) for v in d["ID"]]
    diff = np.abs(a["EBV"].to_numpy(dtype=np.float64) - d["EBV"].to_numpy(dtype=np.float64))
    print(f"packed against dense EBVs: worst difference {diff.max():.3e}")
    np.testing.assert_allclose(a["EBV"].to_numpy(dtype=np.float64), d["EBV"].to_numpy(dtype=np.float64), rtol=0, atol=1e-4)
    np.testing.assert_allclose(outs["list"]["marker effects geno"]["Estimate"], outs["dense"]["marker effects geno"]["Estimate"], atol=1e-4)
    assert [str(v) for v in base["ID"]] == train
    assert np.array_equal(a["EBV"].to_numpy()[:50], base["EBV"].to_numpy()[:50])
    assert np.array_equal(a["PEV"].to_numpy()[:50], base["PEV"].to_numpy()[:50])
    assert open(tmp_path / "list" / "IDs_for_individuals_with_genotypes.txt").read().split() == train
