"""The host side of the relationship matrix of 2-bit packed genotypes, without a GPU: api.genomic_relationship_matrix on PLINK
filesets, .jgb2 backends and resident Genotypes objects, on the stand-in engines of tests/grm_packed_reference.py (numpy grm_packed on
the decoded columns).  The GPU twin is tests/test_gpu_grm_packed.py."""
import contextlib
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

import gblup_reference as GR
import grm_packed_reference as PKR
import plink_reference as PR
from jwas_jl_amd import api, streaming

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _counts(n, p, seed, missing=0.0):
    """n x p copies of A1 (9 = missing); marker 3 is fixed and marker 7 has one copy: quality control drops both."""
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, 0.2 + 0.6 * rng.random(p), size=(n, p)).astype(np.int64)
    G[:, 3] = 0
    G[:, 7] = 0
    G[5, 7] = 1
    if missing:
        G[rng.random((n, p)) < missing] = 9
    return G


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    """The 64 x 200 fileset without missing values: (prefix, ids, markers, the same table as a DataFrame)."""
    G = _counts(64, 200, seed=5)
    prefix = str(tmp_path_factory.mktemp("grm") / "geno")
    ids, markers, _, _ = PR.write_fileset(prefix, G)
    table = pd.DataFrame(G.astype(np.float64), columns=markers)
    table.insert(0, "ID", ids)
    return prefix, ids, markers, table


def _k(frame):
    return frame.iloc[:, 1:].to_numpy()


# ---- the three binary inputs equal the text path -----------------------------------------------------------------------------------------
def test_fileset_stream_and_resident_object_equal_the_text_path(fileset, tmp_path):
    """With n = 64 every marker mean is k / 64, exact in Float32 whichever way it is summed: _impute_center_qc (the text path) and
    _marker_summaries (the scan's counts) select the same markers and give the same frequencies and centred values, so the matrices
    are equal bit for bit."""
    prefix, ids, markers, table = fileset
    text = _quiet(api.genomic_relationship_matrix, table, _engine=GR.GblupStandInEngine())
    eng = PKR.GrmPackedStandInEngine()
    plink = _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", _engine=eng)
    g, _, _, _, _ = _quiet(api._impute_center_qc, np.asfortranarray(_k(table).astype(np.float32)), list(markers), np.float32, True, 0.01, 9.0, True)
    assert eng.p == g.shape[1] == 198 and np.array_equal(eng.decoded(), g)        # the same selection and centred values
    assert eng.closes == 0                                                      # an injected engine is the caller's
    out = _quiet(streaming.prepare_streaming_genotypes, prefix, str(tmp_path / "backend"), input_format="plink", engine=PKR.GrmPackedStandInEngine())
    stream = _quiet(api.genomic_relationship_matrix, out, input_format="stream", _engine=PKR.GrmPackedStandInEngine())
    geno = _quiet(api.plink_genotypes, prefix, engine=PKR.GrmPackedStandInEngine())
    resident = _quiet(api.genomic_relationship_matrix, geno)
    for name, frame in (("plink", plink), ("stream", stream), ("resident", resident)):
        assert list(frame.columns) == ["ID"] + ids and list(frame["ID"]) == ids, name
        assert _k(frame).dtype == np.float32 and np.array_equal(_k(frame), _k(text)), name
    # ... and the .bed path of the fileset is as good as its prefix
    assert np.array_equal(_k(_quiet(api.genomic_relationship_matrix, prefix + ".bed", input_format="plink", _engine=PKR.GrmPackedStandInEngine())), _k(text))


def test_keep_order_quality_control_and_the_divisor(tmp_path):
    G = _counts(80, 60, seed=9, missing=0.03)
    prefix = str(tmp_path / "geno")
    ids, markers, _, _ = PR.write_fileset(prefix, G)
    keep = [ids[i] for i in np.random.default_rng(1).permutation(80)[:50]]
    eng = PKR.GrmPackedStandInEngine()
    seen, grm_packed = {}, eng.grm_packed

    def spy(divisor):
        seen["d"] = np.array(divisor)
        return grm_packed(divisor)
    eng.grm_packed = spy
    Kdf = _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", keep=keep, MAF=0.05, _engine=eng)
    assert list(Kdf["ID"]) == keep and list(Kdf.columns) == ["ID"] + keep
    # the rows are keep's; the markers are those the one copy of the quality control keeps on those rows
    rows = [ids.index(v) for v in keep]
    sub = G[rows]
    miss = sub == 9
    cnt, s1 = (~miss).sum(axis=0), np.where(miss, 0, sub).sum(axis=0).astype(np.float64)
    s2 = np.where(miss, 0, sub * sub).sum(axis=0).astype(np.float64)
    selected, mean, afreq, _ = streaming._marker_summaries(cnt, s1, s2, 50, True, 0.05, True, markers)
    assert eng.p == selected.size <= 58 and 3 not in selected and 7 not in selected
    assert np.array_equal(eng.means, mean)
    # the divisor: Float32 sqrt(2 p (1 - p)) of the backend's allele frequencies, the text path's expression
    assert seen["d"].dtype == np.float32
    assert np.array_equal(seen["d"], np.sqrt(np.float32(2.0) * afreq * (np.float32(1.0) - afreq)).astype(np.float32))
    assert np.array_equal(seen["d"], PKR.divisor_of(mean))
    codes = np.where(miss, 3, sub).astype(np.uint8)[:, selected]
    want = GR.grm_reference(PKR.decode(codes, mean, True), seen["d"])[0].astype(np.float32)
    assert np.array_equal(_k(Kdf), want)
    # quality_control=False keeps a fixed locus: the text path's error, and the scan is dropped with the engine left as it was
    with pytest.raises(ValueError, match=re.escape("needs 0 < p < 1 for every marker (a fixed locus has 2p(1-p) = 0); use quality_control=True")):
        _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", quality_control=False, _engine=PKR.GrmPackedStandInEngine())
    # id_column="FID_IID"
    K3 = _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", id_column="FID_IID", _engine=PKR.GrmPackedStandInEngine())
    assert list(K3["ID"]) == [f"fam{i % 7}_{v}" for i, v in enumerate(ids)]


def test_refusals(fileset, tmp_path):
    prefix, ids, markers, table = fileset

    def refuses(kind, words, file=prefix, **kw):
        eng = kw.pop("_engine", None) or PKR.GrmPackedStandInEngine()
        with pytest.raises(kind, match=re.escape(words)):
            _quiet(api.genomic_relationship_matrix, file, _engine=eng, **kw)
        assert getattr(eng, "loads", 0) == 0                          # refused before anything is loaded

    backend = _quiet(streaming.prepare_streaming_genotypes, prefix, str(tmp_path / "backend"), input_format="plink", engine=PKR.GrmPackedStandInEngine())
    geno = _quiet(api.plink_genotypes, prefix, engine=PKR.GrmPackedStandInEngine())
    for fmt, file in (("plink", prefix), ("stream", backend), ("text", geno)):
        what = "a Genotypes object" if fmt == "text" else f'input_format="{fmt}"'
        refuses(ValueError, f"double_precision=True is not available with {what}: 2-bit packed storage has no Float64 path", file=file,
                input_format=fmt, double_precision=True)
        for name, value in (("separator", ","), ("header", True), ("missing_value", 9.0)):          # given, even with the text default
            refuses(ValueError, f"{name}= describes a text table; it is not an argument of {what}", file=file, input_format=fmt, **{name: value})
    refuses(ValueError, 'input_format must be "text", "plink" or "stream".', input_format="bed")
    refuses(ValueError, 'keep= belongs to input_format="plink"', file=backend, input_format="stream", keep=ids[:5])
    refuses(ValueError, 'keep= belongs to input_format="plink"', file=table, keep=ids[:5], _engine=GR.GblupStandInEngine())
    refuses(ValueError, 'input_format="plink" requires the prefix of a .bed/.bim/.fam fileset.', file=table, input_format="plink")
    refuses(NotImplementedError, "genomic_relationship_matrix needs an engine with grm_packed; the package has no CPU fallback", input_format="plink",
            _engine=PR.PlinkStandInEngine())
    refuses(NotImplementedError, "genomic_relationship_matrix needs an engine with grm_packed; the package has no CPU fallback", file=backend,
            input_format="stream", _engine=GR.GblupStandInEngine())
    with pytest.raises(FileNotFoundError):
        _quiet(api.genomic_relationship_matrix, str(tmp_path / "absent"), input_format="plink", _engine=PKR.GrmPackedStandInEngine())
    with pytest.raises(ValueError, match="counted_allele"):
        _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", counted_allele="B", _engine=PKR.GrmPackedStandInEngine())
    # a storage="stream" Genotypes object has no resident engine
    with pytest.raises(ValueError, match="resident on an engine"):
        _quiet(api.genomic_relationship_matrix, _quiet(api.get_genotypes, backend, method="BayesC", storage="stream"))
    # the text path is what it was: the same defaults, the same refusal of an engine without grm
    assert np.array_equal(_k(_quiet(api.genomic_relationship_matrix, table, _engine=GR.GblupStandInEngine())),
                          _k(_quiet(api.genomic_relationship_matrix, table, separator=",", header=True, missing_value=9.0, input_format="text",
                                    _engine=GR.GblupStandInEngine())))
    with pytest.raises(NotImplementedError, match="needs an engine with grm; the package has no CPU fallback"):
        _quiet(api.genomic_relationship_matrix, table, _engine=object())


def test_a_genotypes_object_keeps_its_engine(fileset):
    prefix, ids, markers, table = fileset
    eng = PKR.GrmPackedStandInEngine()
    geno = _quiet(api.plink_genotypes, prefix, engine=eng)
    loads, payload = eng.loads, eng.get_packed2bit(0, eng.p)
    K1 = _quiet(api.genomic_relationship_matrix, geno)
    K2 = _quiet(api.genomic_relationship_matrix, geno, input_format="plink")       # (the object says what it is; the format is not consulted)
    assert eng.loads == loads == 1 and eng.closes == 0
    assert np.array_equal(eng.get_packed2bit(0, eng.p), payload)
    assert geno.device_backend is eng and geno.storage_mode == "device"
    assert list(K1["ID"]) == ids and np.array_equal(_k(K1), _k(K2))
    # an engine that holds a dense matrix: grm, not grm_packed
    dense = PKR.DenseResidentStandIn()
    X = eng.decoded()
    dense.load_dense(X)
    gd = api.device_genotypes(dense, obsID=ids, centered=True, alleleFreq=geno.alleleFreq, sum2pq=geno.sum2pq)
    Kd = _quiet(api.genomic_relationship_matrix, gd)
    assert dense.loads == 1 and dense.closes == 0
    assert np.array_equal(_k(Kd), _k(K1))
    # a resident engine that cannot form the matrix
    bare = PR.PlinkStandInEngine()
    bare.storage_info = lambda: {"kind": "packed2bit"}
    geno.device_backend = bare
    with pytest.raises(NotImplementedError, match=re.escape("needs an engine with grm_packed; the package has no CPU fallback")):
        api.genomic_relationship_matrix(geno)


def test_the_result_goes_into_a_gblup_run(fileset, tmp_path):
    prefix, ids, markers, table = fileset
    Kdf = _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", _engine=PKR.GrmPackedStandInEngine())
    geno = _quiet(api.get_genotypes, Kdf, 1.0, method="GBLUP")
    model = api.build_model("y1 = intercept + geno", genotypes={"geno": geno})
    ph = pd.DataFrame({"ID": ids, "y1": 1.0 + np.random.default_rng(2).standard_normal(len(ids))})
    out = _quiet(api.runMCMC, model, ph, chain_length=20, seed=3, output_folder=str(tmp_path / "run"), _engine=GR.GblupStandInEngine(), gblup_eigen="host")
    ebv = out["EBV_y1"]
    assert sorted(str(v) for v in ebv["ID"]) == sorted(ids) and np.isfinite(ebv["EBV"].to_numpy(dtype=np.float64)).all()


# ---- the entry point is named where it has to be -------------------------------------------------------------------------------------------
def test_header_bindings_and_documents_name_the_entry_point():
    from jwas_jl_amd import _lib
    from jwas_jl_amd.engine import HipEngine

    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as fh:
            return fh.read()

    header = text("include", "jwas_hip.h")
    assert re.search(r"int\s+jwas_hip_grm_packed2bit\(jwas_hip_ctx\* ctx, const float\* divisor_p, float\* K_host\);", header)
    comment = header[:header.index("jwas_hip_grm_packed2bit(jwas_hip_ctx")].rsplit("/*", 1)[1]
    assert "readgenotypes.jl:403-408" in comment
    assert header.index("int  jwas_hip_grm(") < header.index("jwas_hip_grm_packed2bit(jwas_hip_ctx") < header.index("jwas_hip_grm_estimate_bytes(")
    assert '"jwas_hip_grm_packed2bit"' in text("jwas.jl_amd", "_lib.py")
    assert ":jwas_hip_grm_packed2bit" in text("julia", "JWASHip.jl")
    assert "jwas_hip_grm_packed2bit" in text("INTEGRATION.md")
    assert callable(getattr(HipEngine, "grm_packed", None))
    assert _lib.GRM_CHUNK == 64
