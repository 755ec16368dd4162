"""PLINK 1 binary filesets into 2-bit packed device storage (csrc/plink.hpp, jwas_hip_plink_scan / _commit): the counts, the
committed payload and everything computed from it equal what the host path (prepare_streaming_genotypes(matrix) + load_jgb2)
gives for the same genotypes, bit for bit -- all individuals in file order (the dword path) and shuffled subsets (the gather
path), both counted alleles, ragged sizes."""
import contextlib
import io

import numpy as np
import pytest

import plink_reference as PR
from jwas_jl_amd import plink as P
from jwas_jl_amd import streaming as S
from test_plink_host import HAND_A1, HAND_A2, HAND_BED, assert_same_backend

pytestmark = pytest.mark.gpu

CASES = {"all-1037": (1037, None, 97), "subset-523": (1037, 523, 97), "three-of-70": (70, 3, 130), "shuffled-2300": (2300, 2300, 71)}


@pytest.fixture(scope="module")
def engines():
    import jwas_jl_amd as J
    a, b = J.HipEngine(0), J.HipEngine(0)
    yield a, b
    a.close(); b.close()


def _genotypes(n, p, seed):
    """A1 counts, 9 = missing: a monomorphic marker, one with 10 heterozygotes (allele frequency below 0.01 for n >= 523),
    about 2 % missing codes, one marker without any."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, p)
    G = (rng.random((n, p)) < f).astype(np.int64) + (rng.random((n, p)) < f).astype(np.int64)
    G[rng.random((n, p)) < 0.02] = 9
    G[:, 11] = 2
    G[:, 29] = 0
    G[rng.permutation(n)[:10], 29] = 1
    G[:, 30] = np.where(G[:, 30] == 9, 1, G[:, 30])
    return G


_cache = {}


def _case(name, tmp_path_factory):
    """The fileset of a case, its kept rows, and per counted allele the count matrix and the host-prepared backend (made once)."""
    if name not in _cache:
        n, nkeep, p = CASES[name]
        G = _genotypes(n, p, 100 + n + p)
        d = tmp_path_factory.mktemp(name)
        ids, mids, _, _ = PR.write_fileset(d / "g", G)
        rows = np.arange(n) if nkeep is None else np.random.default_rng(7).permutation(n)[:nkeep]
        keep = None if nkeep is None else [ids[i] for i in rows]
        per = {}
        for counted in ("A1", "A2"):
            M = (G if counted == "A1" else np.where(G == 9, 9, 2 - G))[rows]
            host = S.prepare_streaming_genotypes(M.astype(np.float64), d / f"host{counted}", obs_ids=[ids[i] for i in rows], marker_ids=mids)
            per[counted] = (M, host)
        _cache[name] = (str(d / "g"), n, p, rows, keep, per, d)
    return _cache[name]


@pytest.mark.parametrize("counted", ["A1", "A2"])
@pytest.mark.parametrize("name", list(CASES))
def test_scan_commit_equal_the_host_path(engines, tmp_path_factory, name, counted):
    dev, ref = engines
    bfile, n, p, rows, keep, per, d = _case(name, tmp_path_factory)
    M, host = per[counted]
    codes = PR.codes_of(M)
    # the counts, as exact integers
    counts = dev.plink_scan(bfile + ".bed", n, p, None if keep is None else rows, counted == "A1")
    assert counts.dtype == np.int64
    assert np.array_equal(counts, np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1))
    dev.plink_discard()
    # scan + quality control + commit
    b = P.load_plink(dev, bfile, keep=keep, counted_allele=counted)
    hb = S.load_streaming_backend(host)
    sel = b["selected"]
    assert 11 not in sel and 2 <= sel.size < p                                   # (the monomorphic marker)
    if len(rows) >= 523:
        assert 29 not in sel and 30 in sel                                       # (10 heterozygotes: below MAF; no missing code)
    assert (dev.n, dev.p) == (len(rows), sel.size) == (hb["nObs"], hb["nMarkers"])
    assert b["markerID"] == hb["markerID"] and b["obsID"] == hb["obsID"]
    info = dev.storage_info()
    assert info["kind"] == "packed2bit" and info["n"] == len(rows) and info["p"] == sel.size
    payload = dev.get_packed2bit(0, dev.p)
    assert np.array_equal(payload, S.pack_2bit(codes[:, sel]))                   # (pack_2bit pads with zeros)
    assert np.array_equal(dev.get_packed2bit(dev.p - 2, 2), payload[-2:])
    X = S.decode_markers(hb)
    assert np.array_equal(dev.get_columns(0, dev.p), X)
    # the host-prepared backend of the same genotypes on a second engine: x'x and the Grams
    ref.load_jgb2(host)
    assert np.array_equal(ref.get_packed2bit(0, ref.p), payload)                 # (any packed context, however it was loaded)
    for mode in ("f64", "mfma"):
        for e in (dev, ref):
            e.setup_blocks(64, mode)
        assert np.array_equal(dev.xpx(), ref.xpx())
        for i in range(ref.nblocks):
            assert np.array_equal(dev.gram(i), ref.gram(i))
    # three BayesC sweeps on 64-marker blocks
    rng = np.random.default_rng(3)
    y = (X[:, :2].sum(axis=1) + rng.standard_normal(dev.n)).astype(np.float32)
    y -= y.mean()
    for e in (dev, ref):
        e.init_state("BayesC")
        e.set_residual(y)
    kw = dict(vare=np.float32(0.5 * y.var() + 0.1), var_effect=np.float32(0.05), pi=0.7)
    for it in range(1, 4):
        for e in (dev, ref):
            e.sweep(iteration=it, seed=5, **kw)
    for got, want in zip(dev.get_state(), ref.get_state()):
        assert np.array_equal(got, want)
    assert len(rows) < 523 or np.any(dev.get_state()[0] != 0)
    assert np.array_equal(dev.get_residual(), ref.get_residual())
    # the backend written from the device
    out = S.prepare_streaming_genotypes(bfile + ".fam", d / f"dev{counted}", input_format="plink", engine=dev, keep=keep, counted_allele=counted)
    assert_same_backend(host, out)


def test_every_marker_kept_and_uncentered(engines, tmp_path_factory):
    """quality_control=False: no compaction, the staging buffer becomes the storage; center=False reaches the context."""
    dev, ref = engines
    bfile, n, p, rows, keep, per, d = _case("subset-523", tmp_path_factory)
    M, _ = per["A1"]
    b = P.load_plink(dev, bfile, keep=keep, quality_control=False, center=False)
    assert b["nMarkers"] == p == dev.p and np.array_equal(b["selected"], np.arange(p))
    assert np.array_equal(dev.get_packed2bit(0, p), S.pack_2bit(PR.codes_of(M)))
    host = S.prepare_streaming_genotypes(M.astype(np.float64), d / "noqc", quality_control=False, center=False)
    assert np.array_equal(dev.get_columns(0, p), S.decode_markers(S.load_streaming_backend(host)))


def test_gather_from_global_memory(engines, tmp_path):
    """A raw row of more than 60 KB (n_file > 245 760) does not fit the LDS staging of the gather: k_plink_transcode<kGatherGlobal>
    picks the kept individuals' fields out of global memory.  n_file = 245 800, five markers whose bytes are random (every byte
    is four valid fields), a shuffled subset of 300 individuals that holds the file's first and last one, both counted alleles:
    the counts and the committed payload against the per-individual reference reader."""
    dev, _ = engines
    n_file, p, nkeep = 245_800, 5, 300
    bpm = (n_file + 3) // 4
    assert -(-bpm // 16) * 16 > 60 << 10                                         # (kMaxLdsRow, csrc/plink.hpp)
    rng = np.random.default_rng(n_file)
    bed = tmp_path / "wide.bed"
    bed.write_bytes(PR.MAGIC + rng.integers(0, 256, size=(p, bpm), dtype=np.uint8).tobytes())
    inner = rng.permutation(n_file - 2)[:nkeep - 2] + 1
    rows = np.concatenate([[n_file - 1], inner[:100], [0], inner[100:]]).astype(np.int64)
    assert rows.size == nkeep == np.unique(rows).size
    for counted in ("A1", "A2"):
        codes = PR.codes_of(PR.read_bed(bed, n_file, p, counted)[rows])
        assert all((codes == c).any() for c in range(4))
        counts = dev.plink_scan(bed, n_file, p, rows, counted == "A1")
        assert np.array_equal(counts, np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1))
        dev.plink_commit(np.arange(p), np.ones(p, dtype=np.float32))
        assert (dev.n, dev.p) == (nkeep, p)
        assert np.array_equal(dev.get_packed2bit(0, p), PR.pack_codes(codes))


def test_hand_written_file(engines, tmp_path):
    dev, _ = engines
    (tmp_path / "hand.bed").write_bytes(HAND_BED)
    for a1, want in ((True, HAND_A1), (False, HAND_A2)):
        counts = dev.plink_scan(tmp_path / "hand.bed", 5, 2, None, a1)
        assert np.array_equal(counts, np.stack([(PR.codes_of(want) == c).sum(axis=0) for c in range(4)], axis=1))
        dev.plink_commit([0, 1], [0.0, 0.0])
        assert np.array_equal(S.unpack_2bit(dev.get_packed2bit(0, 2), 5), PR.codes_of(want))


def test_all_missing_marker(engines, tmp_path):
    import jwas_jl_amd as J
    dev, _ = engines
    G = _genotypes(70, 75, 9)
    G[:, 40] = 9
    PR.write_fileset(tmp_path / "m", G)
    counts = dev.plink_scan(tmp_path / "m.bed", 70, 75)
    assert counts[40].tolist() == [0, 0, 0, 70]
    with pytest.raises(ValueError, match=r"Marker snp41 has only missing values\."):
        P.load_plink(dev, tmp_path / "m")
    with pytest.raises(J.JwasHipError, match="jwas_hip_plink_scan has not been called") as ei:      # load_plink discarded its scan
        dev.plink_commit([0], [1.0])
    assert ei.value.code == -3


def test_errors(engines, tmp_path):
    import jwas_jl_amd as J
    dev, _ = engines
    G = _genotypes(70, 75, 10)
    PR.write_fileset(tmp_path / "e", G)
    raw = (tmp_path / "e.bed").read_bytes()
    bed = str(tmp_path / "e.bed")

    def refused(code, match, call):
        with pytest.raises(J.JwasHipError, match=match) as ei:
            call()
        assert ei.value.code == code

    (tmp_path / "magic.bed").write_bytes(b"\x6c\x1c\x01" + raw[3:])
    refused(-1, "not a PLINK 1 .bed file", lambda: dev.plink_scan(tmp_path / "magic.bed", 70, 75))
    (tmp_path / "mode.bed").write_bytes(b"\x6c\x1b\x00" + raw[3:])
    refused(-1, "mode byte 00", lambda: dev.plink_scan(tmp_path / "mode.bed", 70, 75))
    refused(-1, "individuals x 76 markers need", lambda: dev.plink_scan(bed, 70, 76))
    refused(-1, "is not found", lambda: dev.plink_scan(tmp_path / "nope.bed", 70, 75))
    refused(-1, r"rows\[1\] = 70 outside", lambda: dev.plink_scan(bed, 70, 75, [3, 70]))
    refused(-1, r"rows\[1\] = -1 outside", lambda: dev.plink_scan(bed, 70, 75, [3, -1]))
    refused(-1, r"rows\[2\] = 3 is listed twice", lambda: dev.plink_scan(bed, 70, 75, [3, 5, 3]))
    refused(-3, "jwas_hip_plink_scan has not been called", lambda: dev.plink_commit([0], [1.0]))
    dev.plink_scan(bed, 70, 75)
    refused(-1, "strictly ascending", lambda: dev.plink_commit([4, 2], [1.0, 1.0]))
    refused(-1, "strictly ascending", lambda: dev.plink_commit([2, 2], [1.0, 1.0]))
    refused(-1, "strictly ascending", lambda: dev.plink_commit([2, 75], [1.0, 1.0]))
    dev.plink_commit([2, 4], [1.0, 1.0])                                         # (the refused commits left the scan pending)
    assert (dev.n, dev.p) == (70, 2)
    refused(-1, "marker range", lambda: dev.get_packed2bit(1, 2))
    dev.plink_scan(bed, 70, 75)
    dev.load_dense(np.zeros((8, 3), dtype=np.float32))                           # any other load drops the scan
    refused(-3, "jwas_hip_plink_scan has not been called", lambda: dev.plink_commit([0], [1.0]))
    refused(-3, "no 2-bit packed genotypes", lambda: dev.get_packed2bit(0, 1))
    f64 = J.HipEngine(0, precision=64)
    try:
        for call in (lambda: f64.plink_scan(bed, 70, 75), lambda: f64.plink_discard(), lambda: f64.get_packed2bit(0, 1),
                     lambda: f64._chk(f64._L.jwas_hip_plink_commit(f64._h, None, 0, None, 1))):
            refused(-4, "not available in a Float64 context", call)
    finally:
        f64.close()


def test_runmcmc_on_a_fileset_equals_the_stream_backend(engines, tmp_path_factory, tmp_path):
    """runMCMC on plink_genotypes(bfile, keep=the phenotyped IDs in the phenotypes' order) and on the host-prepared backend of the
    same rows: identical tables."""
    import pandas as pd
    from jwas_jl_amd import api
    bfile, n, p, rows, keep, per, d = _case("subset-523", tmp_path_factory)
    M, host = per["A1"]
    rng = np.random.default_rng(21)
    X = S.decode_markers(S.load_streaming_backend(host))
    ph = pd.DataFrame({"ID": keep, "y": (1.0 + X[:, 2] - X[:, 9] + rng.standard_normal(len(keep))).astype(np.float32)})
    outs = []
    for kind in ("plink", "stream"):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = (api.plink_genotypes(bfile, keep=keep, method="BayesC", Pi=0.9) if kind == "plink"
                    else api.get_genotypes(host, method="BayesC", Pi=0.9, storage="stream"))
            model = api.build_model("y = intercept + geno")
            outs.append(api.runMCMC(model, ph, chain_length=30, burnin=5, seed=11, output_folder=str(tmp_path / kind)))
        if kind == "plink":
            assert geno.storage_mode == "device" and geno.obsID == keep and len(geno.counted_alleles) == geno.nMarkers
            geno.device_backend.close()
    a, b = outs
    assert sorted(a) == sorted(b) and "marker effects geno" in a and "EBV_y" in a
    tables = [key for key in a if isinstance(a[key], pd.DataFrame)]              # (the rest: the run's timings)
    assert len(tables) >= 3
    for key in tables:
        pd.testing.assert_frame_equal(a[key], b[key], check_exact=True)
    assert np.any(a["marker effects geno"]["Estimate"] != 0)
