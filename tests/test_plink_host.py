"""PLINK 1 binary filesets, host side: the format helpers of plink_reference, read_fam / read_bim, the keep= and quality-control
errors of plink.load_plink, and prepare_streaming_genotypes(input_format="plink") on a numpy stand-in for the engine: it writes
the files prepare_streaming_genotypes(matrix) writes for the same genotypes, byte for byte."""
import numpy as np
import pytest

import plink_reference as PR
from jwas_jl_amd import plink as P
from jwas_jl_amd import streaming as S

# 2 markers x 5 individuals, spelled out.  Marker 1: fields 0 1 2 3 | 2 -> bytes 0b11_10_01_00, 0b00_00_00_10; marker 2: fields 3 3 0 2 | 1.
HAND_BED = bytes([0x6C, 0x1B, 0x01, 0xE4, 0x02, 0x8F, 0x01])
HAND_A1 = np.array([[2, 0], [9, 0], [1, 2], [0, 1], [1, 9]])        # copies of A1, 9 = missing
HAND_A2 = np.array([[0, 2], [9, 2], [1, 0], [2, 1], [1, 9]])

BACKEND_FILES = (".jgb2", ".mean.f32", ".xpRinvx.f32", ".afreq.f32", ".selected.i32", ".obsid.txt", ".markerid.txt")


def _genotypes(n, p, seed, missing=0.03):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, p)
    G = (rng.random((n, p)) < f).astype(np.int64) + (rng.random((n, p)) < f).astype(np.int64)
    G[:, 3] = 2                                            # monomorphic: removed by quality control
    G[:, 7] = 0
    G[:5, 7] = 1                                           # allele frequency 5 / (2 n): below MAF for n > 250
    G[rng.random((n, p)) < missing] = 9
    return G


def _meta(prefix):
    out = {}
    for line in open(prefix + ".meta"):
        k, v = line.rstrip("\n").split("\t", 1)
        if not k.endswith("_path"):
            out[k] = v
    return out


def assert_same_backend(a, b):
    for ext in BACKEND_FILES:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert _meta(a) == _meta(b)


def test_hand_written_file(tmp_path):
    path = tmp_path / "hand.bed"
    path.write_bytes(HAND_BED)
    assert np.array_equal(PR.read_bed(path, 5, 2, "A1"), HAND_A1)
    assert np.array_equal(PR.read_bed(path, 5, 2, "A2"), HAND_A2)
    assert PR.bed_bytes(HAND_A1) == HAND_BED
    eng = PR.PlinkStandInEngine()
    counts = eng.plink_scan(path, 5, 2, None, True)
    assert counts.tolist() == [[1, 2, 1, 1], [2, 1, 1, 1]]
    counts = eng.plink_scan(path, 5, 2, [4, 0], False)
    assert counts.tolist() == [[1, 1, 0, 0], [0, 0, 1, 1]]
    eng.plink_commit([0, 1], [1.0, 2.0])
    assert eng.get_packed2bit(0, 2).tolist() == [[0b0001], [0b1011]]


@pytest.mark.parametrize("n,p", [(5, 3), (8, 1), (37, 23), (130, 9)])
def test_writer_reader_round_trip(tmp_path, n, p):
    G = _genotypes(n, max(p, 8), n)[:, :p]
    PR.write_fileset(tmp_path / "rt", G)
    assert (tmp_path / "rt.bed").stat().st_size == 3 + p * ((n + 3) // 4)
    assert np.array_equal(PR.read_bed(tmp_path / "rt.bed", n, p), G)
    A2 = np.where(G == 9, 9, 2 - G)
    assert np.array_equal(PR.read_bed(tmp_path / "rt.bed", n, p, "A2"), A2)
    assert np.array_equal(PR.pack_codes(PR.codes_of(G)), S.pack_2bit(PR.codes_of(G)))
    with pytest.raises(ValueError, match="size"):
        PR.read_bed(tmp_path / "rt.bed", n + 4, p)


def test_read_fam_and_bim(tmp_path):
    G = _genotypes(6, 9, 1)
    ids, mids, a1, a2 = PR.write_fileset(tmp_path / "f", G, fids=["A", "A", "B", "B", "C", "C"])
    assert P.read_fam(tmp_path / "f.fam") == ids == [f"id{i + 1}" for i in range(6)]
    assert P.read_fam(tmp_path / "f.fam", "FID_IID")[:3] == ["A_id1", "A_id2", "B_id3"]
    with pytest.raises(ValueError, match="id_column"):
        P.read_fam(tmp_path / "f.fam", "FID")
    assert P.read_bim(tmp_path / "f.bim") == (mids, a1, a2)
    (tmp_path / "bad.fam").write_text("A id1 0 0\n")
    with pytest.raises(ValueError, match="line 1 has 4 fields"):
        P.read_fam(tmp_path / "bad.fam")
    for path in ("f", "f.bed", "f.bim", "f.fam"):
        assert P.resolve_bfile(str(tmp_path / path)) == str(tmp_path / "f")


def test_keep_errors_and_incomplete_fileset(tmp_path):
    G = _genotypes(12, 9, 2)
    PR.write_fileset(tmp_path / "k", G)
    eng = PR.PlinkStandInEngine()
    with pytest.raises(ValueError, match="individual nobody is not in the .fam file"):
        P.load_plink(eng, tmp_path / "k", keep=["id1", "nobody"])
    with pytest.raises(ValueError, match="individual id3 is listed twice"):
        P.load_plink(eng, tmp_path / "k", keep=["id3", "id1", "id3"])
    with pytest.raises(ValueError, match="no individual"):
        P.load_plink(eng, tmp_path / "k", keep=[])
    with pytest.raises(ValueError, match="counted_allele"):
        P.load_plink(eng, tmp_path / "k", counted_allele="minor")
    (tmp_path / "k.bim").unlink()
    with pytest.raises(FileNotFoundError, match="k.bim"):
        P.load_plink(eng, tmp_path / "k")
    PR.write_fileset(tmp_path / "dup", G, obs_ids=["a"] * 2 + [f"b{i}" for i in range(10)])
    with pytest.raises(ValueError, match="individual a is listed twice in the .fam"):
        P.load_plink(eng, tmp_path / "dup", keep=["b1"])
    assert P.load_plink(eng, tmp_path / "dup", quality_control=False)["obsID"][:3] == ["a", "a", "b0"]      # (no keep: file order, as it is)


def test_quality_control_messages_and_discard(tmp_path):
    G = _genotypes(40, 9, 3)
    G[:, 4] = 9
    PR.write_fileset(tmp_path / "q", G)
    eng = PR.PlinkStandInEngine()
    with pytest.raises(ValueError, match=r"Marker snp5 has only missing values\."):
        P.load_plink(eng, tmp_path / "q")
    assert eng.discards == 1 and eng._pending is None
    G[:, :] = 1
    PR.write_fileset(tmp_path / "q2", G)
    with pytest.raises(ValueError, match=r"No markers remain after streaming genotype quality control\."):
        P.load_plink(eng, tmp_path / "q2")
    assert eng.discards == 2
    b = P.load_plink(eng, tmp_path / "q2", quality_control=False, center=False)
    assert b["nMarkers"] == 9 and b["centered"] is False and eng.discards == 2 and (eng.n, eng.p) == (40, 9)


def test_input_format_validation(tmp_path):
    G = _genotypes(12, 9, 4)
    PR.write_fileset(tmp_path / "v", G)
    with pytest.raises(ValueError, match="input_format"):
        S.prepare_streaming_genotypes(str(tmp_path / "v"), tmp_path / "o", input_format="pgen")
    with pytest.raises(ValueError, match="fileset"):
        S.prepare_streaming_genotypes(G, tmp_path / "o", input_format="plink")
    with pytest.raises(ValueError, match='input_format="plink"'):
        S.prepare_streaming_genotypes(G, tmp_path / "o", keep=["id1"])
    with pytest.raises(ValueError, match='input_format="plink"'):
        S.prepare_streaming_genotypes(G, tmp_path / "o", engine=PR.PlinkStandInEngine())
    assert S.prepare_streaming_genotypes(G.astype(float), tmp_path / "o", input_format="text") == str(tmp_path / "o")


@pytest.mark.parametrize("n,p,nkeep,counted,center,qc", [(301, 40, None, "A1", True, True), (301, 40, 120, "A2", True, True),
                                                        (37, 23, 9, "A1", False, True), (50, 12, None, "A2", True, False)])
def test_plink_backend_equals_the_matrix_backend(tmp_path, n, p, nkeep, counted, center, qc):
    G = _genotypes(n, p, 5 + n)
    ids, mids, a1, a2 = PR.write_fileset(tmp_path / "g", G)
    rows = np.arange(n) if nkeep is None else np.random.default_rng(1).permutation(n)[:nkeep]
    keep = None if nkeep is None else [ids[i] for i in rows]
    M = G if counted == "A1" else np.where(G == 9, 9, 2 - G)
    host = S.prepare_streaming_genotypes(M[rows].astype(np.float64), tmp_path / "host", obs_ids=[ids[i] for i in rows], marker_ids=mids,
                                         quality_control=qc, center=center)
    eng = PR.PlinkStandInEngine()
    dev = S.prepare_streaming_genotypes(str(tmp_path / "g.bed"), tmp_path / "dev", input_format="plink", engine=eng, keep=keep,
                                        counted_allele=counted, quality_control=qc, center=center)
    assert dev == str(tmp_path / "dev")
    assert_same_backend(host, dev)
    b = S.load_streaming_backend(dev)
    if qc:
        assert "snp4" not in b["markerID"]                                       # the monomorphic marker
    if qc and n > 250 and nkeep is None:
        assert "snp8" not in b["markerID"]                                       # five heterozygotes among all 301: below MAF
    assert np.array_equal(eng.means, b["marker_means"]) and eng.centered == center
    got = P.load_plink(eng, tmp_path / "g", keep=keep, counted_allele=counted, quality_control=qc, center=center)
    for key in ("nObs", "nMarkers", "stride_bytes", "nMarkersAll", "centered", "sum2pq", "obsID", "markerID"):
        assert got[key] == b[key], key
    for key in ("marker_means", "xpRinvx", "allele_freq"):
        assert np.array_equal(got[key], b[key]), key
    assert np.array_equal(got["selected"] + 1, np.fromfile(dev + ".selected.i32", dtype="<i4"))
    assert got["counted_alleles"] == [(a1 if counted == "A1" else a2)[j] for j in got["selected"]]
