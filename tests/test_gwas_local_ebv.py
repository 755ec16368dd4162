"""GWAS(..., local_EBV=true) (src/3.GWAS/src/GWAS.jl:149-173): the host logic over a numpy stand-in for the device's GWAS
session (tests/gwas_session_standin.py), against the literal restatement of the reference's loop.

Tolerance for the local EBVs (derived, not measured): |value - numpy64| <= (K_w + 4 S) 2^-52 A_iw, see
gwas_session_standin.local_ebv_bound."""
import os

import numpy as np
import pandas as pd
import pytest

from jwas_jl_amd import api, samples as S
from jwas_jl_amd.gwas import GWAS, build_windows
from gwas_session_standin import SessionOracleEngine, literal_local_ebv, local_ebv_bound
from oracle_engine import OracleEngine
from test_gwas import _case

DEMO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_7animals")


def _read_local(path):
    tab = pd.read_csv(path, dtype={"ID": str})
    return tab, tab.iloc[:, 1:].to_numpy(dtype=np.float64)


@pytest.mark.parametrize("sliding", [False, True])
def test_local_ebv_matches_literal_restatement(tmp_path, sliding):
    X, samples, f, mapf, chrom, pos = _case(tmp_path, seed=3)
    GWAS(X, mapf, f, window_size="1 Mb", sliding_window=sliding, threshold=0.05, local_EBV=True, output_folder=str(tmp_path),
         _engine=SessionOracleEngine("dense"))
    win = build_windows(chrom, pos, 1_000_000, sliding)
    nwin = len(win["nsnp"])
    tab, got = _read_local(tmp_path / "localEBV1.txt")
    assert list(tab.columns) == ["ID"] + [f"w{w}" for w in range(1, nwin + 1)]
    assert list(tab["ID"]) == [str(i) for i in range(1, X.shape[0] + 1)]          # a bare genotype array: 1...n
    want = literal_local_ebv(X, samples, win["col_start"], win["col_end"])
    bound = local_ebv_bound(X, samples, win["col_start"], win["col_end"])
    err = np.abs(got - want)
    print("max |err| / bound:", float((err / np.where(bound > 0, bound, 1)).max()))
    assert got.shape == want.shape and (err <= bound).all()
    assert np.abs(want).max() > 0.01                                             # (not a comparison of zeros)


@pytest.mark.parametrize("sliding", [False, True])
def test_flag_changes_nothing_else(tmp_path, sliding):
    X, samples, f, mapf, _, _ = _case(tmp_path, seed=4)
    a, b = tmp_path / "off", tmp_path / "on"
    a.mkdir(); b.mkdir()
    kw = dict(window_size="1 Mb", sliding_window=sliding, threshold=0.05, output_winVarProps=True)
    r0, p0 = GWAS(X, mapf, f, output_folder=str(a), _engine=SessionOracleEngine("dense"), **kw)
    r1, p1 = GWAS(X, mapf, f, local_EBV=True, output_folder=str(b), _engine=SessionOracleEngine("dense"), **kw)
    pd.testing.assert_frame_equal(r0[0], r1[0], check_exact=True)
    assert np.array_equal(p0[0], p1[0])
    for name in sorted(os.listdir(a)):
        assert open(a / name, "rb").read() == open(b / name, "rb").read(), name
    assert sorted(set(os.listdir(b)) - set(os.listdir(a))) == ["localEBV1.txt"]
    assert any(n.startswith("GWAS_") for n in os.listdir(a)) and "MCMC_samples_local_genomic_variance1.txt" in os.listdir(a)


def test_two_files_are_independent(tmp_path):
    X, s1, f1, mapf, chrom, pos = _case(tmp_path, seed=5)
    rng = np.random.default_rng(11)
    s2 = np.where(rng.random((17, s1.shape[1])) < 0.3, rng.standard_normal((17, s1.shape[1])), 0.0).astype(np.float32)
    f2 = str(tmp_path / "MCMC_samples_marker_effects_geno_y2.txt")
    pd.DataFrame(s2, columns=[f"m{j + 1}" for j in range(s1.shape[1])]).to_csv(f2, index=False, float_format="%.9g")
    eng = SessionOracleEngine("dense")
    res = GWAS(X, mapf, f1, f2, window_size="1 Mb", local_EBV=True, output_folder=str(tmp_path), _engine=eng)
    assert len(res) == 2 and eng.begun == 2 and eng.ended == 2
    win = build_windows(chrom, pos, 1_000_000, False)
    for k, s in ((1, s1), (2, s2)):
        _, got = _read_local(tmp_path / f"localEBV{k}.txt")
        want = literal_local_ebv(X, s, win["col_start"], win["col_end"])
        assert (np.abs(got - want) <= local_ebv_bound(X, s, win["col_start"], win["col_end"])).all(), k


def test_binary_samples_go_in_record_by_record(tmp_path, monkeypatch):
    X, samples, f, mapf, chrom, pos = _case(tmp_path, seed=6)
    fbin = str(tmp_path / "MCMC_samples_marker_effects_geno_y1.bin")
    wr = S.MarkerSampleWriter(fbin, [f"m{j + 1}" for j in range(X.shape[1])])
    for a in samples:
        nz = np.flatnonzero(a)
        wr.append(nz, a[nz])
    wr.close()
    ftxt = S.to_text(fbin, str(tmp_path / "converted.txt"))
    d1, d2 = tmp_path / "bin", tmp_path / "txt"
    d1.mkdir(); d2.mkdir()
    GWAS(X, mapf, ftxt, local_EBV=True, output_folder=str(d2), _engine=SessionOracleEngine("dense"))

    def boom(path):
        raise AssertionError("read_dense builds a samples x p matrix; local_EBV=true must not reach it")
    monkeypatch.setattr(S, "read_dense", boom)
    GWAS(X, mapf, fbin, local_EBV=True, output_folder=str(d1), _engine=SessionOracleEngine("dense"))
    assert open(d1 / "localEBV1.txt", "rb").read() == open(d2 / "localEBV1.txt", "rb").read()
    assert open(d1 / "MCMC_samples_local_genomic_variance1.txt", "rb").read() == open(d2 / "MCMC_samples_local_genomic_variance1.txt", "rb").read()
    win = build_windows(chrom, pos, 1_000_000, False)
    _, got = _read_local(d1 / "localEBV1.txt")
    want = literal_local_ebv(X, samples, win["col_start"], win["col_end"])
    assert (np.abs(got - want) <= local_ebv_bound(X, samples, win["col_start"], win["col_end"])).all()


def test_ids_of_a_model_are_the_output_individuals(tmp_path):
    pheno = pd.read_csv(os.path.join(DEMO, "phenotypes.txt"), na_values=["NA"], dtype={"ID": str})
    geno = api.get_genotypes(os.path.join(DEMO, "genotypes.txt"), 1.0, separator=",", method="BayesC")
    model = api.build_model("y1 = intercept + geno", 1.0)
    want_ids = [geno.obsID[i] for i in (4, 0, 2)]
    api.outputEBV(model, want_ids)
    folder = tmp_path / "chain"
    api.runMCMC(model, pheno, chain_length=40, burnin=10, output_samples_frequency=10, outputEBV=True, output_folder=str(folder), seed=5,
                _engine=OracleEngine("block"), block_size=64)
    Mi = model.M[0]
    marker_file = str(folder / "MCMC_samples_marker_effects_geno_y1.txt")
    api.GWAS(model, os.path.join(DEMO, "map.txt"), marker_file, window_size="1 Mb", local_EBV=True, output_folder=str(tmp_path),
             _engine=SessionOracleEngine("dense"))
    tab, got = _read_local(tmp_path / "localEBV1.txt")
    assert list(tab["ID"]) == [Mi.obsID[r] for r in Mi.output_rows] == want_ids
    assert list(tab.columns) == ["ID", "w1", "w2", "w3"]
    smp = pd.read_csv(marker_file).to_numpy(dtype=np.float32)
    Xo = Mi.genotypes[Mi.output_rows, :]
    mp = pd.read_csv(os.path.join(DEMO, "map.txt"), dtype={0: str, 1: str})
    win = build_windows(mp.iloc[:, 1].to_numpy(), mp.iloc[:, 2].to_numpy(dtype=np.int64), 1_000_000, False)
    cs, ce = win["col_start"], win["col_end"]
    assert list(win["nsnp"]) == [2, 1, 2]                  # map.txt: chr 1 [0, 1 Mb), [1, 2 Mb); chr 2 [0, 1 Mb)
    want = literal_local_ebv(Xo, smp, cs, ce)
    assert (np.abs(got - want) <= local_ebv_bound(Xo, smp, cs, ce)).all()


def test_memory_guard_and_estimate(tmp_path):
    X, samples, f, mapf, _, _ = _case(tmp_path, seed=7)
    eng = SessionOracleEngine("dense")
    eng.hbm_free = 20_000
    with pytest.raises(MemoryError, match=r"60 x \d+ x 8"):
        GWAS(X, mapf, f, local_EBV=True, output_folder=str(tmp_path), _engine=eng)
    assert getattr(eng, "begun", 0) == 0 and not os.path.exists(tmp_path / "localEBV1.txt")
    # the library's pure function (no GPU needed, like estimate_bytes): the accumulator is 8 x padded rows x windows
    from jwas_jl_amd import HipEngine
    for n, nwin, nnz in ((700, 40, 3000), (50_000, 6_000, 600_000), (256, 1, 0)):
        ld = (n + 255) // 256 * 256
        off, on = HipEngine.gwas_estimate_bytes(n, nwin, nnz, False), HipEngine.gwas_estimate_bytes(n, nwin, nnz, True)
        assert off > 0 and on - off == 8 * ld * nwin
        assert on == SessionOracleEngine.gwas_estimate_bytes(n, nwin, nnz, True)


def test_engine_without_session_and_gwas_false(tmp_path):
    X, samples, f, mapf, _, _ = _case(tmp_path, seed=8)
    with pytest.raises(TypeError, match="gwas_begin"):
        GWAS(X, mapf, f, local_EBV=True, output_folder=str(tmp_path), _engine=OracleEngine("dense"))
    assert GWAS(X, mapf, f, GWAS=False, local_EBV=True, output_folder=str(tmp_path), _engine=SessionOracleEngine("dense")) == ()
    assert not [n for n in os.listdir(tmp_path) if n.startswith("localEBV")]
