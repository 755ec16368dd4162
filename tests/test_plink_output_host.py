"""EBVs for individuals of a PLINK fileset outside the training set, host side: plink.load_plink_output against the numpy reader of
plink_reference.py on a stand-in engine, the handling of the caller's ID list, and the routing of outputEBV(model, IDs) in run_chain --
a whole runMCMC on a stand-in whose sweep is the CPU oracle's (plink_output_reference.PlinkOutputChainEngine)."""
import contextlib
import io

import numpy as np
import pandas as pd
import pytest

import plink_output_reference as POR
import plink_reference as PR
from jwas_jl_amd import api
from jwas_jl_amd import plink as P

N_FILE, P_FILE, N_TRAIN = 1003, 100, 301
REFUSAL = "storage=:stream reports EBVs for the genotyped individuals in file order (outputEBV(model, IDs) lists stay on the reference)"


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


def _genotypes(n, p, seed):
    """A1 counts, 9 = missing; about 2 % missing.  Markers 3, 13, ... 93 are monomorphic: ten of a hundred fail the quality control of
    any training subset."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.5, p)
    G = (rng.random((n, p)) < f).astype(np.int64) + (rng.random((n, p)) < f).astype(np.int64)
    G[rng.random((n, p)) < 0.02] = 9
    G[:, 3::10] = 2
    return G


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("plink_output")
    G = _genotypes(N_FILE, P_FILE, 41)
    ids, mids, _, _ = PR.write_fileset(d / "g", G)
    train_rows = np.random.default_rng(5).permutation(N_FILE)[:N_TRAIN]
    return str(d / "g"), G, ids, train_rows


def _output_sets(ids):
    rng = np.random.default_rng(9)
    sets = {k: rng.permutation(N_FILE)[:k] for k in (1, 5, 257, 700)}
    sets["all"] = np.arange(N_FILE)
    return sets


@pytest.mark.parametrize("counted", ["A1", "A2"])
def test_load_plink_output_equals_the_reader(fileset, counted):
    prefix, G, ids, train_rows = fileset
    eng = POR.PlinkOutputStandInEngine()
    b = _quiet(P.load_plink, eng, prefix, keep=[ids[i] for i in train_rows], counted_allele=counted)
    src, sel = b["source"], b["selected"]
    assert 85 <= sel.size <= 90 and not set(range(3, 100, 10)) & set(sel.tolist())
    assert (src.prefix, src.id_column, src.counted_allele, src.fam_ids, src.p_file) == (prefix, "IID", counted, ids, P_FILE)
    assert np.array_equal(src.selected, sel)
    training = eng.get_packed2bit(0, eng.p)
    M = PR.read_bed(prefix + ".bed", N_FILE, P_FILE, counted)
    for name, rows in _output_sets(ids).items():
        n_out = P.load_plink_output(eng, src, [ids[i] for i in rows])
        assert n_out == rows.size == eng.n_out
        got = eng.get_output_packed2bit(0, eng.p)
        want = PR.pack_codes(PR.codes_of(M[rows][:, sel]))                          # exactly the training selection; pad fields 0
        assert got.shape == (sel.size, (rows.size + 3) // 4) and np.array_equal(got, want), name
        assert eng._pending is None                                                  # the scan is consumed
    assert np.array_equal(eng.get_packed2bit(0, eng.p), training) and eng.n == N_TRAIN      # the training storage is untouched


def test_id_handling(fileset, tmp_path):
    prefix, G, ids, train_rows = fileset
    eng = POR.PlinkOutputStandInEngine()
    src = _quiet(P.load_plink, eng, prefix, keep=[ids[i] for i in train_rows])["source"]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        kept = P.resolve_plink_output_ids(src, [ids[7], "nobody", ids[2]])
    assert kept == [ids[7], ids[2]] and "Only output EBV for tesing individuals with genotypes." in out.getvalue()
    with pytest.raises(ValueError, match="listed twice"):
        P.load_plink_output(eng, src, [ids[1], ids[4], ids[1]])
    with pytest.raises(ValueError, match="is not in the .fam file"):
        P.load_plink_output(eng, src, [ids[1], "nobody"])
    with pytest.raises(ValueError, match="no individual is listed"):
        P.load_plink_output(eng, src, [])
    assert eng.output_loads == 0 and eng._pending is None


def test_memory_guard_names_both_figures(fileset):
    prefix, G, ids, train_rows = fileset
    eng = POR.PlinkOutputStandInEngine()
    src = _quiet(P.load_plink, eng, prefix, keep=[ids[i] for i in train_rows])["source"]
    eng.device_info = lambda: {"hbm_free": 40_000}
    sb = 768 // 4                                                                    # 700 individuals: ld_out = 768
    with pytest.raises(MemoryError) as err:
        P.load_plink_output(eng, src, ids[:700])
    assert f"{sb * P_FILE / 1e9:.2f} GB" in str(err.value) and f"{sb * eng.p / 1e9:.2f} GB" in str(err.value) and "staging" in str(err.value)
    assert eng.output_loads == 0 and eng._pending is None
    assert _quiet(P.load_plink_output, eng, src, ids[:700], memory_guard="warn") == 700
    assert P.load_plink_output(eng, src, ids[:5]) == 5                               # 64 x (100 + p) bytes fit


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def _phenotypes(G, ids, train_rows):
    rng = np.random.default_rng(3)
    X = np.where(G[train_rows] == 9, 1.0, G[train_rows]).astype(np.float64)
    return pd.DataFrame({"ID": [ids[i] for i in train_rows], "y": (1.0 + X[:, 2] - X[:, 9] + rng.standard_normal(N_TRAIN)).astype(np.float32)})


def _run(geno, ph, out_ids, folder, **kw):
    model = api.build_model("y = intercept + geno", genotypes={"geno": geno})
    if out_ids is not None:
        api.outputEBV(model, out_ids)
    return _quiet(api.runMCMC, model, ph, chain_length=12, burnin=2, seed=7, output_folder=str(folder), **kw)


def test_outputebv_list_on_a_plink_genotypes_object(fileset, tmp_path):
    """The whole runMCMC on the stand-in: the EBV table lists the caller's IDs in the caller's order, unknown IDs dropped; the rows
    are loaded once; every saved sample goes through ebv_output; the ID file stays the training set's."""
    prefix, G, ids, train_rows = fileset
    train = [ids[i] for i in train_rows]
    ph = _phenotypes(G, ids, train_rows)
    candidates = [i for i in ids if i not in set(train)][:40][::-1]
    want = train[:10] + ["nobody"] + candidates
    eng = POR.PlinkOutputChainEngine()
    geno = _quiet(api.plink_genotypes, prefix, keep=train, engine=eng, method="BayesC", Pi=0.9)
    assert geno.plink_source.fam_ids == ids and geno.plink_source.counted_allele == "A1"
    out = _run(geno, ph, want, tmp_path / "list")
    ebv = out["EBV_y"]
    assert [str(v) for v in ebv["ID"]] == train[:10] + candidates
    assert eng.output_loads == 1 and eng.n_out == 50 and eng.ebv_calls >= 1
    assert np.isfinite(ebv["EBV"].to_numpy(dtype=np.float64)).all() and np.any(ebv["EBV"].to_numpy(dtype=np.float64) != 0)
    assert open(tmp_path / "list" / "IDs_for_individuals_with_genotypes.txt").read().split() == train
    # the payload behind those rows: the reader's codes of exactly these individuals over the training selection
    M = PR.read_bed(prefix + ".bed", N_FILE, P_FILE, "A1")
    rows = [ids.index(i) for i in train[:10] + candidates]
    assert np.array_equal(eng.get_output_packed2bit(0, eng.p), PR.pack_codes(PR.codes_of(M[rows][:, geno.selected])))
    # the training IDs in the list get the values of the default run (same seed, same chain)
    eng2 = POR.PlinkOutputChainEngine()
    geno2 = _quiet(api.plink_genotypes, prefix, keep=train, engine=eng2, method="BayesC", Pi=0.9)
    base = _run(geno2, ph, None, tmp_path / "default")["EBV_y"]
    assert [str(v) for v in base["ID"]] == train and eng2.output_loads == 0
    assert np.array_equal(ebv["EBV"].to_numpy()[:10], base["EBV"].to_numpy()[:10])
    # the list that equals the training records in order loads nothing
    eng3 = POR.PlinkOutputChainEngine()
    geno3 = _quiet(api.plink_genotypes, prefix, keep=train, engine=eng3, method="BayesC", Pi=0.9)
    same = _run(geno3, ph, train, tmp_path / "same")["EBV_y"]
    assert eng3.output_loads == 0 and eng3.ebv_calls == 0
    pd.testing.assert_frame_equal(same, base, check_exact=True)


def test_outputebv_list_errors_before_the_chain(fileset, tmp_path):
    prefix, G, ids, train_rows = fileset
    train = [ids[i] for i in train_rows]
    ph = _phenotypes(G, ids, train_rows)
    eng = POR.PlinkOutputChainEngine()
    geno = _quiet(api.plink_genotypes, prefix, keep=train, engine=eng, method="BayesC", Pi=0.9)
    with pytest.raises(ValueError, match="none of the listed individuals"):
        _run(geno, ph, ["nobody", "nobody2"], tmp_path / "empty")
    with pytest.raises(ValueError, match="listed twice"):
        _run(geno, ph, [ids[0], ids[1], ids[0]], tmp_path / "twice")
    assert eng.output_loads == 0


def test_the_other_resident_matrices_keep_their_refusal(fileset, tmp_path):
    """storage="stream" and a device_genotypes object without a PLINK source answer outputEBV(model, IDs) as before."""
    from jwas_jl_amd import streaming as S
    prefix, G, ids, train_rows = fileset
    train = [ids[i] for i in train_rows]
    ph = _phenotypes(G, ids, train_rows)
    backend = _quiet(S.prepare_streaming_genotypes, prefix + ".bed", tmp_path / "backend", input_format="plink", engine=PR.PlinkStandInEngine(), keep=train)
    stream = _quiet(api.get_genotypes, backend, method="BayesC", Pi=0.9, storage="stream")
    with pytest.raises(NotImplementedError) as err:
        _run(stream, ph, train[:20], tmp_path / "stream", _engine=POR.PlinkOutputChainEngine())
    assert REFUSAL in str(err.value)
    eng = POR.PlinkOutputChainEngine()
    geno = _quiet(api.plink_genotypes, prefix, keep=train, engine=eng, method="BayesC", Pi=0.9)
    plain = api.device_genotypes(eng, method="BayesC", Pi=0.9, obsID=train, alleleFreq=geno.alleleFreq, sum2pq=geno.sum2pq)
    assert getattr(plain, "plink_source", None) is None
    with pytest.raises(NotImplementedError) as err:
        _run(plain, ph, train[:20], tmp_path / "plain")
    assert REFUSAL in str(err.value)
    assert eng.output_loads == 0
