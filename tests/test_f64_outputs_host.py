"""The output side of a Float64 run (runMCMC(double_precision=true), JWAS.jl:349-366) on the host: run_chain hands the EBVs of
the output rows and the sparse sample readout to a Float64 engine that offers them (load_output_dense / mul_alpha_output /
alpha_sparse), and GWAS(double_precision=True) passes Float64 genotypes and effects (GWAS.jl:148-165, :199-217).  The engines
here are numpy stand-ins for the device calls."""
import numpy as np
import pandas as pd

from conftest import make_dataset
from jwas_jl_amd import api
from jwas_jl_amd.gwas import GWAS
from oracle_engine import OracleEngine, OracleEngine64


class CountingEngine64(OracleEngine64):
    """OracleEngine64 + the output calls of a Float64 HipEngine in numpy, counting how often the host uses them."""

    def __init__(self):
        super().__init__()
        self.calls = {"load_output_dense": 0, "mul_alpha_output": 0, "alpha_sparse": 0, "window_sums": 0, "window_sums2": 0}
        self.loaded_dtypes = []

    def load_dense(self, X):
        self.loaded_dtypes.append(np.asarray(X).dtype)
        super().load_dense(X)

    def load_output_dense(self, X_out):
        self.calls["load_output_dense"] += 1
        X_out = np.asarray(X_out)
        assert X_out.dtype == np.float64                       # (HipEngine(precision=64) raises TypeError otherwise)
        self.X_out = X_out
        self.n_out = X_out.shape[0]

    def mul_alpha_output(self, trait=0):
        self.calls["mul_alpha_output"] += 1
        return self.X_out @ self.alpha[trait]

    def alpha_sparse(self, trait=0):
        self.calls["alpha_sparse"] += 1
        a = self.alpha[trait]
        idx = np.flatnonzero(a).astype(np.int32)
        return idx, a[idx].copy()

    def window_sums(self, wptr, idx, val, use_output_rows=False):
        self.calls["window_sums"] += 1
        val = np.asarray(val)
        assert val.dtype == np.float64
        X = self.X_out if use_output_rows else self.X
        idx = np.asarray(idx, dtype=np.int64)
        s, q = np.zeros(len(wptr) - 1), np.zeros(len(wptr) - 1)
        for w in range(len(wptr) - 1):
            bv = X[:, idx[wptr[w]:wptr[w + 1]]] @ val[wptr[w]:wptr[w + 1]]
            s[w], q[w] = bv.sum(), (bv * bv).sum()
        return s, q

    def window_sums2(self, wptr, idx, val1, val2, use_output_rows=False):
        self.calls["window_sums2"] += 1
        v1, v2 = np.asarray(val1), np.asarray(val2)
        assert v1.dtype == np.float64 and v2.dtype == np.float64
        X = self.X_out if use_output_rows else self.X
        idx = np.asarray(idx, dtype=np.int64)
        outs = [np.zeros(len(wptr) - 1) for _ in range(5)]
        for w in range(len(wptr) - 1):
            cols = X[:, idx[wptr[w]:wptr[w + 1]]]
            b1, b2 = cols @ v1[wptr[w]:wptr[w + 1]], cols @ v2[wptr[w]:wptr[w + 1]]
            for o, v in zip(outs, (b1.sum(), (b1 * b1).sum(), b2.sum(), (b2 * b2).sum(), (b1 * b2).sum())):
                o[w] = v
        return tuple(outs)


def _run(engine, tmp_path, tag, ids_out):
    n, p = 180, 150
    d = make_dataset(n=n, p=p, ncausal=5, seed=31, center=False)
    ids = [f"id{i}" for i in range(n)]
    gdf = pd.DataFrame(d["raw"], columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    rng = np.random.default_rng(4)
    ph = pd.DataFrame({"ID": ids, "y1": d["y"], "y2": 0.6 * d["y"] + 0.8 * rng.standard_normal(n)})
    geno = api.get_genotypes(gdf, np.eye(2) * 0.5, method="BayesC", double_precision=True)      # (build_model resolves `geno` by name)
    assert geno.genotypes.dtype == np.float64
    model = api.build_model("y1 = intercept + geno\ny2 = intercept + geno", np.eye(2))
    api.outputEBV(model, ids_out)
    return api.runMCMC(model, ph, chain_length=50, burnin=10, seed=5, double_precision=True, output_samples_frequency=10,
                       output_folder=str(tmp_path / tag), _engine=engine)


def test_f64_run_uses_the_engines_output_rows_and_sparse_readout(tmp_path):
    """outputEBV(model, IDs) with a strict subset of the genotyped individuals in another order: a Float64 engine that offers
    the output calls is used for them (once per load, once per saved sample and trait), and the EBVs equal the host path's
    (the unmodified OracleEngine64: X_out_host @ alpha) -- both fp64 sums of <= p terms of O(1) size, different association."""
    rng = np.random.default_rng(9)
    ids_out = [f"id{i}" for i in rng.permutation(180)[:70]]
    assert ids_out != sorted(ids_out, key=lambda s: int(s[2:]))
    eng = CountingEngine64()
    out_dev = _run(eng, tmp_path, "dev", ids_out)
    out_host = _run(OracleEngine64(), tmp_path, "host", ids_out)
    nsaved, t = 4, 2                                           # iterations 20, 30, 40, 50
    assert eng.calls["load_output_dense"] == 1
    assert eng.calls["mul_alpha_output"] == nsaved * t
    assert eng.calls["alpha_sparse"] == nsaved * t
    for k in ("y1", "y2"):
        assert list(out_dev[f"EBV_{k}"]["ID"]) == ids_out == list(out_host[f"EBV_{k}"]["ID"])
        got = out_dev[f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64)
        assert np.abs(got).max() > 1e-3
        np.testing.assert_allclose(got, out_host[f"EBV_{k}"]["EBV"].to_numpy(dtype=np.float64), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(out_dev["marker effects geno"]["Estimate"].to_numpy(), out_host["marker effects geno"]["Estimate"].to_numpy())


# ---- GWAS(double_precision=True) --------------------------------------------------------------------------------------------
def _literal_gwas64(X, samples, col_start, col_end, threshold):
    """GWAS.jl:148-176 as written there, T = Float64"""
    ns, nw = samples.shape[0], len(col_start)
    winVar, props = np.zeros((ns, nw)), np.zeros((ns, nw))
    for i in range(ns):
        a = samples[i]
        genVar = np.var(X @ a, ddof=1)
        for w in range(nw):
            v = np.var(X[:, col_start[w]:col_end[w]] @ a[col_start[w]:col_end[w]], ddof=1)
            winVar[i, w] = v
            props[i, w] = v / genVar if genVar != 0 else np.nan
    props[np.isnan(props)] = 0.0
    return winVar, props, (props > threshold).mean(axis=0)


def _literal_gcov64(X, s1, s2, col_start, col_end):
    """GWAS.jl:199-217 as written there, T = Float64"""
    ns, nw = s1.shape[0], len(col_start)
    gcov, gcor = np.zeros((ns, nw)), np.zeros((ns, nw))
    for i in range(ns):
        for w in range(nw):
            sl = slice(col_start[w], col_end[w])
            b1, b2 = X[:, sl] @ s1[i, sl], X[:, sl] @ s2[i, sl]
            c = np.cov(b1, b2)
            gcov[i, w] = c[0, 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                gcor[i, w] = c[0, 1] / np.sqrt(c[0, 0] * c[1, 1])
    gcov[np.isnan(gcov)] = 0.0
    gcor[~np.isfinite(gcor)] = 0.0
    return gcov, gcor


def _gwas_case(tmp_path, seed=5, n=70, p=40, ns=20):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, size=(n, p)).astype(np.float64) + 0.25 * rng.standard_normal((n, p))       # real-valued: Float64 digits matter
    X -= X.mean(0)
    ids = [f"m{j + 1}" for j in range(p)]
    files, samples = [], []
    for k in (1, 2):
        s = np.where(rng.random((ns, p)) < 0.2, rng.standard_normal((ns, p)), 0.0)
        s[3] = 0.0                                              # a sample with no marker in the model
        f = tmp_path / f"MCMC_samples_marker_effects_geno_y{k}.txt"
        pd.DataFrame(s, columns=ids).to_csv(f, index=False, float_format="%.17g")
        files.append(f.name); samples.append(s)
    chrom = np.repeat(["1", "2", "3"], [15, 15, 10])
    pos = np.concatenate([np.sort(rng.integers(1, 4_000_000, 15)), np.sort(rng.integers(1, 3_000_000, 15)), np.sort(rng.integers(1, 2_500_000, 10))])
    pd.DataFrame({"markerID": ids, "chromosome": chrom, "position": pos}).to_csv(tmp_path / "map.txt", index=False)
    return X, samples, files


def test_gwas_double_precision_matches_float64_restatement(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                 # (relative file names: the output name is built from them)
    X, (s1, s2), files = _gwas_case(tmp_path)
    eng = CountingEngine64()
    res, props = GWAS(X, "map.txt", files[0], window_size="1 Mb", threshold=0.05, output_winVarProps=True, output_folder=".",
                      double_precision=True, _engine=eng)
    assert eng.loaded_dtypes == [np.dtype(np.float64)] and eng.calls["window_sums"] == s1.shape[0]
    np.testing.assert_array_equal(eng.X, X)                     # the Float64 genotypes as given, not rounded through Float32
    tab = res[0]
    from jwas_jl_amd.gwas import build_windows
    mapf = pd.read_csv("map.txt", dtype={"chromosome": str})
    win = build_windows(mapf["chromosome"].to_numpy(), mapf["position"].to_numpy(dtype=np.int64), 1_000_000, False)
    winVar, wprops, wppa = _literal_gwas64(X, s1, win["col_start"], win["col_end"], 0.05)
    order = np.argsort(-wppa, kind="stable")
    np.testing.assert_array_equal(tab["window"].to_numpy(), order + 1)
    np.testing.assert_array_equal(tab["WPPA"].to_numpy(), wppa[order])
    np.testing.assert_allclose(tab["estimateGenVar"].to_numpy(), winVar.mean(axis=0)[order], rtol=1e-12)
    np.testing.assert_allclose(props[0], wprops, rtol=1e-10, atol=1e-15)
    # the window genetic covariance / correlation of two traits' samples
    eng2 = CountingEngine64()
    res2 = GWAS(X, "map.txt", files[0], files[1], GWAS=False, genetic_correlation=True, output_folder=".", double_precision=True, _engine=eng2)
    assert eng2.calls["window_sums2"] == s1.shape[0]
    gcov, gcor = _literal_gcov64(X, s1, s2, win["col_start"], win["col_end"])
    np.testing.assert_allclose(res2[-1]["estimate_cov"].to_numpy(), gcov.mean(axis=0), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(res2[-1]["estimate_cor"].to_numpy(), gcor.mean(axis=0), rtol=1e-9, atol=1e-12)


def test_gwas_default_stays_float32(tmp_path, monkeypatch):
    """double_precision=False (the default) is the Float32 path: the genotypes and the effects reach the engine as Float32,
    and the tables equal those of a call that does not name the option."""
    monkeypatch.chdir(tmp_path)
    X, _, files = _gwas_case(tmp_path, seed=8)

    class Spy(OracleEngine):
        seen = []

        def load_dense(self, Xd):
            Spy.seen.append(np.asarray(Xd).dtype)
            super().load_dense(Xd)

        def window_sums(self, wptr, idx, val, use_output_rows=False):
            Spy.seen.append(np.asarray(val).dtype)
            return super().window_sums(wptr, idx, val, use_output_rows)

    a = GWAS(X, "map.txt", files[0], threshold=0.05, output_folder=".", _engine=OracleEngine("dense"))[0]
    b = GWAS(X, "map.txt", files[0], threshold=0.05, output_folder=".", double_precision=False, _engine=Spy("dense"))[0]
    assert set(Spy.seen) == {np.dtype(np.float32)}
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    # ... and differs from the Float64 evaluation in the digits Float32 genotypes cannot hold
    c = GWAS(X, "map.txt", files[0], threshold=0.05, output_folder=".", double_precision=True, _engine=CountingEngine64())[0]
    a_, c_ = a.sort_values("window"), c.sort_values("window")
    assert not np.array_equal(a_["estimateGenVar"].to_numpy(), c_["estimateGenVar"].to_numpy())
    np.testing.assert_allclose(a_["estimateGenVar"].to_numpy(), c_["estimateGenVar"].to_numpy(), rtol=1e-4)
