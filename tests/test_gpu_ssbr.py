"""The single-step imputation session on the device (jwas_hip_ss_*, csrc/ssbr.hpp) and runMCMC(single_step_analysis=True) end to end.

The solve is judged by its componentwise residual against the standard backward-error bound of a sparse LU solve,

    |Ai_nn X + Ai_ng Mg|  <=  4 (l + 2) 2^-53 (Pr'|L||U|Pc' |X| + |Ai_ng||Mg|),      l = the longest row of L, U or [Ai_nn Ai_ng]

(every solution element is a sum of at most l products accumulated by fma and one division: forward and backward substitution each
contribute (l + 1) u relative to |L||U||X|, forming the right-hand side (l + 1) u relative to |Ai_ng||Mg|, evaluating the residual in
Float64 here as much again; 4 (l + 2) covers their sum) -- derived, not measured.  The tests without the gpu marker check on the CPU
that SciPy's own solution meets the same bounds on the same inputs, and that the chain tolerances of the end-to-end comparison
absorb a 1e-13 relative perturbation of the imputed matrix."""
import contextlib
import functools
import io

import numpy as np
import pytest

import ssbr_reference as SR
import locpar_ped_reference as PR
from ssbr_reference import SsOracleEngine, SsOracleEngine64

EINVAL, ESTATE, EUNSUP, ENOMEM = -1, -3, -4, -5
U53 = 2.0 ** -53
P_COLS, CHUNK = 70, 64


@functools.lru_cache(maxsize=None)
def _solve_case(kind):
    """n_n = 83, g = 37, 70 right-hand sides.  kind "plain": 42 founders + 3 x 26 by 4 sires; "long": the long-row pedigree (a0 and 42
    of its offspring non-genotyped)."""
    from jwas_jl_amd.single_step import Pedigree
    if kind == "plain":
        ped = Pedigree(*PR.generate_pedigree(42, 3, 26, 4, 0.1, seed=11))
        gen, non = SR.split(ped, 37, seed=2)
    else:
        cs = SR.small_case()
        ped, gen, non = cs["ped"], cs["gen"], cs["non"]
    assert len(non) == 83 and len(gen) == 37
    Ai_nn, Ai_ng, lu = SR.blocks(ped, gen)
    rng = np.random.default_rng(17)
    fr = rng.uniform(0.1, 0.9, P_COLS)
    Mg = rng.binomial(2, fr, size=(37, P_COLS)).astype(np.float64) - 2.0 * fr[None, :]
    return dict(ped=ped, gen=gen, non=non, Ai_nn=Ai_nn.tocsr(), Ai_ng=Ai_ng, lu=lu, Mg=np.asfortranarray(Mg))


def _bound(cs, X):
    """(residual, bound) of A^nn X = -A^ng Mg, n_n x columns."""
    import scipy.sparse as sp
    lu, A, Ang, Mg = cs["lu"], cs["Ai_nn"], cs["Ai_ng"], cs["Mg"][:, :X.shape[1]]
    n = A.shape[0]
    Pr = sp.csc_matrix((np.ones(n), (lu.perm_r, np.arange(n))), shape=(n, n))
    Pc = sp.csc_matrix((np.ones(n), (np.arange(n), lu.perm_c)), shape=(n, n))
    B = Pr.T @ (abs(lu.L) @ abs(lu.U)) @ Pc.T
    ell = max(int(np.diff(lu.L.tocsr().indptr).max()), int(np.diff(lu.U.tocsr().indptr).max()), int((np.diff(A.indptr) + np.diff(Ang.indptr)).max()))
    return np.abs(A @ X + Ang @ Mg), 4 * (ell + 2) * U53 * (B @ np.abs(X) + abs(Ang) @ np.abs(Mg)), ell


def _rows(cs, n_rec=65, seed=3):
    """Record rows (duplicates, genotyped and non-genotyped mixed) and output rows (the whole pedigree) as rows of [M_n; M_g]."""
    rng = np.random.default_rng(seed)
    first = rng.choice(120, 60, replace=False)
    prow = np.concatenate([first, rng.choice(first, n_rec - 60, replace=False)]).astype(np.int32)
    assert (prow < 83).any() and (prow >= 83).any()
    at = {v: i for i, v in enumerate(cs["non"] + cs["gen"])}
    return prow, np.array([at[v] for v in cs["ped"].ids], dtype=np.int32)


def _dense(cs):
    """The stand-in's [M_n; M_g] in Float64."""
    Mg = cs["Mg"]
    return np.vstack([np.linalg.solve(cs["Ai_nn"].toarray(), -(cs["Ai_ng"] @ Mg)), Mg])


# ---- on the CPU: the bars hold for SciPy's own solve on these inputs -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "long"])
def test_scipy_solution_meets_the_residual_bound(kind):
    cs = _solve_case(kind)
    X = cs["lu"].solve(-(cs["Ai_ng"] @ cs["Mg"]))
    res, bound, ell = _bound(cs, X)
    assert ell >= (40 if kind == "long" else 5)
    assert np.all(res <= bound)
    if kind == "long":
        # the Float32 bar of the scatter test, on its inputs (the long-row pedigree, the block as it arrives in Float32): SciPy against
        # the dense solve, both rounded to Float32 -- within one ulp, at most 0.1 % differ at all.  (In the "plain" pedigree some
        # founders have no genotyped relative: their imputed genotypes are exactly 0 and a solver's rounding noise around 0 is not
        # within an ulp of anything, so the scatter test does not use it.)
        cs32 = dict(cs, Mg=cs["Mg"].astype(np.float32).astype(np.float64))
        a, b = cs["lu"].solve(-(cs["Ai_ng"] @ cs32["Mg"])).astype(np.float32), _dense(cs32)[:83].astype(np.float32)
        assert np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))) and np.mean(a != b) <= 1e-3


def _e2e(traits, engine, folder, weighted):
    from jwas_jl_amd import api
    cs = SR.small_case(traits=tuple(traits))
    with contextlib.redirect_stdout(io.StringIO()):
        G = 1.0 if len(traits) == 1 else np.array([[1.0, 0.3], [0.3, 0.8]])
        geno = api.get_genotypes(cs["gdf"], G, method="BayesC", Pi=0.9 if len(traits) == 1 else 0.0, double_precision=True)
        model = api.build_model("\n".join(f"{tr} = intercept + age + geno" for tr in traits))
        api.set_covariate(model, "age")
        out = api.runMCMC(model, cs["ph"], single_step_analysis=True, pedigree=cs["ped"], chain_length=40, burnin=10, seed=13, double_precision=True,
                          heterogeneous_residuals=weighted, output_folder=str(folder), _engine=engine)
    return out, cs


def _compare(outs, tmp_path, traits, nlp):
    """The bars of tests/test_gpu_locpar_ped.py::_compare."""
    eo, eh = outs["ref"]["marker effects geno"], outs["hip"]["marker effects geno"]
    d_eff = np.abs(eh["Estimate"].to_numpy(dtype=np.float64) - eo["Estimate"].to_numpy(dtype=np.float64)).max()
    d_ebv = max(np.abs(outs["hip"][f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64) - outs["ref"][f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64)).max()
                for tr in traits)
    lo, lh = outs["ref"]["location parameters"], outs["hip"]["location parameters"]
    assert list(lo["Level"]) == list(lh["Level"]) and len(lo) == len(traits) * nlp
    d_lp = np.abs(lh["Estimate"].to_numpy(dtype=np.float64) - lo["Estimate"].to_numpy(dtype=np.float64)).max()
    key = "_".join(f"{tr}:ϵ" for tr in traits) + "_variances"
    a, b = (np.loadtxt(tmp_path / nm / f"MCMC_samples_{key}.txt", delimiter=",", skiprows=1, ndmin=2) for nm in ("ref", "hip"))
    assert a.shape == b.shape and a.shape[0] == 30
    d_var = float(np.abs(a - b).max())
    print(f"runMCMC single-step {traits}: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, location parameters {d_lp:.3e}, variance samples {d_var:.3e}")
    assert d_eff <= 1e-8 and d_ebv <= 1e-7 and d_lp <= 1e-9 and d_var <= 1e-9
    np.testing.assert_allclose(eh["Model_Frequency"].to_numpy(dtype=np.float64), eo["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)


class _Perturbed64(SsOracleEngine64):
    """The stand-in with its imputed matrices perturbed by 1e-13 relative: what a different but backward-stable solve may return."""

    def ss_impute(self, j0, Mg):
        super().ss_impute(j0, Mg)
        rng = np.random.default_rng(1000 + j0)
        for mat in (self.X, self.X_out):
            mat[:, j0:j0 + np.shape(Mg)[1]] *= 1.0 + 1e-13 * rng.standard_normal((mat.shape[0], np.shape(Mg)[1]))


@pytest.mark.parametrize("traits,weighted", [(["y"], True), (["y1", "y2"], False)])
def test_chain_bars_absorb_a_perturbed_imputation_on_the_cpu(tmp_path, traits, weighted):
    outs = {"ref": _e2e(traits, SsOracleEngine64(), tmp_path / "ref", weighted)[0], "hip": _e2e(traits, _Perturbed64(), tmp_path / "hip", weighted)[0]}
    _compare(outs, tmp_path, traits, 3 + 83)


# ---- on the device ---------------------------------------------------------------------------------------------------------------
def _chunks(p=P_COLS, ldc=CHUNK):
    return [(j0, min(p, j0 + ldc)) for j0 in range(0, p, ldc)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "long"])
def test_solve_meets_the_residual_bound(kind):
    import jwas_jl_amd as J
    cs = _solve_case(kind)
    hip = J.HipEngine(0, precision=64)
    try:
        assert hip.ss_begin(cs["lu"], cs["Ai_ng"], markers_per_chunk=CHUNK) == CHUNK
        allrows = np.arange(120, dtype=np.int32)
        full = np.hstack([hip.ss_solve_host(cs["Mg"][:, a:b], allrows) for a, b in _chunks()])       # 64 columns, then 6
        hip.ss_end()
    finally:
        hip.close()
    assert full.shape == (120, P_COLS) and np.array_equal(full[83:], cs["Mg"])
    res, bound, ell = _bound(cs, full[:83])
    print(f"ss_solve_host {kind}: l = {ell}, worst residual / bound = {np.max(res / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(res <= bound)


def _read_matrices(hip, p):
    """(sweep matrix n x p, output matrix n_out x p) through mul_alpha / mul_alpha_output with unit effect vectors."""
    hip.setup_blocks(64, "f64")
    hip.init_state("BayesC", 1)
    cols, outs = [], []
    for j in range(p):
        e = np.zeros(p, dtype=hip.dtype)
        e[j] = 1.0
        hip.set_state(0, alpha=e)
        cols.append(hip.mul_alpha(0))
        outs.append(hip.mul_alpha_output(0))
    return np.stack(cols, axis=1), np.stack(outs, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 64])
def test_scatter_into_both_targets(precision):
    import jwas_jl_amd as J
    cs = _solve_case("long")
    prow, prow_out = _rows(cs)
    dtype = np.float64 if precision == 64 else np.float32
    ptot, j_first = 80, 5                                       # columns [5, 75) are imputed; the rest keep the poison
    poison = 7.5
    hip = J.HipEngine(0, precision=precision)
    try:
        hip.load_dense(np.full((len(prow), ptot), poison, dtype=dtype, order="F"))          # 65 rows: 191 pad rows up to the granule of 256
        hip.load_output_dense(np.full((len(prow_out), ptot), poison, dtype=dtype, order="F"))
        hip.ss_begin(cs["lu"], cs["Ai_ng"], markers_per_chunk=CHUNK)
        hip.ss_set_rows("sweep", prow)
        hip.ss_set_rows("output", prow_out)
        for a, b in _chunks():
            hip.ss_impute(j_first + a, cs["Mg"][:, a:b].astype(dtype))
        raw = {tg: hip.ss_get_columns(tg, 0, ptot) for tg in ("sweep", "output")}       # all ld rows: the n rows, then the pad rows
        hip.ss_end()
        if precision == 32:
            direct = hip.get_columns(0, ptot)
        X, Xo = _read_matrices(hip, ptot)
    finally:
        hip.close()
    if precision == 32:
        assert np.array_equal(direct, X)                        # the two column readers agree
    lo, hi = j_first, j_first + P_COLS
    for M in (X, Xo):                                           # columns outside [j0, j0 + count) are untouched
        assert np.all(M[:, :lo] == poison) and np.all(M[:, hi:] == poison)
    # pad rows are exactly zero, read as they lie in device memory (the other readers return the n rows only; the unweighted Gram
    # tiles sum over all ld rows); the n rows of that reader are what the two others returned
    for tg, M in (("sweep", X), ("output", Xo)):
        n_ = M.shape[0]
        assert raw[tg].shape == (256, ptot) and raw[tg].dtype == dtype and n_ % 256 != 0
        assert np.array_equal(raw[tg][:n_], M)
        assert np.all(raw[tg][n_:] == 0.0) and not np.any(np.signbit(raw[tg][n_:, lo:hi]))
    Xi, Xoi = X[:, lo:hi], Xo[:, lo:hi]
    assert np.array_equal(Xi, Xoi[[int(np.flatnonzero(prow_out == r)[0]) for r in prow]])          # a record's row is its individual's output row
    if precision == 32:
        cs32 = dict(cs, Mg=cs["Mg"].astype(np.float32).astype(np.float64))                        # (the block arrives in Float32)
        ref = _dense(cs32)
        for got, rows in ((Xi, prow), (Xoi, prow_out)):
            want = ref[rows].astype(np.float32)
            assert np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want))))
            print(f"scatter Float32: {np.mean(got != want):.5f} of the elements differ from the stand-in's")
            assert np.mean(got != want) <= 1e-3
    else:
        full = Xoi[np.argsort(prow_out)]                        # rows of [M_n; M_g] in order
        assert np.array_equal(full[83:], cs["Mg"])
        res, bound, _ = _bound(cs, full[:83])
        assert np.all(res <= bound)


@pytest.mark.gpu
def test_chunk_size_does_not_change_a_bit():
    import jwas_jl_amd as J
    cs = _solve_case("long")
    prow, _ = _rows(cs)
    got = {}
    hip = J.HipEngine(0)
    try:
        for ldc in (64, 256):
            hip.alloc_dense(len(prow), P_COLS)
            assert hip.ss_begin(cs["lu"], cs["Ai_ng"], markers_per_chunk=ldc) == ldc
            hip.ss_set_rows("sweep", prow)
            for a, b in _chunks(ldc=ldc):
                hip.ss_impute(a, cs["Mg"][:, a:b].astype(np.float32))
            host = np.hstack([hip.ss_solve_host(cs["Mg"][:, a:b], prow) for a, b in _chunks(ldc=ldc)])
            assert np.all(hip.ss_get_columns("sweep", 0, P_COLS)[len(prow):] == 0.0)      # (alloc_dense leaves the pad rows as they were: the scatter zeroes them)
            hip.ss_end()
            got[ldc] = (hip.get_columns(0, P_COLS), host)
    finally:
        hip.close()
    assert np.array_equal(got[64][0], got[256][0]) and np.array_equal(got[64][1], got[256][1])


@pytest.mark.gpu
def test_error_contract():
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    from jwas_jl_amd.engine import _csr_arrays
    cs = _solve_case("plain")
    lu, Ang = cs["lu"], cs["Ai_ng"]
    prow, prow_out = _rows(cs)
    L, U, A = (_csr_arrays(M) for M in (lu.L, lu.U, Ang))
    Mg32 = cs["Mg"].astype(np.float32)

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    def begin(L_=L, U_=U, pr=lu.perm_r, pc=lu.perm_c, A_=A, **kw):
        kw.setdefault("markers_per_chunk", CHUNK)
        return hip.ss_begin((L_, U_, pr, pc), A_, **kw)

    def edit(M, fn):
        ptr, col, val = (v.copy() for v in M)
        fn(ptr, col, val)
        return ptr, col, val

    row = int(np.argmax(np.diff(L[0])))                         # a row of L with off-diagonal entries
    assert L[0][row + 1] - L[0][row] >= 3
    urow = int(np.argmax(np.diff(U[0])))
    hip = J.HipEngine(0)
    try:
        # before a session: every other entry point is a call-order error
        hip._ss = (83, 37, CHUNK)
        assert [code(hip.ss_set_rows, "sweep", prow), code(hip.ss_impute, 0, Mg32[:, :8]), code(hip.ss_solve_host, cs["Mg"][:, :2], prow), code(hip.ss_end)] == [ESTATE] * 4
        # _begin validates before any launch
        def swap(ptr, col, val):
            a = ptr[row]
            col[a], col[a + 1] = col[a + 1], col[a]
        def dup(ptr, col, val):
            col[ptr[row] + 1] = col[ptr[row]]
        def oob(ptr, col, val):
            col[ptr[urow + 1] - 1] = 83
        def neg(ptr, col, val):
            col[ptr[row]] = -1
        def zero_diag(ptr, col, val):
            val[ptr[5]] = 0.0
        def nan_diag(ptr, col, val):
            val[ptr[5]] = np.nan
        def l_diag(ptr, col, val):
            val[ptr[row + 1] - 1] = 2.0
        def shift_ptr(ptr, col, val):
            ptr[0] = 1
        # U with an entry below its diagonal / L with one above: move the diagonal out of place
        def u_lower(ptr, col, val):
            col[ptr[urow]] = 0 if urow > 0 else 1
        for bad in (dict(L_=edit(L, swap)), dict(L_=edit(L, dup)), dict(U_=edit(U, oob)), dict(L_=edit(L, neg)), dict(U_=edit(U, zero_diag)),
                    dict(U_=edit(U, nan_diag)), dict(L_=edit(L, l_diag)), dict(L_=edit(L, shift_ptr)), dict(U_=edit(U, u_lower)),
                    dict(A_=edit(A, lambda ptr, col, val: col.__setitem__(0, 37)), g=37),
                    dict(pr=np.where(np.arange(83) == 0, lu.perm_r[1], lu.perm_r)), dict(pc=np.full(83, 83, dtype=np.int32)),
                    dict(L_=U, U_=L)):
            assert code(begin, **bad) == EINVAL, bad.keys()
        assert code(begin, budget_bytes=1000) == ENOMEM
        hip.comm_init_loopback(0, 0, 1)
        assert code(begin) == EUNSUP                            # a context with a communicator
        hip.comm_destroy()
        assert begin() == CHUNK
        # targets
        assert code(hip.ss_impute, 0, Mg32[:, :8]) == ESTATE    # no target rows
        assert code(hip.ss_set_rows, "sweep", prow) == ESTATE   # no matrix
        assert code(hip.ss_set_rows, "output", prow_out) == ESTATE
        hip.alloc_dense(len(prow), P_COLS)
        assert code(hip.ss_set_rows, "sweep", prow[:-1]) == EINVAL
        assert code(hip.ss_set_rows, 2, prow) == EINVAL
        assert code(hip.ss_set_rows, "sweep", np.where(np.arange(len(prow)) == 3, 120, prow)) == EINVAL
        assert code(hip.ss_solve_host, cs["Mg"][:, :2], np.array([-1], dtype=np.int32)) == EINVAL
        hip.ss_set_rows("sweep", prow)
        assert code(hip.ss_impute, 0, Mg32[:, :65]) == EINVAL   # count > ldc
        assert code(hip.ss_impute, 64, Mg32[:, :8]) == EINVAL   # past the last column
        assert code(hip.ss_solve_host, cs["Mg"][:, :65], prow) == EINVAL
        hip.ss_impute(0, Mg32[:, :CHUNK])
        assert code(hip.ss_get_columns, "sweep", 0, P_COLS + 1) == EINVAL
        assert code(hip.ss_get_columns, "output", 0, 1) == ESTATE         # no output matrix
        hip.alloc_dense(len(prow) + 1, P_COLS)                            # (no blocks are set up: only the size guard can fire)
        assert code(hip.ss_impute, 0, Mg32[:, :CHUNK]) == ESTATE          # the target was replaced by a matrix of another size
        hip.alloc_dense(len(prow), P_COLS)
        hip.ss_impute(0, Mg32[:, :CHUNK])                                 # ... and by one of the same size: the rows still fit
        hip.setup_blocks(64, "f64")
        assert code(hip.ss_impute, 0, Mg32[:, :CHUNK]) == ESTATE          # x'x and the Grams depend on the matrix
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.ss_impute, 0, Mg32[:, :CHUNK]) == EUNSUP
        hip.comm_destroy()
        hip.ss_end()
        assert code(hip.ss_end) == ESTATE
        nnz = (len(L[1]), len(U[1]), len(A[1]))
        for chunk in (1, 64, 65, 1000, 10 ** 6):
            assert J.HipEngine.ss_estimate_bytes(83, 37, *nnz, chunk) == SR.estimate_bytes(83, 37, *nnz, chunk) > 8 * 64 * 83
    finally:
        hip.close()


@pytest.mark.gpu
@pytest.mark.parametrize("traits,weighted", [(["y"], True), (["y1", "y2"], False)])
def test_runmcmc_float64_gpu_vs_standin(tmp_path, traits, weighted):
    outs = {"ref": _e2e(traits, SsOracleEngine64(), tmp_path / "ref", weighted)[0], "hip": _e2e(traits, None, tmp_path / "hip", weighted)[0]}
    _compare(outs, tmp_path, traits, 3 + 83)
    assert list(outs["hip"]["EBV_" + traits[0]]["ID"]) == SR.small_case()["ped"].ids


@pytest.mark.gpu
def test_runmcmc_float32_contract(tmp_path):
    """A short Float32 run on dense storage: it completes, everything is finite, tables and files as in the host test."""
    import os
    from jwas_jl_amd import api
    cs = SR.small_case()
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(cs["gdf"], 1.0, method="BayesC", Pi=0.9)
        model = api.build_model("y = intercept + age + geno")
        api.set_covariate(model, "age")
        out = api.runMCMC(model, cs["ph"], single_step_analysis=True, pedigree=cs["ped"], chain_length=12, burnin=4, seed=3, output_folder=str(tmp_path / "r"))
    lp = out["location parameters"]
    assert list(lp["Effect"]) == ["intercept", "age"] + ["ϵ"] * 83 + ["J"] and list(lp["Level"][2:85]) == cs["non"]
    assert np.all(np.isfinite(lp["Estimate"])) and np.all(np.isfinite(lp["SD"]))
    assert list(out["EBV_y"]["ID"]) == cs["ped"].ids and np.all(np.isfinite(out["EBV_y"]["EBV"])) and np.all(np.isfinite(out["EBV_y"]["PEV"]))
    assert np.all(np.isfinite(out["marker effects geno"]["Estimate"])) and np.all(np.isfinite(out["y:ϵ_variances"]["Estimate"]))
    assert "heritability" not in out and "genetic_variance" not in out
    for nm, shape in (("MCMC_samples_y.ϵ.txt", (8, 83)), ("MCMC_samples_y.J.txt", (8, 1)), ("MCMC_samples_y:ϵ_variances.txt", (8, 1))):
        tab = np.loadtxt(tmp_path / "r" / nm, delimiter=",", skiprows=1, ndmin=2)
        assert tab.shape == shape and np.all(np.isfinite(tab)), nm
    assert not os.path.exists(tmp_path / "r" / "MCMC_samples_heritability.txt")
