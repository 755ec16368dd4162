"""The pedigree random effect on the device (csrc/locpar.hpp, k_locpar_draw_structured and the quadratic-form kernels) through
the C ABI and runMCMC, against the numpy restatement of tests/locpar_ped_reference.py on the same Philox counters and on the
DEVICE's own colours (locpar_group_colors).

TERM BY TERM the device and the restatement start from one common state.  Both evaluate the same formulas in double; they differ
in the order of the sums and in the libm behind Box-Muller.  The bound of tests/test_gpu_locpar.py (_level_bound), with three
changes for a structured term, u = 2^-53:

    own_l = 2 (n_l + k nnz_l + t + 4) u A_l / lhs_l + 16 u (|mean_l| + sd_l) + 2^-46 sd_l
    A_l   = sum_{i in l} w_i |x_i| sum_m |c_km r_m,i| + |d_l c_kk sol_l| + sum_m sum_j |p_km V_lj u_m,j|
    e_l  <= own_l + sum_{j in an earlier colour} |p_kk V_lj| e_j / lhs_l

n_l is widened by the k nnz_l prior products of the k member terms, A_l by their absolute values, and a level of a later colour
reads the device's values of its neighbours in earlier colours, which differ from the restatement's by e_j.
Every test prints the figures it measured before it asserts."""
import contextlib
import functools
import io

import numpy as np
import pandas as pd
import pytest

import locpar_reference as LP
import locpar_ped_reference as PR
from locpar_ped_reference import PedOracleEngine, PedOracleEngine64
from test_gpu_locpar import _genotypes, _level_bound, _phenotypes, _spd, _ulp32

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EINVAL, ESTATE, EUNSUP = -1, -3, -4


@functools.lru_cache(maxsize=None)
def _pedigree(size):
    """200 animals (20 founders + 3 x 60) or 10 200 (200 founders + 5 x 2 000); the structure as set_random passes it on."""
    from jwas_jl_amd.single_step import Pedigree
    ped = PR.ped200() if size == 200 else Pedigree(*PR.generate_pedigree(200, 5, 2000, 8, 0.1, seed=10200))
    assert len(ped.ids) == size
    return ped, PR.structure_from_pedigree(ped)


def _records(q, n, rng):
    """Levels of n records over q animals: a tenth of the records on animal 5, the rest on animals whose index is not a multiple
    of 3 (repeated records; every third animal has none)."""
    lev = rng.integers(0, q, n)
    lev = np.where(lev % 3 == 0, (lev + 1) % q, lev)
    lev = np.where(lev % 3 == 0, lev + 1, lev)
    lev[rng.random(n) < 0.1] = 5
    return lev.astype(np.int32)


def _setup(precision, size, n, t, weighted, seed=3):
    """Per trait: intercept; the animal term (random effect 0, structured); a 7-level herd term (random effect 1, i.i.d.)."""
    import jwas_jl_amd as J
    rng = np.random.default_rng(seed + 17 * t)
    ped, V = _pedigree(size)
    q = len(ped.ids)
    X = _genotypes(n, precision)
    hip = J.HipEngine(0, precision=precision)
    ref = PedOracleEngine64() if precision == 64 else PedOracleEngine("block")
    w = rng.uniform(0.25, 4.0, n) if weighted else None
    r0 = rng.standard_normal((t, n)) * 1.3
    lev, herd = _records(q, n, rng), rng.integers(0, 7, n).astype(np.int32)
    for e in (hip, ref):
        e.load_dense(X)
        e.set_weights(None if w is None else w.astype(X.dtype))
        e.setup_blocks(64, "f64")
        e.init_state("BayesC" if t == 1 else "MTBayesC", t)
        for k in range(t):
            e.set_residual(r0[k].astype(X.dtype), k)
        e.locpar_begin(t)
        e.locpar_set_group_structure(0, V.indptr, V.indices, V.data)
        for k in range(t):
            e.locpar_add_covariate(k, None)
            e.locpar_add_factor(k, lev, q, 0)
            e.locpar_add_factor(k, herd, 7, 1)
    kw = dict(vare=1.7) if t == 1 else dict(Rinv=np.linalg.inv(_spd(t, rng, 0.8)))
    if t > 1:
        kw["Rinv"] = (kw["Rinv"] + kw["Rinv"].T) / 2
    kw["Gi"] = [_spd(t, rng, s) for s in (2.0, 0.7)]
    # the stand-in visits the DEVICE's colours
    color = hip.locpar_group_colors(0)
    ref._lp_struct[0] = PR.prepare_structure(V, color)
    sol0 = rng.standard_normal(ref.locpar_size())
    return hip, ref, kw, sol0, V, color, lev


def _structured_bound(det, t, W):
    """own_l and its propagation through the colours (module docstring); n_l already holds the k nnz_l prior products."""
    own = _level_bound(det, t)
    e = np.zeros_like(own)
    for L, absrows in zip(W["levels"], W["absrows"]):
        e[L] = own[L] + np.abs(det["pkk"]) * (absrows @ e) / det["lhs"][L]          # (e of later colours is still zero here)
    return e


def _check_properties(V, color, lev):
    """What the parity cases rely on, asserted rather than trusted."""
    from jwas_jl_amd import api
    nnz_l = np.diff(V.indptr)
    coo = V.tocoo()
    offd = coo.row != coo.col
    assert np.all(color[coo.row[offd]] != color[coo.col[offd]]) and np.array_equal(color, PR.greedy_colors(V))
    assert color.max() + 1 >= 4
    assert nnz_l.max() > PR.LONG_ROW and nnz_l.max() > 64 and (nnz_l <= PR.LONG_ROW).any()
    frac = np.abs(V.data * 4096) % 1                                       # an inbred animal: values that are no small dyadic fraction
    assert (frac != 0).any()
    assert (np.bincount(lev, minlength=V.shape[0]) == 0).any()              # an animal without records


PARITY_CASES = [(p, 200, 1003, t, w) for p in (64, 32) for t in (1, 3) for w in (False, True)] + [(64, 10200, 20011, 1, True)]


@pytest.mark.parametrize("precision,size,n,t,weighted", PARITY_CASES)
def test_term_by_term_parity(precision, size, n, t, weighted):
    hip, ref, kw, sol0, V, color, lev = _setup(precision, size, n, t, weighted)
    dtype = np.float64 if precision == 64 else np.float32
    try:
        _check_properties(V, color, lev)
        if size > 200:
            assert max(np.bincount(color)) > 256                            # several workgroups per colour
        assert hip.locpar_size() == ref.locpar_size() == len(sol0)
        ref.locpar_set_sol(sol0)
        worst_sol = worst_res = 0.0
        flips = total = 0
        for j, T in enumerate(ref._lp_terms):
            k = T.trait
            for m in range(t):                                   # the common state
                hip.set_residual(ref.get_residual(m), m)
            before_sol, before_r = ref.locpar_get_sol(), ref.get_residual(k).astype(np.float64)
            hip.locpar_set_sol(before_sol)
            det = []
            ref.locpar_step(iteration=2, seed=77, first_term=j, last_term=j + 1, details=det, **kw)
            hip.locpar_step(iteration=2, seed=77, first_term=j, last_term=j + 1, **kw)
            got, want = hip.locpar_get_sol(), ref.locpar_get_sol()
            sl = slice(T.off, T.off + T.nlevels)
            other = np.ones(len(got), dtype=bool)
            other[sl] = False
            assert np.array_equal(got[other], before_sol[other])            # only this term moved: the other terms' sol bit-unchanged
            structured = T.group == 0
            if structured:
                assert np.all(det[0]["lhs"] > 0)                             # a level with lhs = 0 cannot occur
                assert np.all(got[sl] != before_sol[sl])                     # every level was drawn, the ones without records too
            bound = _structured_bound(det[0], t, ref._lp_struct[0]) if structured else _level_bound(det[0], t)
            err = np.abs(got[sl] - want[sl])
            live = det[0]["live"]
            ratio = float(np.max(err[live] / bound[live]))
            if structured:
                worst_sol = max(worst_sol, ratio)
            assert ratio <= 1.0, (j, ratio)
            for m in range(t):                                               # other traits' residuals bit-unchanged
                if m != k:
                    assert np.array_equal(hip.get_residual(m), ref.get_residual(m))
            r_dev, r_ref = hip.get_residual(k).astype(np.float64), ref.get_residual(k).astype(np.float64)
            delta_dev = got[sl] - before_sol[sl]
            own = LP.term_apply(T, before_r.astype(dtype), delta_dev, dtype).astype(np.float64)
            lvl = np.maximum(T.level, 0)
            xd = np.where(T.inl, np.abs(T.x * delta_dev[lvl]), 0.0)
            slack = 4 * U * (np.abs(before_r) + xd)
            if precision == 64:
                assert np.all(np.abs(r_dev - own) <= slack)
                lim = np.where(T.inl, np.abs(T.x) * bound[lvl], 0.0) + slack
                worst_res = max(worst_res, float(np.max(np.abs(r_dev - r_ref) / np.maximum(lim, 1e-300))))
                assert np.all(np.abs(r_dev - r_ref) <= lim)
            else:
                assert np.array_equal(r_dev, own)
                diff = np.abs(r_dev - r_ref)
                assert np.all(diff <= _ulp32(r_ref))
                flips += int((diff != 0).sum())
                total += n
        print(f"locpar-ratio ped parity p{precision} q{size} n{n} t{t} w{int(weighted)} colours {color.max() + 1}: sol {worst_sol:.3f}"
              + (f", residual {worst_res:.3f}" if precision == 64 else f", float32 roundings that differ {flips} of {total}"))
        assert flips <= max(1, total // 10000)
    finally:
        hip.close()


def test_quadratic_forms():
    """utu of the structured effect: symmetric, within 2 (nnz + q) u sum |u_a,l V_lj u_b,j| of the numpy product; the i.i.d.
    effect next to it keeps U'U."""
    t = 3
    hip, ref, kw, sol0, V, color, lev = _setup(64, 200, 1003, t, True)
    try:
        hip.locpar_set_sol(sol0)
        worst = 0.0
        for it in range(1, 4):
            st = hip.locpar_step(iteration=it, seed=9, **kw)
            sol = hip.locpar_get_sol()
            for g, members in sorted(ref._lp_groups.items()):
                Um = np.stack([sol[ref._lp_terms[j].off:ref._lp_terms[j].off + ref._lp_terms[j].nlevels] for j in members])
                q = Um.shape[1]
                if g == 0:
                    want, lim = Um @ (V @ Um.T), 2 * (V.nnz + q) * U * (np.abs(Um) @ (abs(V) @ np.abs(Um).T))
                else:
                    want, lim = Um @ Um.T, 2 * q * U * (np.abs(Um) @ np.abs(Um).T)
                assert st["utu"][g].shape == (t, t) and np.array_equal(st["utu"][g], st["utu"][g].T)
                worst = max(worst, float(np.max(np.abs(st["utu"][g] - want) / lim)))
                assert np.all(np.abs(st["utu"][g] - want) <= lim)
        print(f"locpar-ratio ped quadratic forms: {worst:.3f}")
    finally:
        hip.close()


def _synthetic_structure(q):
    """A sparse symmetric positive definite q x q matrix that is no pedigree's: tridiagonal, plus three rows (and columns) of about 40,
    300 and 700 entries -- each longer than the rows a single thread adds, the longest among the last 256 rows; strictly
    diagonally dominant."""
    import scipy.sparse as sp
    rng = np.random.default_rng(q)
    off = sp.diags([np.full(q - 1, -0.3)], [1], shape=(q, q), format="lil")
    for row, cnt in ((100, 40), (30_000, 300), (q - 100, 700)):
        cols = rng.choice(q, cnt, replace=False)
        cols = cols[np.abs(cols - row) > 1]
        lo, hi = cols[cols < row], cols[cols > row]
        off[lo, row] = rng.uniform(-0.02, 0.02, len(lo))
        off[row, hi] = rng.uniform(-0.02, 0.02, len(hi))
    off = sp.triu(off.tocsr(), 1)
    V = off + off.T
    V = (V + sp.diags(1.0 + np.asarray(abs(V).sum(axis=1)).ravel())).tocsr()
    V.sort_indices()
    return V


@pytest.mark.parametrize("t", [1, 3])
def test_quadratic_forms_over_more_than_256_workgroups(t):
    """test_quadratic_forms' bound at 65 836 levels: 258 workgroups of k_locpar_quad_rows, so k_locpar_quad_reduce's threads 0 and 1
    take a second trip over the per-workgroup sums.  Against scipy.sparse in float64."""
    import jwas_jl_amd as J
    q, n = 65_836, 1003
    V = _synthetic_structure(q)
    nnz_l = np.diff(V.indptr)
    assert (q + 255) // 256 == 258 and abs(V - V.T).max() == 0 and [c // 10 for c in sorted(nnz_l)[-3:]] == [4, 30, 70] and PR.LONG_ROW < 40
    assert nnz_l[65_536:].max() == nnz_l.max()
    rng = np.random.default_rng(5 + t)
    hip = J.HipEngine(0, precision=64)
    try:
        hip.load_dense(_genotypes(n, 64)); hip.setup_blocks(64, "f64"); hip.init_state("BayesC" if t == 1 else "MTBayesC", t)
        for k in range(t):
            hip.set_residual(rng.standard_normal(n) * 1.3, k)
        hip.locpar_begin(t)
        hip.locpar_set_group_structure(0, V.indptr, V.indices, V.data)
        lev = _records(q, n, rng)
        for k in range(t):
            hip.locpar_add_factor(k, lev, q, 0)
        assert hip.locpar_size() == t * q
        kw = dict(vare=1.7) if t == 1 else dict(Rinv=np.linalg.inv(_spd(t, rng, 0.8)))
        if t > 1:
            kw["Rinv"] = (kw["Rinv"] + kw["Rinv"].T) / 2
        kw["Gi"] = [_spd(t, rng, 2.0)]
        hip.locpar_set_sol(rng.standard_normal(t * q))
        worst = 0.0
        for it in (1, 2):
            st = hip.locpar_step(iteration=it, seed=9, **kw)
            Um = hip.locpar_get_sol().reshape(t, q)
            want, lim = Um @ (V @ Um.T), 2 * (V.nnz + q) * U * (np.abs(Um) @ (abs(V) @ np.abs(Um).T))
            tail = Um[:, 65_536:] @ (V[65_536:] @ Um.T)                        # what the rows of the last two workgroups contribute
            assert np.all(np.abs(np.diag(tail)) > lim.diagonal())               # (a reduction that stops at 256 sums cannot pass)
            got = st["utu"][0]
            assert got.shape == (t, t) and np.array_equal(got, got.T)
            worst = max(worst, float(np.max(np.abs(got - want) / lim)))
            assert np.all(np.abs(got - want) <= lim)
        print(f"locpar-ratio quadratic forms over 258 workgroups t{t}: {worst:.3f}")
    finally:
        hip.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_same_seed_same_bits_and_running_means(precision):
    outs = []
    for rep in range(2):
        hip, ref, kw, sol0, V, color, lev = _setup(precision, 200, 1003, 3, True)
        try:
            hip.locpar_set_sol(sol0)
            mean, mean2 = np.zeros(len(sol0)), np.zeros(len(sol0))
            for it in range(1, 6):
                hip.locpar_step(iteration=it, seed=5, **kw)
                if it > 2:
                    hip.locpar_accumulate(it - 2)
                    sol = hip.locpar_get_sol()
                    mean += (sol - mean) / (it - 2)
                    mean2 += (sol * sol - mean2) / (it - 2)
            m, m2 = hip.locpar_get_means()
            assert np.array_equal(m, mean) and np.array_equal(m2, mean2)      # the recurrence, bit for bit
            outs.append((hip.locpar_get_sol(), [hip.get_residual(k) for k in range(3)]))
        finally:
            hip.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)
    assert not np.any(outs[0][0] == sol0)


def test_exact_posterior_on_the_device():
    """The case of the CPU experiment (tests/test_locpar_ped_host.py): intercept + the 200-animal term, weights, fixed variances,
    4 000 steps after 200; every chain mean within 5 batch-means standard errors (40 batches) of the mixed-model solve."""
    import jwas_jl_amd as J
    case = PR.posterior_case()
    z_ref = PR.posterior_z(PR.posterior_setup(PedOracleEngine64(), case), case)
    hip = J.HipEngine(0, precision=64)
    try:
        z = PR.posterior_z(PR.posterior_setup(hip, case), case)
        print(f"exact posterior, worst z of 201: device {z.max():.2f}, restatement {z_ref.max():.2f}")
        assert z.shape == (201,) and z.max() <= 5.0
    finally:
        hip.close()


def test_error_contract():
    """The three new entry points return the documented codes before any launch."""
    import jwas_jl_amd as J
    from jwas_jl_amd import _lib
    n = 300
    X = _genotypes(n, 32)
    ped, V = _pedigree(200)
    q = V.shape[0]
    hip = J.HipEngine(0)
    try:
        def code(fn, *a, **kw):
            with pytest.raises(_lib.JwasHipError) as ei:
                fn(*a, **kw)
            return ei.value.code

        def csr(M):
            M = M.tocsr()
            M.sort_indices()
            return M.indptr, M.indices, M.data
        hip.load_dense(X)
        hip.setup_blocks(64, "f64")
        hip.init_state("BayesC", 1)
        assert code(hip.locpar_set_group_structure, 0, *csr(V)) == ESTATE                 # before _begin
        hip.locpar_begin(1)
        assert code(hip.locpar_group_colors, 0) == EINVAL                                 # no structure yet
        assert code(hip.locpar_set_group_structure, 8, *csr(V)) == EINVAL                 # random effect outside 0..7
        ip, ix, vv = csr(V)
        for k, bad in enumerate((np.nan, np.inf)):
            v2 = vv.copy(); v2[k + 3] = bad
            assert code(hip.locpar_set_group_structure, 0, ip, ix, v2) == EINVAL          # non-finite
        i2 = ix.copy(); i2[ip[0]], i2[ip[0] + 1] = ix[ip[0] + 1], ix[ip[0]]
        assert code(hip.locpar_set_group_structure, 0, ip, i2, vv) == EINVAL              # unsorted columns
        i2 = ix.copy(); i2[ip[0] + 1] = ix[ip[0]]
        assert code(hip.locpar_set_group_structure, 0, ip, i2, vv) == EINVAL              # a duplicate column
        i2 = ix.copy(); i2[-1] = q
        assert code(hip.locpar_set_group_structure, 0, ip, i2, vv) == EINVAL              # a column outside the matrix
        D = V.tolil(); D[7, 7] = -1.0
        assert code(hip.locpar_set_group_structure, 0, *csr(D)) == EINVAL                 # a non-positive diagonal
        D = V.tolil(); D[q - 1, q - 1] = 0.0; D = D.tocsr(); D.eliminate_zeros()
        assert code(hip.locpar_set_group_structure, 0, *csr(D)) == EINVAL                 # a missing diagonal
        D = V.tolil(); D[3, 0] = D[3, 0] + 0.25
        assert code(hip.locpar_set_group_structure, 0, *csr(D)) == EINVAL                 # asymmetric values
        D = V.tolil(); D[q - 1, 1] = 0.5
        assert code(hip.locpar_set_group_structure, 0, *csr(D)) == EINVAL                 # an asymmetric pattern
        ip2 = ip.copy(); ip2[5] = ip2[6] + 1
        assert code(hip.locpar_set_group_structure, 0, ip2, ix, vv) == EINVAL             # row pointers that decrease
        hip.locpar_set_group_structure(0, ip, ix, vv)
        color = hip.locpar_group_colors(0)
        assert np.array_equal(color, PR.greedy_colors(V))
        hip._locpar_struct_levels[0] = q + 1
        assert code(hip.locpar_group_colors, 0) == EINVAL                                 # another nlevels
        hip._locpar_struct_levels[0] = q
        lev = (np.arange(n) % 7).astype(np.int32)
        assert code(hip.locpar_add_factor, 0, lev, 7, 0) == EINVAL                        # a member with another nlevels
        hip.locpar_add_factor(0, lev, q, 0)
        assert code(hip.locpar_set_group_structure, 0, ip, ix, vv) == ESTATE              # a member of the effect exists
        hip.locpar_set_group_structure(1, ip, ix, vv)                                     # another effect can still get one
        hip.locpar_get_sol()
        assert code(hip.locpar_set_group_structure, 2, ip, ix, vv) == ESTATE              # after the first use of sol
        st = hip.locpar_step(iteration=1, seed=1, vare=1.0, Gi=[np.eye(1)])
        assert np.all(hip.locpar_get_sol() != 0) and st["utu"][0][0, 0] > 0
        hip.locpar_end()
        assert code(hip.locpar_group_colors, 0) == ESTATE
        assert J.HipEngine.locpar_structure_estimate_bytes(q, V.nnz) == PedOracleEngine.locpar_structure_estimate_bytes(q, V.nnz)
        assert 8 * (q + 1) + 12 * V.nnz + 4 * q <= J.HipEngine.locpar_structure_estimate_bytes(q, V.nnz) < 1e5
        hip.comm_init_loopback(0, 0, 1)                                                   # a sharded context
        assert code(hip.locpar_set_group_structure, 0, ip, ix, vv) == EUNSUP
        hip.comm_destroy()
    finally:
        hip.close()


# ---- runMCMC ------------------------------------------------------------------------------------------------------------------
def _ped_for(ids, seed=4):
    """A pedigree over `ids` plus 40 ancestors without records or genotypes: 40 founders, then len(ids) offspring in 3 generations."""
    from jwas_jl_amd.single_step import Pedigree
    n = len(ids)
    _, sire, dam = PR.generate_pedigree(40, 3, n // 3, 4, 0.1, seed=seed)
    assert len(sire) == 40 + n
    return Pedigree([f"anc{i}" for i in range(40)] + list(ids), sire, dam)


def _compare(outs, tmp_path, traits, nlp):
    eo, eh = outs["ref"]["marker effects geno"], outs["hip"]["marker effects geno"]
    d_eff = np.abs(eh["Estimate"].to_numpy(dtype=np.float64) - eo["Estimate"].to_numpy(dtype=np.float64)).max()
    d_ebv = max(np.abs(outs["hip"][f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64) - outs["ref"][f"EBV_{tr}"]["EBV"].to_numpy(dtype=np.float64)).max()
                for tr in traits)
    lo, lh = outs["ref"]["location parameters"], outs["hip"]["location parameters"]
    assert list(lo["Level"]) == list(lh["Level"]) and len(lo) == len(traits) * nlp
    d_lp = np.abs(lh["Estimate"].to_numpy(dtype=np.float64) - lo["Estimate"].to_numpy(dtype=np.float64)).max()
    a, b = (np.loadtxt(tmp_path / nm / "MCMC_samples_polygenic_effects_variance.txt", delimiter=",", skiprows=1) for nm in ("ref", "hip"))
    assert a.shape == b.shape and a.shape[0] == 30
    d_var = float(np.abs(a - b).max())
    print(f"runMCMC pedigree effect {traits}: effects {d_eff:.3e}, EBVs {d_ebv:.3e}, location parameters {d_lp:.3e}, variance samples {d_var:.3e}")
    assert d_eff <= 1e-8 and d_ebv <= 1e-7 and d_lp <= 1e-9 and d_var <= 1e-9
    np.testing.assert_allclose(eh["Model_Frequency"].to_numpy(dtype=np.float64), eo["Model_Frequency"].to_numpy(dtype=np.float64), atol=1e-12)
    tab = outs["hip"]["polygenic effects covariance matrix"]
    assert list(tab["Covariance"]) == [f"{a_}:ID_{b_}:ID" for a_ in traits for b_ in traits]
    assert not any(k.endswith("ID_variances") for k in outs["hip"])


def test_runmcmc_single_trait_weighted_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = _phenotypes(small_data, ["y"])
    ped = _ped_for(list(ph["ID"]))
    outs = {}
    for name, engine in (("ref", PedOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", Pi=0.9, double_precision=True)
            model = api.build_model("y = intercept + age + ID + geno")
            api.set_covariate(model, "age")
            api.set_random(model, "ID", ped, 0.3)
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True, heterogeneous_residuals=True,
                                     output_folder=str(tmp_path / name), _engine=engine)
    _compare(outs, tmp_path, ["y"], 2 + len(ped.ids))


def test_runmcmc_three_traits_one_threshold_gpu_vs_standin(tmp_path, small_data):
    from jwas_jl_amd import api
    gdf, ph = _phenotypes(small_data, ["a", "b", "c"])
    ph["c"] = np.digitize(ph["c"], [np.median(ph["c"])]) + 1.0
    ped = _ped_for(list(ph["ID"]))
    outs = {}
    for name, engine in (("ref", PedOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            geno = api.get_genotypes(gdf, method="BayesC", double_precision=True)
            model = api.build_model("a = intercept + age + ID + geno\nb = intercept + age + ID + geno\nc = intercept + age + ID + geno",
                                    categorical_trait=["c"])
            api.set_covariate(model, "age")
            api.set_random(model, "ID", ped, np.array([[0.3, 0.1, 0.0], [0.1, 0.4, 0.05], [0.0, 0.05, 0.2]]))
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True,
                                     output_folder=str(tmp_path / name), _engine=engine)
    _compare(outs, tmp_path, ["a", "b", "c"], 2 + len(ped.ids))


def test_runmcmc_float32_packed_storage_contract(tmp_path, small_data):
    """A Float32 run on 2-bit packed storage: it runs, the files and tables are present, all values finite."""
    from jwas_jl_amd import api, streaming as S
    gdf, ph = _phenotypes(small_data, ["y"])
    ph["ID"] = [str(i) for i in range(len(ph))]
    ped = _ped_for(list(ph["ID"]))
    prefix = S.prepare_streaming_genotypes(small_data["raw"].astype(np.float64), tmp_path / "st", obs_ids=list(ph["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", Pi=0.9, storage="stream")
        model = api.build_model("y = intercept + age + ID + geno")
        api.set_covariate(model, "age")
        api.set_random(model, "ID", ped)
        out = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, output_folder=str(tmp_path / "r"))
    lines = open(tmp_path / "r" / "MCMC_samples_polygenic_effects_variance.txt").read().splitlines()
    v = np.array([float(x) for x in lines[1:]])
    assert lines[0] == "y:ID_y:ID" and v.shape == (30,) and np.all(np.isfinite(v)) and np.all(v > 0)
    lp = out["location parameters"]
    assert len(lp) == 2 + len(ped.ids) and list(lp["Level"][2:]) == ped.ids
    assert np.all(np.isfinite(lp["Estimate"])) and np.all(np.isfinite(lp["SD"]))
    assert np.all(np.isfinite(out["polygenic effects covariance matrix"]["Estimate"])) and np.all(np.isfinite(out["EBV_y"]["EBV"]))
    assert np.all(np.isfinite(out["marker effects geno"]["Estimate"]))
