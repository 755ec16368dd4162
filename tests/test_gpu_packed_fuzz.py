"""2-bit packed storage, BIT FOR BIT: the sweep on a packed context (update_role_wide: 1024-row slices, one dword = 16
individuals per lane, the centring factored out of the sum per lane, the missing-code patch, the ragged-row mask) against the
oracle summing a block's x'R^-1 r in that kernel's own association order (oracle dot_xr with a packed source and ACC_DEVICE).
The harness is test_gpu_fuzz.py's: both sides use the oracle's x'x, Grams and cross-Grams, four sweeps, and every effect,
indicator and residual element of every trait must be EQUAL, as must the number of changes per sweep.  Pinned edge shapes
first, then a seeded sample of the whole configuration space; the grouped launches (not bit-exact on dense storage either)
are held to the bars of test_gpu_packed.py."""
import os

import numpy as np
import pytest

from conftest import make_dataset
from oracle_engine import OracleEngine
from test_gpu_fuzz import _random_case
from jwas_jl_amd import streaming as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import jwas_jl_amd as J
    e = J.HipEngine(0)
    yield e
    e.close()


def _packed_dataset(n, p, seed, centered, missing, lane):
    """Genotype codes 0/1/2 (make_dataset's raw matrix), `missing` of them replaced by code 3, optionally one marker with a
    16-row lane missing entirely; per-marker means over the observed codes (of at least 40 generated rows, so that the one-
    and three-row matrices are not all zero after centring); the decoded Float32 matrix (decode_marker!) and a phenotype."""
    big = max(n, 40)
    d = make_dataset(n=big, p=p, ncausal=min(6, p), seed=seed, center=False)
    rng = np.random.default_rng([seed, 0x2B17])
    codes = d["raw"].astype(np.uint8)
    if missing > 0:
        codes[rng.random((big, p)) < missing] = 3
    if lane:
        l0 = 16 * int(rng.integers(0, (n + 15) // 16))
        codes[l0:l0 + 16, int(rng.integers(0, p))] = 3
    miss = codes == 3
    means = np.array([codes[~miss[:, j], j].mean(dtype=np.float32) if (~miss[:, j]).any() else np.float32(0.5)
                      for j in range(p)], dtype=np.float32)
    codes, miss = np.ascontiguousarray(codes[:n]), miss[:n]
    v = np.where(miss, means[None, :], codes.astype(np.float32)).astype(np.float32)
    X = np.asfortranarray((v - means[None, :]).astype(np.float32) if centered else v)
    y = d["y"][:n].astype(np.float32)
    y = (y - y.mean()).astype(np.float32) if n > 1 else y
    return codes, means, X, y


def _sweep_arguments(c, rng, y):
    """The sweep's variances and priors for configuration c (the constructions of test_random_configurations_against_the_oracle)."""
    method, t, p, sp = c["method"], c["t"], c["p"], c["sparsity"]
    v = np.float32(max(float(np.var(y)), 0.1))
    g = np.float32(0.02)
    A = rng.standard_normal((t, t)); Rm = ((A @ A.T / t + np.eye(t)) * v).astype(np.float32)
    Bm = rng.standard_normal((t, t)); Gm = ((Bm @ Bm.T / t + np.eye(t)) * g).astype(np.float32)
    if method == "BayesC":
        kw = dict(vare=v, var_effect=g, pi=sp)
        if c["marker_prior"]:
            kw = dict(vare=v, var_effect=g, pi_vec=np.clip(sp + rng.uniform(-0.2, 0.2, p), 0.0, 0.999))
    elif method == "BayesB":
        kw = dict(vare=v, var_effect=g, var_effect_vec=rng.uniform(0.005, 0.04, p).astype(np.float32), pi=sp)
    elif method == "BayesR":
        rest = np.array([0.5, 0.3, 0.2]) * (1 - sp)
        kw = dict(vare=v, var_effect=np.float32(0.1), pi_classes=np.concatenate([[sp], rest]))
        if c["marker_prior"]:
            pm = rng.dirichlet(np.ones(4), size=p) * 0.5 + 0.5 * kw["pi_classes"]
            kw["pi_matrix"] = pm / pm.sum(axis=1, keepdims=True)
    elif method == "MegaBayesC":
        kw = dict(vare=np.diag(np.diag(Rm)), var_effect=np.diag(np.diag(Gm)), pi=np.full(t, sp))
    elif method == "MegaBayesB":
        Vm = np.zeros((p, t, t), dtype=np.float32)
        for k in range(t):
            Vm[:, k, k] = g * np.exp(rng.uniform(-1, 1, p))
        kw = dict(vare=np.diag(np.diag(Rm)), var_effect=np.eye(t, dtype=np.float32), pi=np.full(t, sp), var_effect_matrix=Vm)
    else:
        prior = np.full(1 << t, (1 - sp) / ((1 << t) - 1)); prior[0] = sp
        if sp == 0.0:
            prior = np.full(1 << t, 1e-3); prior[-1] = 1.0
        prior /= prior.sum()
        kw = dict(vare=Rm, var_effect=Gm, log_prior_states=np.log(prior))
        if method in ("MTBayesB", "MTBayesB_II"):
            Wm = rng.standard_normal((p, t, t))
            kw["var_effect_matrix"] = ((Wm @ Wm.transpose(0, 2, 1) / t + np.eye(t)) * (g * np.exp(rng.uniform(-1, 1, p)))[:, None, None]).astype(np.float32)
    if c["indep"]:
        kw["independent_blocks"] = True
    return kw


def _case(method="BayesC", t=1, n=530, p=150, part=("uniform", 64), nreps=1, sparsity=0.9, seed=1, weights=False, indep=False,
          marker_prior=False, centered=True, missing=0.02, lane=False):
    return dict(method=method, t=t, n=n, p=p, part=part, nreps=nreps, sparsity=sparsity, seed=seed, weights=weights, indep=indep,
                marker_prior=marker_prior, centered=centered, missing=missing, lane=lane)


def _assert_bit_equal(hip, c, min_row_groups=1):
    """Runs configuration c on the packed device context and on the oracle in the device's order: equal in every bit."""
    import oracle as O
    rng = np.random.default_rng(c["seed"])
    method, t, n, p = c["method"], c["t"], c["n"], c["p"]
    codes, means, X, y = _packed_dataset(n, p, c["seed"] % 1000, c["centered"], c["missing"], c["lane"])
    w = rng.uniform(0.3, 3.0, n).astype(np.float32) if c["weights"] else None
    hip.load_packed2bit(S.pack_2bit(codes), n, means, centered=c["centered"]); hip.set_weights(w)
    assert hip.storage_info()["kind"] == "packed2bit"
    spg, nrg, _ = hip.update_geometry()
    assert nrg >= min_row_groups, (spg, nrg)
    O.set_device_order(spg)
    orc = OracleEngine("lookahead", acc=O.ACC_DEVICE)
    orc.load_dense(X); orc.set_weights(w)
    try:
        for e in (orc, hip):
            if c["part"][0] == "explicit":
                e.setup_blocks_explicit(c["part"][1], "f64")
            else:
                e.setup_blocks(c["part"][1], "f64")
        # the device takes the oracle's inner products (how they are summed is then no part of the comparison)
        hip.set_xpx(orc._xpx); hip.set_grams_packed(orc._grams)
        orc._w()
        st_ = list(orc._bs) + [p]
        for kb in range(1, len(st_) - 1):
            hip.set_cross_gram(kb, O.cross_gram(X, st_[kb - 1], st_[kb] - st_[kb - 1], st_[kb], st_[kb + 1] - st_[kb], O.ACC_DEVICE))
        O.set_weights(None)
        for e in (orc, hip):
            e.init_state(method, t)
            for k in range(t):
                e.set_residual(((1 + 0.3 * k) * y).astype(np.float32), k)
            if method == "BayesR":
                e.set_state(0, delta=np.ones(p, dtype=np.int32))
            elif t > 1:
                for k in range(t):
                    e.set_state(k, delta=np.ones(p, dtype=np.float32))
        kw = _sweep_arguments(c, rng, y)
        nreps = c["nreps"] if method not in ("MTBayesC_II", "MTBayesB_II") or c["nreps"] in (1, 2) else 1
        orc.set_packed_source(codes, means, centered=c["centered"])
        for it in range(1, 5):
            so = orc.sweep(iteration=it, seed=c["seed"], nreps=nreps, **kw)
            sh = hip.sweep(iteration=it, seed=c["seed"], nreps=nreps, **kw)
            assert so["n_events"] == sh["n_events"], f"{c} iteration {it}"
    finally:
        O.set_device_order(8)
        orc.set_packed_source(None, None)
    for k in range(t):
        ao, bo, do = orc.get_state(k)
        ah, bh, dh = hip.get_state(k)
        assert np.array_equal(do, dh), f"{c}"
        assert np.array_equal(ah, ao) and np.array_equal(bh, bo), f"{c}: max |d alpha| {np.abs(ah - ao).max()}"
        assert np.array_equal(hip.get_residual(k), orc.get_residual(k)), f"{c}"


# ---- (a) pinned edge cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,method", [
    (1, "BayesC"),              # a single row
    (3, "BayesC"),              # less than one byte of a column
    (15, "BayesC"),             # less than one lane's dword
    (16, "BayesC"), (17, "BayesC"),                                  # either side of the ragged-row mask's full lane
    (1023, "BayesC"), (1024, "BayesC"), (1025, "BayesC"), (1025, "BayesR"),     # either side of a 1024-row slice
    (2048, "BayesC"),           # two full slices
    (2300, "BayesC"),           # a ragged third slice
])
def test_edge_row_counts_equal_the_oracle_bit_for_bit(hip, n, method):
    _assert_bit_equal(hip, _case(method=method, n=n, p=150, part=("uniform", 64), sparsity=0.8, seed=400 + n, missing=0.02, lane=n >= 16))


def test_two_row_groups_at_the_default_geometry(hip):
    """n = 8200: nine 1024-row slices, more than the eight of one row group -- the sampler adds two partials per column."""
    _assert_bit_equal(hip, _case(n=8200, p=130, part=("uniform", 64), sparsity=0.8, seed=8200, missing=0.02, lane=True), min_row_groups=2)


def test_two_row_groups_of_four_slices(hip, monkeypatch):
    """n = 4100 with four slices per row group (JWAS_HIP_SPG is read at every matrix load): five slices, two row groups, the
    second one with a single active wave."""
    monkeypatch.setenv("JWAS_HIP_SPG", "4")
    _assert_bit_equal(hip, _case(n=4100, p=130, part=("uniform", 64), sparsity=0.8, seed=4100, missing=0.02, lane=True), min_row_groups=2)
    assert hip.update_geometry()[0] == 4


def test_fewer_markers_than_column_groups(hip):
    """p = 5: most column groups of the launch own no column (ncols = 0), the others one."""
    c = _case(n=300, p=5, part=("uniform", 64), sparsity=0.3, seed=55)
    _assert_bit_equal(hip, c)
    assert hip.update_geometry()[2] > 5


def test_dense_prior_block_of_512_markers(hip):
    """pi = 0 on 512-marker blocks: every marker changes in every sweep, so a block's change list is eight trips of the 64-entry
    apply loop and the dense single-trait sampler (dense_big_st) runs on packed columns."""
    _assert_bit_equal(hip, _case(n=300, p=600, part=("uniform", 512), sparsity=0.0, seed=512))
    assert hip.last_sweep_schedule() & (1 << 7)                          # JWAS_HIP_SCHED_DENSE_BIG


def test_block_of_1024_markers(hip, monkeypatch):
    """A 1024-marker block with more than 64 columns per column group: the second chunk of marker means (mnext) and of the LDS
    flush.  A short matrix gets 32 column groups (32 columns each) by default, and the geometries with fewer than 16 belong to
    matrices of > 100 000 rows: JWAS_HIP_MAX_NCG (read at every matrix load, like JWAS_HIP_SPG) caps them at 8 here."""
    monkeypatch.setenv("JWAS_HIP_MAX_NCG", "8")
    c = _case(n=300, p=1100, part=("uniform", 1024), sparsity=0.9, seed=1024)
    _assert_bit_equal(hip, c)
    assert -(-1024 // hip.update_geometry()[2]) > 64


@pytest.mark.parametrize("t", [3, 4])
def test_three_and_four_traits_sampler_one(hip, t):
    """NT = 3 and 4: the update role keeps fl32(w r) as float, not double."""
    _assert_bit_equal(hip, _case(method="MTBayesC", t=t, n=530, p=200, part=("uniform", 64), sparsity=0.9, seed=30 + t, weights=(t == 3)))


def test_uncentred_storage_with_weights(hip):
    """centered = false with residual weights: the branch fma(mu, sm, acc) on fl32(w r), a missing lane included."""
    _assert_bit_equal(hip, _case(n=530, p=200, part=("uniform", 64), sparsity=0.8, seed=77, weights=True, centered=False, missing=0.3, lane=True))


# ---- (b) a seeded sample of the configuration space -------------------------------------------------------------------------
def _random_packed_case(seed):
    """test_gpu_fuzz._random_case (shape, partition, sampler, prior sparsity, repetitions, weights, independent blocks,
    per-marker priors: the same draws and the same caps on block size for the oracle's patience) extended by the storage's own
    dimensions: centred or not, the fraction of missing codes, and now and then a marker with a fully missing 16-row lane."""
    c = _random_case(seed)
    rng = np.random.default_rng([int(seed), 0x9AC4ED])
    c["centered"] = bool(rng.random() < 0.6)
    c["missing"] = float(rng.choice([0.0, 0.02, 0.3]))
    c["lane"] = bool(rng.random() < 0.2)
    return c


_NCASES = max(150, int(os.environ.get("JWAS_FUZZ_CASES", "400")) * 3 // 8)     # (JWAS_FUZZ_CASES=6000 for a long run: 2250 cases)


@pytest.mark.parametrize("seed", list(range(_NCASES)))
def test_random_packed_configurations_against_the_oracle(hip, seed):
    """Differential fuzzing of the sweep on 2-bit packed storage: whatever the shape, partition, sampler (single-trait, multi-trait
    samplers I and II, constraint = true, per-marker covariances), prior, repetition count, residual weights, independent blocks,
    per-marker priors, centring and missing pattern, the device chain equals the oracle's BIT FOR BIT."""
    _assert_bit_equal(hip, _random_packed_case(5000 + seed))


# ---- grouped launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centered", [True, False])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("method", ["BayesC", "BayesB", "BayesR"])
@pytest.mark.parametrize("m", [2, 4])
def test_random_grouped_launches_on_packed_storage(hip, m, method, weights, centered):
    """Grouped launches (k_group_step<., PackedCols>) on random shapes, with and without residual weights, centred or not.  The
    grouped sweep is not bit-exact against the oracle's grouped restatement on dense storage either, so these are held to the bars
    of test_packed_grouped_launches_match_the_oracle: identical trajectories (indicators, the number of changes of every sweep),
    effects within 5e-6, residuals within 3e-5."""
    rng = np.random.default_rng([m, len(method), ord(method[-1]), weights, centered])
    bs = int(rng.choice([64, 128]))
    n = int(rng.integers(40, 700)) if rng.random() < 0.6 else int(rng.integers(1030, 2400))
    p = bs * int(rng.integers(m + 1, 2 * m + 3)) + int(rng.integers(1, bs))
    codes, means, X, y = _packed_dataset(n, p, int(rng.integers(0, 1000)), centered, float(rng.choice([0.0, 0.02, 0.3])), True)
    w = rng.uniform(0.3, 3.0, n).astype(np.float32) if weights else None
    hip.load_packed2bit(S.pack_2bit(codes), n, means, centered=centered); hip.set_weights(w)
    orc = OracleEngine("lookahead")
    orc.load_dense(X); orc.set_weights(w)
    for e in (hip, orc):
        e.setup_blocks(bs, "f64")
        e.setup_groups(m, "f64")
        e.init_state(method)
        e.set_residual(y)
    if method == "BayesR":
        for e in (hip, orc):
            e.set_state(0, delta=np.ones(p, dtype=np.int32))
    vare = np.float32(0.5 * y.var())
    varg = np.float32(0.5 * y.var() / (0.1 * 0.4 * p))
    if method == "BayesC":
        kw = dict(vare=vare, var_effect=varg, pi=0.9)
    elif method == "BayesB":
        kw = dict(vare=vare, var_effect=varg, var_effect_vec=np.full(p, varg, dtype=np.float32), pi=0.8)
    else:
        kw = dict(vare=vare, var_effect=np.float32(5 * varg), pi_classes=np.array([0.9, 0.05, 0.03, 0.02]))
    try:
        orc.set_packed_source(codes, means, centered=centered)
        for it in range(1, 7):
            sp = hip.sweep(iteration=it, seed=9, group_launch=True, **kw)
            so = orc.sweep(iteration=it, seed=9, group_launch=True, **kw)
            assert so["n_events"] == sp["n_events"], f"iteration {it} (n = {n}, p = {p}, block {bs})"
    finally:
        orc.set_packed_source(None, None)
    ap, _, dp = hip.get_state(0)
    ao, _, do = orc.get_state(0)
    assert np.array_equal(do, dp)
    np.testing.assert_allclose(ap, ao, rtol=0, atol=5e-6)
    np.testing.assert_allclose(hip.get_residual(0), orc.get_residual(0), rtol=0, atol=3e-5)
