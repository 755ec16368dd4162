"""Several genotype categories on the device: the residual hand-over between two contexts (jwas_hip_residual_handover), the
two-context chain against the oracle's, runMCMC end to end against its stand-in run, and the law of the chain against the
enumerated posterior (tests/multigeno_reference.py)."""
import numpy as np
import pandas as pd
import pytest

import draw_laws as DL
import multigeno_reference as MR
from conftest import make_dataset
from multigeno_reference import MultiOracleEngine, MultiOracleEngine64
from jwas_jl_amd import api
from jwas_jl_amd import streaming as S

pytestmark = pytest.mark.gpu

N, P1, P2, BS = 301, 70, 50, 32            # n = 301: a ragged second 256-row slice
LAW_SWEEPS = 10_000                        # (30 000 sweeps took 11.8 s on the device, more than a test may take; the CPU twin shows the SE bound holds at 10 000)


def _engine(precision=32):
    import jwas_jl_amd as J
    return J.HipEngine(0, precision=precision)


def _data(seed=5):
    d = make_dataset(n=N, p=P1 + P2, ncausal=8, seed=seed, center=False)
    return d, d["y"] - d["y"].mean()


# ---- 1. the hand-over ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("t", [1, 3])
def test_residual_handover_copies_every_trait_and_keeps_the_pad_rows(t, precision):
    dtype = np.float64 if precision == 64 else np.float32
    d, y = _data()
    X = (d["raw"] - d["means"]).astype(dtype)
    rng = np.random.default_rng(t)
    src, dst = _engine(precision), _engine(precision)
    try:
        method = "BayesC" if t == 1 else "MTBayesC"
        for e, Xe in ((src, X[:, :P1]), (dst, X[:, P1:])):
            e.load_dense(np.asfortranarray(Xe))
            e.setup_blocks(64, "f64")
            e.init_state(method, t)
            for k in range(t):
                e.set_state(k, delta=np.ones(e.p, dtype=dtype))
        R = np.stack([(y * (1 + 0.5 * k) + 0.1 * rng.standard_normal(N)).astype(dtype) for k in range(t)])
        for k in range(t):
            src.set_residual(R[k], k)
            dst.set_residual(rng.standard_normal(N).astype(dtype), k)
        dst.residual_handover(src)
        for k in range(t):
            assert np.array_equal(dst.get_residual(k), R[k])
            assert np.array_equal(src.get_residual(k), R[k])
        for k in range(t):                      # a copy, not an alias
            src.set_residual(np.zeros(N, dtype=dtype), k)
        for k in range(t):
            assert np.array_equal(dst.get_residual(k), R[k])
        dst.residual_handover(dst)              # dst is src: nothing happens
        assert np.array_equal(dst.get_residual(0), R[0])
        vare = np.float32(0.5) if t == 1 else (0.5 * np.eye(t) + 0.1).astype(np.float32)
        varg = np.float32(0.02) if t == 1 else (0.02 * np.eye(t) + 0.005).astype(np.float32)
        kw = dict(pi=0.7) if t == 1 else dict(log_prior_states=np.log(np.full(1 << t, 1.0 / (1 << t))))
        st = dst.sweep(iteration=1, seed=3, vare=vare, var_effect=varg, marker_offset=P1, **kw)
        after = np.stack([dst.get_residual(k) for k in range(t)]).astype(np.float64)
        want = after @ after.T                  # over the n rows only: pad rows that were not zero would show here
        print(f"hand-over t{t} f{precision}: resid_ss relative difference {np.abs(st['resid_ss'] / want - 1).max():.2e} (bound 1e-6)")
        np.testing.assert_allclose(st["resid_ss"], want, rtol=1e-6)
        assert not np.array_equal(after, R.astype(np.float64))
    finally:
        src.close(); dst.close()


def test_residual_handover_errors():
    import jwas_jl_amd as J
    d, y = _data()
    X = np.asfortranarray((d["raw"] - d["means"]).astype(np.float32))

    def ready(Xe, t=1, precision=32):
        e = _engine(precision)
        e.load_dense(np.asfortranarray(Xe.astype(e.dtype)))
        e.setup_blocks(64, "f64")
        e.init_state("BayesC" if t == 1 else "MTBayesC", t)
        return e
    engines = []
    try:
        dst = ready(X[:, :P1]); engines.append(dst)
        dst.set_residual(y)
        cases = {"n": ready(X[:300, P1:]), "ntraits": ready(X[:, P1:], t=2), "precision": ready(X[:, P1:], precision=64)}
        engines += list(cases.values())
        for what, src in cases.items():
            for a, b in ((dst, src), (src, dst)):
                with pytest.raises(J.JwasHipError) as ei:
                    a.residual_handover(b)
                assert ei.value.code == -1, what                 # JWAS_HIP_EINVAL
        empty = _engine(); engines.append(empty)
        loaded = _engine(); engines.append(loaded)
        loaded.load_dense(X[:, P1:])
        loaded.setup_blocks(64, "f64")                       # genotypes, no init_state
        for src in (empty, loaded):
            for a, b in ((dst, src), (src, dst)):
                with pytest.raises(J.JwasHipError) as ei:
                    a.residual_handover(b)
                assert ei.value.code == -3                   # JWAS_HIP_ESTATE
        assert np.array_equal(dst.get_residual(), y)         # no refused call wrote anything
    finally:
        for e in engines:
            e.close()


# ---- 2. the two-context chain against the oracle's -----------------------------------------------------------------------------------
KW1 = dict(vare=np.float32(0.5), var_effect=np.float32(0.02), pi=0.7)
KW2 = dict(vare=np.float32(0.5), var_effect=np.float32(0.2), pi_classes=np.array([0.6, 0.2, 0.15, 0.05]))


@pytest.mark.parametrize("variant", ["dense", "packed", "f64"])
def test_two_context_chain_matches_the_oracle_chain(variant):
    """Category 1 BayesC, category 2 BayesR, 5 sweeps, fixed hyper-parameters, offsets as the driver sets them; indicators and
    classes equal, effects within 5e-6, the residual within 2e-5 (tests/test_gpu_parity.py's rule).  packed: category 1 is 2-bit
    packed storage and its oracle forms the block right-hand sides in the packed order."""
    f64 = variant == "f64"
    dtype = np.float64 if f64 else np.float32
    d, y = _data()
    raw = d["raw"].astype(np.float64)
    means = raw.mean(axis=0, dtype=np.float32).astype(np.float32)
    X = np.asfortranarray((raw.astype(np.float32) - means[None, :]).astype(dtype))
    codes = raw[:, :P1].astype(np.uint8)
    hips = [_engine(64 if f64 else 32), _engine(64 if f64 else 32)]
    orcs = [MultiOracleEngine64(), MultiOracleEngine64()] if f64 else [MultiOracleEngine("lookahead"), MultiOracleEngine("lookahead")]
    try:
        for pair in (hips, orcs):
            for e, Xe, method in ((pair[0], X[:, :P1], "BayesC"), (pair[1], X[:, P1:], "BayesR")):
                if variant == "packed" and e is hips[0]:
                    e.load_packed2bit(S.pack_2bit(codes), N, means[:P1], centered=True)
                else:
                    e.load_dense(np.asfortranarray(Xe))
                if f64:
                    e.setup_blocks(BS, "f64")
                else:                                        # (a Float32 context runs blocks of 32 as an explicit partition)
                    e.setup_blocks_explicit(np.arange(0, e.p, BS, dtype=np.int64), "f64")
                e.init_state(method)
                e.set_state(delta=np.ones(e.p, dtype=np.int32 if method == "BayesR" else dtype))
            pair[0].set_residual(y.astype(dtype))
        for it in range(1, 6):
            for pair in (hips, orcs):
                if it > 1:
                    pair[0].residual_handover(pair[1])
                if variant == "packed" and pair is orcs:
                    pair[0].set_packed_source(codes, means[:P1], centered=True)
                try:
                    s1 = pair[0].sweep(iteration=it, seed=3, marker_offset=0, **KW1)
                finally:
                    if variant == "packed" and pair is orcs:
                        pair[0].set_packed_source(None, None)
                pair[1].residual_handover(pair[0])
                s2 = pair[1].sweep(iteration=it, seed=3, marker_offset=P1, **KW2)
                if pair is hips:
                    sh = (s1, s2)
                else:
                    assert s1["n_events"] == sh[0]["n_events"] and s2["n_events"] == sh[1]["n_events"], f"iteration {it}"
        for hip, orc in zip(hips, orcs):
            ah, _, dh = hip.get_state()
            ao, _, do = orc.get_state()
            assert np.any(ao != 0)
            assert np.array_equal(dh, do)
            np.testing.assert_allclose(ah, ao, rtol=0, atol=5e-6)
        np.testing.assert_allclose(hips[1].get_residual(), orcs[1].get_residual(), rtol=0, atol=2e-5)
    finally:
        for e in hips:
            e.close()


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------
def test_runmcmc_mixed_model_gpu_matches_its_stand_in_run(tmp_path):
    """BayesB + RR-BLUP with a covariate, 60 iterations: one HipEngine per category (the default) against the same host loop on the
    oracle's engines, compared as tests/test_gpu_e2e.py compares a single-category run."""
    from test_gpu_e2e import _setup
    from test_multigeno_host import mixed_model
    gdf, ph, d = _setup("BayesB", 0.9)
    cols = list(gdf.columns[1:])
    g1, g2 = gdf[["ID"] + cols[:800]], gdf[["ID"] + cols[800:]]
    ph = ph.assign(x1=np.random.default_rng(3).standard_normal(len(ph)))
    outs = {}
    for tag, eng in (("orc", [MultiOracleEngine("lookahead"), MultiOracleEngine("lookahead")]), ("hip", None)):
        outs[tag] = api.runMCMC(mixed_model(g1, g2), ph, chain_length=60, burnin=10, seed=2026, output_folder=str(tmp_path / tag),
                                _engine=eng, block_size=256, gram_mode="f64")
    for name in ("geno1", "geno2"):
        eo, eh = outs["orc"][f"marker effects {name}"], outs["hip"][f"marker effects {name}"]
        assert np.any(eo["Estimate"] != 0)
        np.testing.assert_allclose(eh["Estimate"], eo["Estimate"], atol=1e-4)
        np.testing.assert_allclose(eh["Model_Frequency"], eo["Model_Frequency"], atol=1e-4)
        np.testing.assert_allclose(eh["SD"], eo["SD"], atol=1e-4)
    assert float(outs["hip"]["residual variance"]["Estimate"][0]) == pytest.approx(
        float(outs["orc"]["residual variance"]["Estimate"][0]), rel=1e-4)
    np.testing.assert_allclose(outs["hip"]["EBV_y1"]["EBV"], outs["orc"]["EBV_y1"]["EBV"], atol=1e-3)
    assert float(outs["hip"]["pi_geno1"]["Estimate"][0]) == pytest.approx(float(outs["orc"]["pi_geno1"]["Estimate"][0]), abs=1e-4)


# ---- 4. the law on the device ----------------------------------------------------------------------------------------------------------
def test_two_category_chain_on_the_device_has_the_enumerated_law():
    """tests/test_multigeno_host.py's law test on two HipEngines, same acceptance (its CPU twin shows the standard errors within
    their bound at 10 000 and at 30 000 sweeps)."""
    import time
    case = MR.two_category_case()
    exact, Ea, Eaa = MR.exact_marker_mixture_moments(np.hstack([case["X1"], case["X2"]]), case["y"], case["vare"], case["class_vars"],
                                                     case["class_probs"])
    e1, e2 = _engine(), _engine()
    try:
        t0 = time.perf_counter()
        counts, alphas = MR.run_two_category_chain(e1, e2, case, LAW_SWEEPS, DL.CHAIN_BURN)
        secs = time.perf_counter() - t0
    finally:
        e1.close(); e2.close()
    m = MR.chain_figures(counts, alphas, exact, Ea, Eaa)
    print(f"two-category law on the device: {LAW_SWEEPS} sweeps in {secs:.1f} s; worst state frequency difference {m['freq']:.4f} "
          f"(bound 0.02), means within {m['dev1']:.2f} SE, second moments within {m['dev2']:.2f} SE (bound 5), worst SE "
          f"{m['se_sd']:.4f} of the posterior sd (bound 0.02)")
    assert MR.figures_pass(m), m
