"""CPU twins of tests/test_gpu_draw_laws.py and of the effect-moment checks of tests/test_gpu_statistical.py: the same helpers
(tests/draw_laws.py), the same inputs and the same bounds on the draws of the C oracle and the numpy stand-ins.  They make "the
reference alone stays within the bound" an executed statement, and test the helpers where there is no GPU.  Every test prints the
statistic, the bound and N before it asserts."""
import numpy as np
import pytest

import draw_laws as DL
import oracle as O
from jwas_jl_amd import mcmc
from mtmiss_reference import impute
from oracle_engine import OracleEngine


def oracle_iw_draws(t, df, diagonal=False):
    scale, beta = DL.iw_inputs(t)
    G = np.concatenate([O.sample_marker_covariances(beta, df, scale, DL.IW_SEED, it, DL.IW_MARKER0, diagonal=diagonal)
                        for it in DL.IW_ITERATIONS])
    Psi = np.tile(DL.iw_psi(scale, beta), (len(DL.IW_ITERATIONS), 1, 1))
    return G, Psi


def test_bounds():
    assert abs(DL.ks_bound(200_000) - 0.00602) < 5e-6 and abs(DL.corr_bound(200_000) - 0.01118) < 5e-6
    rng = np.random.default_rng(1)
    x = rng.standard_normal(50_000)
    assert DL.ks_stat(x, DL.norm_cdf) <= DL.ks_bound(50_000) < DL.ks_stat(1.1 * x, DL.norm_cdf)      # (sd off by 10 %: D ~ 0.023)
    assert DL.ks_stat(rng.chisquare(2.5, 50_000), DL.chi2_cdf(2.5)) <= DL.ks_bound(50_000)


@pytest.mark.parametrize("t", [2, 3, 4])
@pytest.mark.parametrize("ddf", [5.0, 0.5, -0.5])
def test_oracle_marker_covariance_draws_follow_the_inverse_wishart_law(t, ddf):
    """orc_sample_marker_covariances (the Float32 device path's restatement): df = t + 5 (production), t + 0.5 (the last row's
    chi-square takes the a < 1 boost branch), t - 0.5 (inverse-free pivots on the unit vectors only: the float32 G is too
    ill-conditioned to invert)."""
    df = t + ddf
    G, Psi = oracle_iw_draws(t, df)
    assert len(G) == 200_000
    DL.assert_iw_law(G, Psi, df, "oracle f32", bartlett=ddf > 0, max_excluded=1e-4 if ddf == 0.5 else 0.0, unit_only=ddf < 0)


@pytest.mark.parametrize("t", [2, 3, 4])
@pytest.mark.parametrize("df", [5.0, 1.5, 0.6])
def test_oracle_diagonal_draws_follow_the_scaled_inverse_chi2_law(t, df):
    G, Psi = oracle_iw_draws(t, df, diagonal=True)
    DL.assert_diagonal_law(G, Psi, df, "oracle f32")


@pytest.mark.parametrize("t", [4, 3, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_standin_imputation_follows_the_conditional_normal(t, dtype):
    R, codes, e = DL.mtmiss_inputs(t)
    B, U, _ = mcmc.missing_pattern_tables(R)
    before = e.astype(dtype)
    after = impute(before, codes, B, U, iteration=DL.MT_ITERATION, seed=DL.MT_SEED)
    assert after.dtype == dtype
    DL.assert_imputation_law(R, codes, before, after, f"stand-in {np.dtype(dtype).name}")


# ---- the effects of the exact-posterior chains (the twins of tests/test_gpu_statistical.py) ---------------------------------------
def test_the_two_enumerations_agree_on_independent_traits():
    """constraint = true is two independent single-trait problems: the Kronecker enumeration must give what the single-trait
    enumeration gives trait by trait, and no covariance between the traits."""
    case = DL.mt_chain_case("MegaBayesC")
    P, Ea, Eaa = DL.exact_mixture_moments_mt(case["X"], case["Y"], case["R"], case["G"], case["prior"])
    p = case["X"].shape[1]
    pi = case["kw"]["pi"]
    for k in range(2):
        _, ea, eaa = DL.exact_mixture_moments(case["X"], case["Y"][k], case["R"][k, k], [0.0, case["G"][k, k]], [pi[k], 1 - pi[k]])
        np.testing.assert_allclose(Ea[k * p:(k + 1) * p], ea, rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(Eaa[k * p:(k + 1) * p, k * p:(k + 1) * p], eaa, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(Eaa[:p, p:], np.outer(Ea[:p], Ea[p:]), rtol=1e-10, atol=1e-14)
    assert abs(sum(P.values()) - 1) < 1e-12


@pytest.mark.parametrize("method,precision", [("BayesC", 32), ("BayesR", 32), ("BayesC", 64)])
def test_oracle_chain_samples_the_exact_posterior(method, precision):
    if precision == 64:
        from oracle_engine import OracleEngine64
        DL.assert_st_chain(OracleEngine64(), DL.st_chain_case(method), f"oracle f64 {method}", np.float64)
    else:
        DL.assert_st_chain(OracleEngine("lookahead"), DL.st_chain_case(method), f"oracle f32 {method}")


@pytest.mark.parametrize("kind,precision", [("MTBayesC", 32), ("MTBayesC_II", 32), ("MegaBayesC", 32), ("MTBayesB", 32), ("MTBayesC", 64)])
def test_oracle_multitrait_chain_samples_the_exact_posterior(kind, precision):
    if precision == 64:
        from oracle_engine import OracleEngine64
        DL.assert_mt_chain(OracleEngine64(), DL.mt_chain_case(kind), f"oracle f64 {kind}", np.float64)
    else:
        DL.assert_mt_chain(OracleEngine("lookahead"), DL.mt_chain_case(kind), f"oracle f32 {kind}")


def test_float64_restatement_draws_follow_the_inverse_wishart_law():
    """tests/f64_mt_reference.sample_marker_covariances (the Float64 context's restatement, pure Python: 4 000 draws here, the bounds
    follow N) at df = t + 0.5.  At the full 200 000 draws the Float64 device draws are the oracle's to float32 rounding
    (tests/test_gpu_f64_multitrait.py), so the oracle twin above speaks for them."""
    from f64_mt_reference import sample_marker_covariances
    t, df = 3, 3.5
    scale, beta = DL.iw_inputs(t, 2000)
    G = np.concatenate([sample_marker_covariances(beta.astype(np.float64), df, scale, DL.IW_SEED, it, DL.IW_MARKER0) for it in (1, 2)])
    DL.assert_iw_law(G, np.tile(DL.iw_psi(scale, beta), (2, 1, 1)), df, "restatement f64")
