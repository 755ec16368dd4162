"""The device's draws against their EXACT laws, computed in float64 from the inputs alone (tests/draw_laws.py) -- not against a
restatement on the same counters, which would share a wrong degrees-of-freedom, a transposed factor or K K' in the place of K' K:

A. k_sample_marker_covariances<2|3|4> (Float32, full and diagonal) and k64_sample_marker_covariances: Bartlett's theorem on the
   whitened draws and the inverse-free pivots, at the production df = t + 5, at df = t + 0.5 (the last row's chi-square takes the
   a < 1 boost branch exp(log u / a)) and, Float32, at df = t - 0.5.
B. k_mtmiss_impute: B e_o + z U has the law N(R_mo R_oo^-1 e_o, R_mm - R_mo R_oo^-1 R_om) for every pattern at t = 2, 3, 4.

tests/test_draw_laws_host.py runs the same checks with the same inputs and bounds on the oracle and the stand-in.  Every test
prints the statistic, the bound and N before it asserts.

Measured on an MI355X (the oracle / stand-in on the same inputs in brackets), N = 200 000, bounds KS 0.00602, correlation 0.01118:
    inverse-Wishart, df >= t + 0.5   KS D <= 0.00352 (0.00352)   correlation <= 0.00659 (0.00659)   excluded, Float32 df = t + 0.5: 5e-6 (5e-6)
    df = t - 0.5, unit-vector pivots KS D <= 0.00312 (0.00312)
    diagonal form                    KS D <= 0.00311 (0.00311)
    imputation, N = 14 000 a pattern KS D 0.57 of 0.02276 (0.57)   correlation 0.51 of 0.04226 (0.51)
What the checks catch, on the CPU twins: a chi-square with df + 1 gives a pivot D of 0.12 (t = 2, df = 7) and 0.25 (t = 3, df = 3.5);
U transposed in the imputation gives a correlation of 0.48 at t = 4 and 0.17 at t = 3 (at t = 2 U is 1 x 1: nothing to transpose)."""
import numpy as np
import pytest

import draw_laws as DL
from jwas_jl_amd import mcmc

pytestmark = pytest.mark.gpu


def _design(n, p, dtype):
    """Any n x p design will do (the draws read beta and the residuals only): a small matrix tiled."""
    rng = np.random.default_rng(5)
    small = rng.standard_normal((n, 64))
    small -= small.mean(axis=0)
    return np.asfortranarray(np.tile(small, (1, -(-p // 64)))[:, :p].astype(dtype))


def device_iw_draws(precision, t, df, method="MTBayesB"):
    import jwas_jl_amd as J
    dtype = np.float64 if precision == 64 else np.float32
    scale, beta = DL.iw_inputs(t)
    p = beta.shape[1]
    hip = J.HipEngine(0, precision=precision)
    try:
        hip.load_dense(_design(300, p, dtype)); hip.setup_blocks(64, "f64"); hip.init_state(method, t)
        for k in range(t):
            hip.set_state(k, alpha=beta[k].astype(dtype), beta=beta[k].astype(dtype), delta=np.ones(p, dtype=dtype))
        G = []
        for it in DL.IW_ITERATIONS:
            hip.sample_marker_covariances(df, scale, seed=DL.IW_SEED, iteration=it, marker_offset=DL.IW_MARKER0)
            G.append(hip.marker_covariances())
    finally:
        hip.close()
    G = np.concatenate(G)
    assert G.dtype == dtype and len(G) == 200_000
    return G, np.tile(DL.iw_psi(scale, beta), (len(DL.IW_ITERATIONS), 1, 1))


@pytest.mark.parametrize("t", [2, 3, 4])
@pytest.mark.parametrize("precision,ddf", [(32, 5.0), (32, 0.5), (32, -0.5), (64, 5.0), (64, 0.5)])
def test_marker_covariance_draws_follow_the_inverse_wishart_law(precision, t, ddf):
    """Float64 context and Float32 at df = t + 5: no draw may be left out.  Float32 at df = t + 0.5: a draw whose float32 G makes
    M^-1 indefinite may be left out of the Bartlett check only, at most 1e-4 of them (the oracle: <= 2e-5).  Float32 at
    df = t - 0.5: the pivots on the unit vectors only (condition numbers reach 1e16)."""
    df = t + ddf
    G, Psi = device_iw_draws(precision, t, df)
    DL.assert_iw_law(G, Psi, df, f"device f{precision}", bartlett=ddf > 0,
                     max_excluded=1e-4 if (precision == 32 and ddf == 0.5) else 0.0, unit_only=ddf < 0)


@pytest.mark.parametrize("t", [2, 3, 4])
@pytest.mark.parametrize("df", [5.0, 1.5, 0.6])
def test_diagonal_draws_follow_the_scaled_inverse_chi2_law(t, df):
    """constraint = true (MEGABAYESB, Float32 only): (scale_kk + b_k^2) / G_kk ~ chi2(df), off-diagonals exactly 0."""
    G, Psi = device_iw_draws(32, t, df, method="MegaBayesB")
    DL.assert_diagonal_law(G, Psi, df, "device f32")


@pytest.mark.parametrize("t", [4, 3, 2])
@pytest.mark.parametrize("precision", [64, 32])
def test_imputation_follows_the_conditional_normal(precision, t):
    """Every pattern (14, 6, 2 incomplete ones), 14 000 records each, shuffled: observed cells and complete records bit-unchanged,
    the whitened missing cells N(0, I) and uncorrelated with the observed ones -- the mean and S from R alone."""
    import jwas_jl_amd as J
    dtype = np.float64 if precision == 64 else np.float32
    R, codes, e = DL.mtmiss_inputs(t)
    n = len(codes)
    B, U, _ = mcmc.missing_pattern_tables(R)
    before = e.astype(dtype)
    hip = J.HipEngine(0, precision=precision)
    try:
        hip.load_dense(_design(n, 64, dtype)); hip.setup_blocks(64, "f64"); hip.init_state("MTBayesC", t)
        for k in range(t):
            hip.set_residual(before[k], k)
        hip.mtmiss_begin(codes)
        hip.mtmiss_impute(iteration=DL.MT_ITERATION, seed=DL.MT_SEED, B=B, U=U)
        after = np.stack([hip.get_residual(k) for k in range(t)])
    finally:
        hip.close()
    assert after.dtype == dtype
    DL.assert_imputation_law(R, codes, before, after, f"device f{precision}")
