"""Annotation priors on the device (csrc/annot.hpp) through the C ABI and runMCMC, against the numpy restatement of
tests/annot_reference.py on the same Philox counters and in the same order of every sum.

STEP BY STEP the device and the restatement start from one common state: delta is set on both, and the device's session is opened
anew with the stand-in's coefficients before every call.  mu is the same IEEE operations on the same doubles.  What differs is the
libm: erfc / erfcinv on the device against ndtr / ndtri in the restatement, and log / cos in Box-Muller.  With u = 2^-53:

  the draw.  Both solve S(x) = q, q = S(L) - v S(L), L = -/+ mu the standardised bound (never mirrored twice: the other bound is
  infinite).  S(L) carries a few ulp of erfc and the rounding of its argument L / sqrt 2, which erfc turns into a relative error
  (1 + L^2) u; the subtraction rounds at the size of S(L), not of q, so q carries an ABSOLUTE error rho S(L) however small it is;
  the quantile turns an absolute error of q into that over phi(x); the inverse function adds a few ulp of x:
      |d e_i| <= E_i = ((16 + 4 (1 + L_i^2)) S(L_i) / phi(x_i) + 16 |x_i|) u
  (tests/liability_reference.truncated_std_normal_mp, the 50-digit replay of the same formula, puts the restatement itself at
  at most 0.18 of this bound on the BayesC inputs below (every third marker replayed): the cancellation in q is what dominates for draws far above L.)
  the liability: |d l_i| <= E_i + 2 u (|mu_i| + |e_i|)

  coefficient k (the sums run in ONE order on both sides, so only d e propagates; the n_A term is the allowance of
  tests/test_gpu_locpar.py for a sum of n_A doubles with n_A in place of n_l):
      |d c_k| <= C_k = inv_k (sum_A |D_ik| E_i^(k) + 2 (n_A + 4) u A_k) + 16 u (|mean_k| + sd_k) + 2^-46 sd_k
      A_k = sum_A |D_ik e_i| + |d_k c_k|,  sd_k = sqrt(inv_k),  mean_k = inv_k (S_k + d_k c_k)
      E_i^(k+1) = E_i^(k) + |D_ik| C_k + 2 u (|e_i| + |D_ik (c_k - c_k')|)
  (2^-46 sd: Box-Muller -- the angle 2 pi u2 carries one rounding, which the cosine passes on as an absolute error and the radius
  (<= 8.5) multiplies, plus a few ulp of log, sqrt and cos.)

  mu after the step: |d mu_i| <= sum_k |D_ik| C_k + 2 K u sum_k |D_ik c_k|
  P_s = clip(Phi(mu)): |d P| <= phi(mu) |d mu| + 8 u P;   1 - P the same + u
  a row entry is a product of up to three such factors f: |d row| <= sum_f (d f prod of the others) + 4 u row;
  the tree's logs: |d log row| <= d row / row + 4 u |log row|.

Every test prints the worst ratio (measured difference / bound) before it asserts ratio <= 1."""
import contextlib
import functools
import io

import numpy as np
import pandas as pd
import pytest
from scipy.special import ndtr

import annot_reference as R
from annot_reference import AnnotOracleEngine, AnnotOracleEngine64

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EPS = 2.0 ** -52
EINVAL, ESTATE, EUNSUP = -1, -3, -4
METHOD = {"BayesC": ("BayesC", 1), "BayesR": ("BayesR", 1), "tree": ("MTBayesC", 2)}


@functools.lru_cache(maxsize=None)
def _genotypes(p, precision):
    rng = np.random.default_rng(p)
    return np.asfortranarray(rng.integers(0, 3, (24, p)).astype(np.float64 if precision == 64 else np.float32))


def _design(p, ncols, seed=5):
    rng = np.random.default_rng(seed + ncols)
    A = rng.standard_normal((p, max(ncols - 1, 0)))
    if ncols > 1:
        A[:, 0] = (rng.random(p) < 0.3).astype(np.float64)          # a 0 / 1 annotation
    return np.hstack([np.ones((p, 1)), A])


def _delta(kind, p, rng):
    if kind == "BayesR":
        return [rng.choice([1, 2, 3, 4], p, p=[0.5, 0.25, 0.15, 0.1]).astype(np.int32)]
    if kind == "BayesC":
        return [(rng.random(p) < 0.3).astype(np.float64)]
    return [(rng.random(p) < 0.4).astype(np.float64), (rng.random(p) < 0.3).astype(np.float64)]


def _engines(kind, precision, p):
    import jwas_jl_amd as J
    X = _genotypes(p, precision)
    hip = J.HipEngine(0, precision=precision)
    ref = AnnotOracleEngine64() if precision == 64 else AnnotOracleEngine("block")
    for e in (hip, ref):
        e.load_dense(X)
        e.setup_blocks(64, "f64")
        e.init_state(*METHOD[kind])
    return hip, ref


def _start_prior(kind, p):
    if kind == "BayesC":
        return np.full(p, 0.7)
    row = np.array([0.7, 0.15, 0.1, 0.05])
    return np.tile(np.log(row) if kind == "tree" else row, (p, 1))


def _set_delta(engines, deltas):
    for e in engines:
        for k, d in enumerate(deltas):
            e.set_state(k, delta=d)


def _amplification(L, x):
    """S(L) / phi(x): what an error of q = S(L) (1 - v) relative to S(L) becomes in x."""
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        return ndtr(-L) / (np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi))


def _step_bounds(D, det, var, new_coef):
    """(liability bound per marker, coefficient bounds) of one step from the restatement's detail record."""
    p, K = D.shape
    act, z, mu, e0 = det["act"], det["z"], det["mu_in"], det["e0"]
    sgn = np.where(z, 1.0, -1.0)
    L, x = -sgn * mu, sgn * e0
    E = np.where(act, ((16 + 4 * (1 + L * L)) * _amplification(L, x) + 16 * np.abs(x)) * U, 0.0)
    liab_b = E + 2 * U * (np.abs(mu) + np.abs(e0))
    C = np.zeros(K)
    nA = det["n_active"]
    if nA == 0:
        return liab_b, C
    e = e0.copy()
    for k in range(K):
        xk = np.ones(p) if k == 0 else D[:, k]
        if k > 0:
            xp = np.ones(p) if k == 1 else D[:, k - 1]
            dck = det["old"][k - 1] - new_coef[k - 1]
            E = np.where(act, E + np.abs(xp) * C[k - 1] + 2 * U * (np.abs(e) + np.abs(xp * dck)), 0.0)
            e = np.where(act, e + xp * dck, 0.0)
        inv, d, S = det["inv"][k], det["d"][k], det["S"][k]
        A = float(np.abs(xk * e)[act].sum()) + abs(d * det["old"][k])
        mean, sd = inv * (S + d * det["old"][k]), np.sqrt(inv)
        C[k] = inv * (float((np.abs(xk) * E)[act].sum()) + 2 * (nA + 4) * U * A) + 16 * U * (abs(mean) + sd) + 2.0 ** -46 * sd
    return liab_b, C


def _table_bounds(kind, D, coef, Cb):
    """coef, Cb: (nsteps, K).  Bound of every entry of the table (the shape of the table)."""
    ns, K = coef.shape
    dP, P = [], []
    for s in range(ns):
        mu = R.mu_of(D, coef[s])
        dmu = np.abs(D) @ Cb[s] + 2 * K * U * (np.abs(D) @ np.abs(coef[s]))
        ps = R.phi(mu)
        dP.append(np.exp(-0.5 * mu * mu) / np.sqrt(2 * np.pi) * dmu + 8 * U * ps)
        P.append(np.clip(ps, EPS, 1 - EPS))
    if kind == "BayesC":
        return dP[0] + U
    p1, p2, p3 = P
    d1, d2, d3 = dP
    q1, q2, q3 = 1 - p1, 1 - p2, 1 - p3
    e1, e2, e3 = d1 + U, d2 + U, d3 + U                       # the bounds of 1 - P

    def prod(*fs):
        """fs: (value, bound) factors."""
        vals = [f[0] for f in fs]
        tot = np.prod(vals, axis=0)
        b = 4 * U * tot
        for i, (v, dv) in enumerate(fs):
            b = b + dv * np.prod([vals[j] for j in range(len(fs)) if j != i] or [1.0], axis=0)
        return tot, b

    if kind == "BayesR":
        rows = [prod((q1, e1)), prod((p1, d1), (q2, e2)), prod((p1, d1), (p2, d2), (q3, e3)), prod((p1, d1), (p2, d2), (p3, d3))]
        return np.stack([b for _, b in rows], axis=1)
    rows = [prod((q1, e1)), prod((p1, d1), (q2, e2), (p3, d3)), prod((p1, d1), (q2, e2), (q3, e3)), prod((p1, d1), (p2, d2))]
    return np.stack([b / v + 4 * U * np.abs(np.log(v)) for v, b in rows], axis=1)


# p = 263 229: 258 pieces of 1024 markers, so annot_ordered_sum's threads 0 and 1 take a second trip over the pieces
@pytest.mark.parametrize("p,precision,kind", [(p, prec, kind) for kind in ("BayesC", "BayesR", "tree") for prec in (32, 64) for p in (1003, 2085)]
                         + [(263_229, 64, kind) for kind in ("BayesC", "BayesR", "tree")])
def test_step_parity_from_a_common_state(kind, precision, p):
    hip, ref = _engines(kind, precision, p)
    ns = 1 if kind == "BayesC" else 3
    worst = {"liability": 0.0, "mu": 0.0, "coefficients": 0.0, "table": 0.0}
    try:
        for ncols in (1, 2, 9):
            D = _design(p, ncols)
            rng = np.random.default_rng(100 * ncols + p)
            coef0 = (rng.standard_normal((ncols, ns)) * 0.4) if ns > 1 else rng.standard_normal(ncols) * 0.4
            ref.annot_begin(kind, D, coef0, 1.0, _start_prior(kind, p))
            for it in (1, 2, 3):
                deltas = _delta(kind, p, rng)
                _set_delta((hip, ref), deltas)
                var = rng.uniform(0.5, 2.0, ns) if ns > 1 else float(rng.uniform(0.5, 2.0))
                cf_before = ref._an["coef"].copy()                           # (nsteps, K)
                liab_before = ref._an["liab"].copy()
                hip.annot_begin(kind, D, cf_before.T if ns > 1 else cf_before[0], 1.0, _start_prior(kind, p))
                details = []
                rr = ref.annot_step(iteration=it, seed=21, variance=var, details=details)
                rh = hip.annot_step(iteration=it, seed=21, variance=var)
                assert np.array_equal(rh["n_active"], rr["n_active"])
                cf_ref = ref._an["coef"]
                Cb = np.zeros((ns, ncols))
                lh = hip.annot_liability().reshape(p, -1)
                for s in range(ns):
                    det = details[s]
                    lb, Cb[s] = _step_bounds(D, det, float(np.broadcast_to(var, (ns,))[s]), cf_ref[s])
                    act = det["act"]
                    if det["n_active"]:
                        got, want = lh[act, s], ref._an["liab"][s][act]
                        assert np.all(np.isfinite(got)) and np.all(np.where(det["z"][act], got >= 0, got <= 0))
                        worst["liability"] = max(worst["liability"], float(np.max(np.abs(got - want) / lb[act])))
                        ch = rh["coefficients"].reshape(ncols, -1)[:, s]
                        worst["coefficients"] = max(worst["coefficients"], float(np.max(np.abs(ch - cf_ref[s]) / Cb[s])))
                    else:
                        assert np.array_equal(rh["coefficients"].reshape(ncols, -1)[:, s], cf_before[s])
                    assert np.array_equal(ref._an["liab"][s][~act], liab_before[s][~act])
                    assert not lh[~act, s].any()                            # (a fresh session: the stored liability is 0)
                dmu = np.stack([np.abs(D) @ Cb[s] + 2 * ncols * U * (np.abs(D) @ np.abs(cf_ref[s])) for s in range(ns)], axis=1)
                worst["mu"] = max(worst["mu"], float(np.max(np.abs(hip.annot_mu().reshape(p, -1) - ref.annot_mu().reshape(p, -1)) / dmu)))
                tb = _table_bounds(kind, D, cf_ref, Cb)
                th, tr = hip.annot_prior(), ref.annot_prior()
                assert np.all(np.isfinite(th))
                worst["table"] = max(worst["table"], float(np.max(np.abs(th - tr) / tb)))
                mb = np.atleast_2d(tb.T).mean(axis=1) if kind != "tree" else None
                if mb is not None:                                          # the column means: the mean of the entries' bounds + the sum's rounding
                    assert np.all(np.abs(rh["means"] - rr["means"]) <= mb + 2 * (p + 4) * U)
                hip.annot_end()
            ref.annot_end()
        print(f"{kind} Float{precision} p={p}: worst ratios {worst}")
        assert all(v <= 1.0 for v in worst.values()), worst
    finally:
        hip.close()


@pytest.mark.parametrize("kind", ["BayesC", "BayesR", "tree"])
def test_float32_and_float64_contexts_build_the_same_table(kind):
    p, ncols = 2085, 3
    D = _design(p, ncols)
    rng = np.random.default_rng(8)
    deltas = _delta(kind, p, rng)
    ns = 1 if kind == "BayesC" else 3
    coef0 = rng.standard_normal((ncols, ns)) * 0.3 if ns > 1 else rng.standard_normal(ncols) * 0.3
    got = []
    for precision in (32, 64):
        hip, _ = _engines(kind, precision, p)
        try:
            _set_delta((hip,), deltas)
            hip.annot_begin(kind, D, coef0, 1.0, _start_prior(kind, p))
            res = hip.annot_step(iteration=4, seed=9, variance=1.3)
            got.append((hip.annot_prior(), hip.annot_liability(), res["coefficients"], res["means"]))
        finally:
            hip.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


def test_structure_empty_and_single_active_sets():
    p, ncols = 1003, 2
    D = _design(p, ncols)
    hip, ref = _engines("BayesR", 64, p)
    try:
        coef0 = np.array([[0.2, -0.3, 0.1], [0.5, 0.4, -0.2]])
        # every delta = 1: steps 2 and 3 have empty active sets, their coefficients stay, their columns are still rebuilt
        _set_delta((hip, ref), [np.ones(p, dtype=np.int32)])
        for e in (hip, ref):
            e.annot_begin("BayesR", D, coef0, 1.0, _start_prior("BayesR", p))
        rh, rr = hip.annot_step(iteration=1, seed=3, variance=1.0), ref.annot_step(iteration=1, seed=3, variance=1.0)
        assert list(rh["n_active"]) == [p, 0, 0] == list(rr["n_active"])
        assert np.array_equal(rh["coefficients"][:, 1:], coef0[:, 1:])
        assert not np.array_equal(rh["coefficients"][:, 0], coef0[:, 0])
        assert not hip.annot_liability()[:, 1:].any()
        th = hip.annot_prior()
        p2 = np.clip(R.phi(R.mu_of(D, coef0[:, 1])), EPS, 1 - EPS)
        np.testing.assert_allclose(th[:, 1] / (1.0 - th[:, 0]), 1.0 - p2, rtol=1e-12)      # column 2 = P1 (1 - P2) with the untouched step-2 coefficients
        np.testing.assert_allclose(th.sum(axis=1), 1.0, rtol=0, atol=4 * EPS)
        np.testing.assert_allclose(hip.annot_mu()[:, 1:], ref.annot_mu()[:, 1:], rtol=0, atol=0)
        # exactly one active marker in steps 2 and 3; the others keep their stored liability bit for bit
        stored = hip.annot_liability()
        d = np.ones(p, dtype=np.int32); d[::2] = 1; d[777] = 4
        _set_delta((hip, ref), [d])
        rh = hip.annot_step(iteration=2, seed=3, variance=1.0)
        assert list(rh["n_active"]) == [p, 1, 1]
        now = hip.annot_liability()
        keep = np.ones(p, dtype=bool); keep[777] = False
        assert np.array_equal(now[keep, 1:], stored[keep, 1:])
        assert np.all(now[777, 1:] >= 0) and np.all(np.isfinite(now)) and now[777, 1] != 0
        assert np.all(np.isfinite(rh["coefficients"]))
        # one active marker: d_0 = 1, the intercept's conditional is N(c_0 + e, 1); slopes shrink towards 0 by 1 / (x^2 + 1 / var)
        assert np.all(np.isfinite(hip.annot_prior()))
    finally:
        hip.close()


def test_structure_far_tails():
    """mu = +-40: the tail branch of the truncated normal.  The liability is finite and on its side of 0, the prior is clipped."""
    p = 1003
    D = np.hstack([np.ones((p, 1)), np.zeros((p, 1))])
    D[:, 1] = np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
    delta = np.zeros(p); delta[::4] = 1.0; delta[1::4] = 1.0       # both signs of mu with both responses
    hip, _ = _engines("BayesC", 64, p)
    try:
        _set_delta((hip,), [delta])
        hip.annot_begin("BayesC", D, np.array([0.0, 40.0]), 1.0, _start_prior("BayesC", p))
        hip.annot_step(iteration=1, seed=2, variance=1e-12)         # (a tight prior: the slope stays near 0 after the draw)
        l = hip.annot_liability()
        assert np.all(np.isfinite(l))
        assert np.all(l[delta != 0] >= 0) and np.all(l[delta == 0] <= 0)
        wrong = (delta != 0) != (D[:, 1] > 0)                        # response against the sign of mu: the far tail
        assert wrong.sum() > p // 3 and np.all(np.abs(l[wrong]) < 1.0)
        # responses that agree with the sign of mu and a loose prior: the slope stays near 40, the table is clipped
        hip.annot_end()
        _set_delta((hip,), [(D[:, 1] > 0).astype(np.float64)])
        hip.annot_begin("BayesC", D, np.array([0.0, 40.0]), 1.0, _start_prior("BayesC", p))
        res = hip.annot_step(iteration=1, seed=2, variance=1e6)
        slope = res["coefficients"][1]
        pi = hip.annot_prior()
        mu = hip.annot_mu()
        assert np.allclose(mu, res["coefficients"][0] + D[:, 1] * slope, rtol=0, atol=1e-12)
        assert slope > 30 and np.all(np.abs(mu) > 9)
        assert np.all(pi[mu > 0] == EPS) and np.all(pi[mu < 0] == 1 - EPS)
        assert pi.min() >= EPS and pi.max() <= 1 - EPS
    finally:
        hip.close()


def _sweep_kw(kind):
    if kind == "tree":
        return dict(vare=np.eye(2), var_effect=np.eye(2) * 0.05)
    return dict(vare=1.0, var_effect=0.05)


@pytest.mark.parametrize("kind,precision", [("BayesC", 32), ("BayesR", 32), ("tree", 32), ("BayesC", 64), ("BayesR", 64), ("tree", 64)])
def test_determinism_and_the_resident_table(kind, precision):
    """Two sessions give the same bits; the sweep after a step equals a sweep handed the downloaded table through the host pointer."""
    p, ncols = 2085, 3
    D = _design(p, ncols)
    rng = np.random.default_rng(12)
    y = rng.standard_normal(24)
    ns = 1 if kind == "BayesC" else 3
    coef0 = rng.standard_normal((ncols, ns)) * 0.3 if ns > 1 else rng.standard_normal(ncols) * 0.3
    runs = []
    for resident in (True, True, False):
        hip, _ = _engines(kind, precision, p)
        try:
            for k in range(METHOD[kind][1]):
                hip.set_residual(y * (1 + k), k)
                hip.set_state(k, delta=np.ones(p))
            hip.annot_begin(kind, D, coef0, 1.0, _start_prior(kind, p))
            extra = dict(pi_classes=None) if kind == "BayesR" else {}
            st = hip.sweep(iteration=1, seed=5, resident_priors=True, **_sweep_kw(kind), **extra)
            res = hip.annot_step(iteration=1, seed=5, variance=1.2)
            table = hip.annot_prior()
            if resident:
                st = hip.sweep(iteration=2, seed=5, resident_priors=True, **_sweep_kw(kind), **extra)
            else:
                hip.annot_end()
                key = {"BayesC": "pi_vec", "BayesR": "pi_matrix", "tree": "log_prior_states"}[kind]
                st = hip.sweep(iteration=2, seed=5, **_sweep_kw(kind), **{key: table})
            state = [hip.get_state(k) for k in range(METHOD[kind][1])]
            runs.append((table, res["coefficients"], res["means"], [s[0] for s in state], [s[2] for s in state], hip.get_residual(0)))
        finally:
            hip.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    assert 0 < np.count_nonzero(runs[0][3][0]) < p


def test_accumulate_is_the_running_mean():
    p = 1003
    D = _design(p, 2)
    hip, _ = _engines("BayesC", 64, p)
    try:
        hip.set_state(0, delta=(np.arange(p) % 3 == 0).astype(np.float64))
        hip.annot_begin("BayesC", D, np.zeros(2), 1.0, _start_prior("BayesC", p))
        tabs = []
        for k in (1, 2, 3):
            hip.annot_step(iteration=k, seed=1, variance=1.0)
            hip.annot_accumulate(k)
            tabs.append(hip.annot_prior())
        m, m2 = hip.annot_means()
        assert np.allclose(m, np.mean(tabs, axis=0), rtol=1e-13, atol=0) and np.allclose(m2, np.mean(np.square(tabs), axis=0), rtol=1e-13, atol=0)
    finally:
        hip.close()


def test_error_contract():
    import jwas_jl_amd as J
    p = 1003
    D = _design(p, 2)

    def code(fn, *a, **k):
        try:
            fn(*a, **k)
        except J.JwasHipError as ex:
            return ex.code
        return 0

    hip = J.HipEngine(0)
    try:
        hip.load_dense(_genotypes(p, 32))
        hip.setup_blocks(64, "f64")
        assert code(hip.annot_begin, "BayesC", D, np.zeros(2), 1.0, _start_prior("BayesC", p)) == ESTATE      # before init_state
        hip.init_state("BayesC", 1)
        hip._annot = (0, 1, 2)
        assert code(hip.annot_step, iteration=1, seed=1, variance=1.0) == ESTATE                                # before begin
        assert code(hip.annot_begin, "BayesR", D, np.zeros((2, 3)), 1.0, _start_prior("BayesR", p)) == EINVAL  # kind against the method
        assert code(hip.annot_begin, "BayesC", D[:-1], np.zeros(2), 1.0, _start_prior("BayesC", p - 1)) == EINVAL
        bad = D.copy(); bad[5, 0] = 2.0
        assert code(hip.annot_begin, "BayesC", bad, np.zeros(2), 1.0, _start_prior("BayesC", p)) == EINVAL
        assert code(hip.annot_begin, "BayesC", D, np.zeros(2), -1.0, _start_prior("BayesC", p)) == EINVAL
        hip.comm_init_loopback(0, 0, 1)
        assert code(hip.annot_begin, "BayesC", D, np.zeros(2), 1.0, _start_prior("BayesC", p)) == EUNSUP       # a sharded context
        hip.comm_destroy()
        hip.annot_begin("BayesC", D, np.zeros(2), 1.0, _start_prior("BayesC", p))
        assert code(hip.annot_begin, "BayesC", D, np.zeros(2), 1.0, _start_prior("BayesC", p)) == ESTATE       # a second begin
        assert code(hip.annot_step, iteration=0, seed=1, variance=1.0) == EINVAL
        assert code(hip.annot_step, iteration=1, seed=1, variance=0.0) == EINVAL
        hip.set_residual(np.random.default_rng(1).standard_normal(24).astype(np.float32), 0)
        assert code(hip.sweep, iteration=1, seed=1, vare=1.0, var_effect=0.05, pi_vec=np.full(p, 0.5)) == EINVAL   # a host pointer during a session
        hip.sweep(iteration=1, seed=1, vare=1.0, var_effect=0.05, resident_priors=True)
        hip.annot_end()
        assert code(hip.annot_accumulate, 1) == ESTATE
        hip.init_state("MTBayesC", 2)
        hip.setup_blocks(64, "f64")
        hip.annot_begin("tree", D, np.zeros((2, 3)), 1.0, _start_prior("tree", p))
        hip.init_state("MTBayesC", 2)                                 # a new chain ends the session
        assert code(hip.annot_step, iteration=1, seed=1, variance=1.0) == ESTATE
    finally:
        hip.close()
    hip = J.HipEngine(0)
    try:                                                              # constraint = true
        hip.load_dense(_genotypes(p, 32))
        hip.setup_blocks(64, "f64")
        hip.init_state(5, 2)                                          # JWAS_HIP_MEGABAYESC
        assert code(hip.annot_begin, "tree", D, np.zeros((2, 3)), 1.0, _start_prior("tree", p)) == EUNSUP
    finally:
        hip.close()


# ---- runMCMC ------------------------------------------------------------------------------------------------------------------
def _annotated_problem(small_data, two_traits):
    raw = small_data["raw"][:, :320].astype(np.float64)
    n, p = raw.shape
    rng = np.random.default_rng(41)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(raw, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    ann = np.zeros((p, 2)); ann[:p // 4, 0] = 1.0; ann[:, 1] = rng.standard_normal(p)
    beta = np.zeros(p); beta[rng.choice(p // 4, 12, replace=False)] = rng.standard_normal(12)
    g = (raw - raw.mean(0)) @ beta
    y = g / g.std() * np.sqrt(0.6) + rng.standard_normal(n) * np.sqrt(0.4)
    ph = pd.DataFrame({"ID": ids, "y1": y})
    if two_traits:
        ph["y2"] = 0.7 * y + 0.7 * rng.standard_normal(n)
    return gdf, ph, ann


@pytest.mark.parametrize("case", ["BayesC", "BayesR", "tree"])
def test_runmcmc_gpu_vs_standin(tmp_path, small_data, case):
    from jwas_jl_amd import api
    gdf, ph, ann = _annotated_problem(small_data, case == "tree")
    outs = {}
    for name, engine in (("ref", AnnotOracleEngine64()), ("hip", None)):
        with contextlib.redirect_stdout(io.StringIO()):
            if case == "tree":
                Pi = {(0.0, 0.0): 0.7, (1.0, 0.0): 0.1, (0.0, 1.0): 0.1, (1.0, 1.0): 0.1}
                geno = api.get_genotypes(gdf, np.eye(2) * 0.5, method="BayesC", annotations=ann, Pi=Pi, double_precision=True)
                model = api.build_model("y1 = intercept + geno\ny2 = intercept + geno", np.eye(2))
            else:
                pi = dict(Pi=0.7) if case == "BayesC" else dict(Pi=[0.7, 0.15, 0.1, 0.05])
                geno = api.get_genotypes(gdf, method=case, annotations=ann, double_precision=True, **pi)
                model = api.build_model("y1 = intercept + geno")
            outs[name] = api.runMCMC(model, ph, chain_length=40, burnin=10, seed=13, double_precision=True, annotation_priors="device",
                                     output_folder=str(tmp_path / name), _engine=engine)
    eo, eh = outs["ref"]["marker effects geno"], outs["hip"]["marker effects geno"]
    d_eff = np.abs(eh["Estimate"].to_numpy(dtype=np.float64) - eo["Estimate"].to_numpy(dtype=np.float64)).max()
    d_freq = np.abs(eh["Model_Frequency"].to_numpy(dtype=np.float64) - eo["Model_Frequency"].to_numpy(dtype=np.float64)).max()
    co, chh = outs["ref"]["annotation coefficients geno"], outs["hip"]["annotation coefficients geno"]
    d_coef = np.abs(chh["Estimate"].to_numpy(dtype=np.float64) - co["Estimate"].to_numpy(dtype=np.float64)).max()
    d_pi = np.abs(outs["hip"]["pi_geno"]["Estimate"].to_numpy(dtype=np.float64) - outs["ref"]["pi_geno"]["Estimate"].to_numpy(dtype=np.float64)).max()
    print(f"runMCMC {case}: effects {d_eff:.3e}, frequencies {d_freq:.3e}, annotation coefficients {d_coef:.3e}, pi {d_pi:.3e}")
    assert d_freq <= 1e-12 and d_eff <= 1e-8 and d_coef <= 1e-9 and d_pi <= 1e-9


def test_device_chain_samples_the_probit_posterior():
    """tests/test_annot_host.py's exact-posterior check on the device: the chain length and the seed were fixed on the CPU."""
    import jwas_jl_amd as J
    case = R.posterior_case()
    hip = R.posterior_engine(J.HipEngine(0, precision=64), case)
    try:
        ma, sa = R.batch_means(R.posterior_chain(hip))
    finally:
        hip.close()
    mb, sb = R.batch_means(R.host_chain(case))
    ratio = np.abs(ma - mb) / (4.0 * np.sqrt(sa ** 2 + sb ** 2))
    print("device", ma, "host", mb, "ratio", ratio)
    assert np.all(ratio <= 1.0), ratio
