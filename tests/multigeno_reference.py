"""TEST INFRASTRUCTURE for models with several genotype categories (jwas.jl_amd/multigeno.py): the stand-in engines -- the CPU oracle's
engines with the residual hand-over of jwas_hip_residual_handover -- and the exact posterior of a small model whose markers have
priors of their own, by enumeration in float64 (nothing here restates a kernel)."""
import itertools
import math

import numpy as np

from oracle_engine import OracleEngine, OracleEngine64


class _Handover:
    """residual_handover, an optional call log shared by the engines of one model, and the free HBM a memory guard is shown."""
    hbm_free = 1 << 40

    def _init_log(self, log, tag):
        self.log, self.tag = log, tag

    def device_info(self):
        return {"n_cu": 0, "hbm_total": self.hbm_free, "hbm_free": self.hbm_free}

    def residual_handover(self, src):
        """jwas_hip_residual_handover: all traits of src's residual become this engine's; the contexts must agree (EINVAL) and both
        hold genotypes and a state (ESTATE); dst is src: nothing happens.  A copy."""
        if self.method is None or src.method is None or self.n == 0 or src.n == 0:
            raise RuntimeError("residual_handover: load genotypes and call init_state on both engines first")
        if self.n != src.n or self.ntraits != src.ntraits or self.r.dtype != src.r.dtype:
            raise ValueError("residual_handover: the engines differ in n, traits or precision")
        if self.log is not None:
            self.log.append(("handover", self.tag, src.tag))
        if src is not self:
            self.r[...] = src.r

    def sweep(self, **kw):
        if self.log is not None:
            self.log.append(("sweep", self.tag, int(kw.get("marker_offset", 0))))
        return super().sweep(**kw)

    def get_residual(self, trait=0):
        if self.log is not None:
            self.log.append(("get_residual", self.tag))
        return super().get_residual(trait)


class MultiOracleEngine(_Handover, OracleEngine):
    def __init__(self, form="block", log=None, tag=None, **kw):
        OracleEngine.__init__(self, form, **kw)
        self._init_log(log, tag)


class MultiOracleEngine64(_Handover, OracleEngine64):
    def __init__(self, log=None, tag=None):
        OracleEngine64.__init__(self)
        self._init_log(log, tag)


def exact_marker_mixture_moments(X, y, vare, class_vars, class_probs):
    """draw_laws.exact_mixture_moments with classes of the marker's own: y = X a + e, e ~ N(0, vare I), a_j | class k ~
    N(0, class_vars[j][k]) (variance 0: a_j = 0) with prior class_probs[j][k].  All prod_j K_j configurations s are enumerated:
    P(s | y) ~ prod_j class_probs[j][s_j] N(y; 0, vare I + X D_s X'); a | s, y ~ N(m_s, V_s).  Returns (P, E[a], E[a a'])."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = X.shape
    assert len(class_vars) == p and len(class_probs) == p
    logp, cond = {}, {}
    for s in itertools.product(*[range(len(cv)) for cv in class_vars]):
        d = np.array([class_vars[j][k] for j, k in enumerate(s)], dtype=np.float64)
        V = vare * np.eye(n) + (X * d) @ X.T
        logp[s] = -0.5 * (np.linalg.slogdet(V)[1] + y @ np.linalg.solve(V, y)) + sum(math.log(class_probs[j][k]) for j, k in enumerate(s))
        act = np.flatnonzero(d > 0)
        m, C = np.zeros(p), np.zeros((p, p))
        if len(act):
            Xs = X[:, act]
            Vs = np.linalg.inv(Xs.T @ Xs / vare + np.diag(1.0 / d[act]))
            m[act] = Vs @ (Xs.T @ y) / vare
            C[np.ix_(act, act)] = Vs
        cond[s] = (m, C)
    mx = max(logp.values())
    tot = sum(math.exp(v - mx) for v in logp.values())
    P = {s: math.exp(v - mx) / tot for s, v in logp.items()}
    Ea = sum(P[s] * cond[s][0] for s in P)
    Eaa = sum(P[s] * (cond[s][1] + np.outer(cond[s][0], cond[s][0])) for s in P)
    return P, Ea, Eaa


# ---- the law of a two-category chain: category 1 BayesC (two markers), category 2 BayesR (two markers), fixed hyper-parameters ----
GAMMA = np.array([0.0, 0.01, 0.1, 1.0])


def two_category_case():
    """Four correlated markers, two per category; 2 x 2 x 4 x 4 = 64 configurations."""
    rng = np.random.default_rng(41)
    n = 40
    z = rng.standard_normal((n, 1))
    X = (0.6 * z + rng.standard_normal((n, 4))).astype(np.float32)
    X -= X.mean(0)
    y = (0.8 * X[:, 0] - 0.5 * X[:, 2] + 0.5 * rng.standard_normal(n)).astype(np.float32)
    y -= y.mean()
    pi1, var1 = 0.6, 0.3
    pis2, sig2 = np.array([0.5, 0.2, 0.2, 0.1]), 0.5
    c1 = ([0.0, var1], [pi1, 1 - pi1])
    c2 = (list(GAMMA * sig2), list(pis2))
    return dict(X1=X[:, :2], X2=X[:, 2:], y=y, vare=0.6, seed=91,
                kw1=dict(var_effect=np.float32(var1), pi=pi1), kw2=dict(var_effect=np.float32(sig2), pi_classes=pis2),
                class_vars=[c1[0], c1[0], c2[0], c2[0]], class_probs=[c1[1], c1[1], c2[1], c2[1]])


def run_two_category_chain(e1, e2, case, sweeps, burn, dtype=np.float32, wrong_prior=False):
    """The driver's iteration on two engines with fixed hyper-parameters: hand-over, sweep of category 1 (offset 0), hand-over, sweep of
    category 2 (offset p1).  wrong_prior: category 2 runs category 1's BayesC prior instead of its own (the chain a test must reject;
    its states are reported as classes 0 / 3).  Returns ({state: count}, effects after burn-in, sweeps - burn x 4)."""
    X1, X2, y = case["X1"].astype(dtype), case["X2"].astype(dtype), case["y"].astype(dtype)
    m2 = "BayesC" if wrong_prior else "BayesR"
    for e, X, m in ((e1, X1, "BayesC"), (e2, X2, m2)):
        e.load_dense(np.asfortranarray(X)); e.setup_blocks(64, "f64"); e.init_state(m)
    e1.set_state(delta=np.zeros(2, dtype=dtype))
    e2.set_state(delta=np.zeros(2, dtype=dtype) if wrong_prior else np.ones(2, dtype=np.int32))
    e1.set_residual(y)
    cast = (lambda v: np.float32(v)) if dtype == np.float32 else float
    kw1 = dict(case["kw1"], vare=cast(case["vare"]))
    kw2 = dict(case["kw1"] if wrong_prior else case["kw2"], vare=cast(case["vare"]))
    for kw in (kw1, kw2):
        kw["var_effect"] = cast(kw["var_effect"])
    counts, alphas = {}, np.empty((sweeps - burn, 4))
    owner = e1
    for it in range(1, sweeps + 1):
        for e, offset, kw in ((e1, 0, kw1), (e2, 2, kw2)):
            if e is not owner:
                e.residual_handover(owner)
                owner = e
            e.sweep(iteration=it, seed=case["seed"], marker_offset=offset, **kw)
        if it > burn:
            a1, _, d1 = e1.get_state()
            a2, _, d2 = e2.get_state()
            s2 = tuple(3 * int(v) for v in d2) if wrong_prior else tuple(int(v) - 1 for v in d2)
            s = tuple(int(v) for v in d1) + s2
            counts[s] = counts.get(s, 0) + 1
            alphas[it - burn - 1] = np.concatenate([a1, a2])
    return counts, alphas


def chain_figures(counts, alphas, exact, Ea, Eaa):
    """The figures of draw_laws.assert_st_chain: worst state-frequency difference and draw_laws.moments_check's three."""
    import draw_laws as DL
    tot = len(alphas)
    m = DL.moments_check(alphas, Ea, Eaa)
    m["freq"] = max(abs(counts.get(s, 0) / tot - pr) for s, pr in exact.items())
    return m


def figures_pass(m, tol=0.02):
    """The project's acceptance rule (draw_laws.assert_st_chain / assert_effect_moments)."""
    return m["freq"] < tol and m["dev1"] <= 5.0 and m["dev2"] <= 5.0 and m["se_sd"] <= 0.02
