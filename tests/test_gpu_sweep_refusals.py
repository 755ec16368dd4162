"""Every refusal of the sweep's parameter checks, in both widths: its code, its message, and which one wins when two conditions fail.

The checks of jwas_sweep_params (csrc/jwas_hip.hip: sweep_fill_params of a Float32 context, f64_fill_params of a Float64 one, and the
prior fill the two share) are driven through the bare C ABI on one small context per width (n = 300, p = 40, one block of the smallest
size the library admits, 64; a second one with a 1024-marker block for the block-size limits).  The expected strings are written from the source of the commit before the two
fills shared their common part; every row passed there unchanged."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_dataset

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUP = -1, -3, -4
N, P_SMALL, P_BIG = 300, 40, 1040
INF = float("inf")

M_COV = ("multi-trait BayesA/B needs per-marker effect covariances (var_effect_matrix, or jwas_hip_sample_marker_covariances)",
         "multi-trait BayesA/B needs per-marker effect covariances (jwas_hip_set_marker_covariances_f64, or jwas_hip_sample_marker_covariances)")
M_INDEP = "independent_blocks is not available with per-marker effect covariances"
M_COV_LPR = "marker-specific joint priors are not available with per-marker effect covariances"
M_RSING = "residual covariance matrix is singular"
M_GSING = "marker effect covariance matrix is singular"
M_S2 = "All MTBayesABC sampler II state probabilities are zero or invalid."
M_LPR_T = "marker-specific joint priors support 2 traits (got 3)"
M_VARE = "residual variance must be positive"
M_VARG = "marker effect variance must be positive"
M_PI01 = "pi must lie in [0,1]"
M_SIGMA = "BayesR sigmaSq must be positive."
M_NEG = "BayesR pi entries must be nonnegative."
M_SUM = "BayesR pi must sum to 1."
M_BVEC = ("BayesB needs per-marker effect variances (var_effect_vec)", "BayesB needs per-marker effect variances (var_effect_vec_f64)")
M_ANNOT = ("an annotation session is open: the sweep reads its resident prior table, pi_vec / pi_matrix / log_prior_states_matrix must be NULL")
M_F64_VM = ("var_effect_matrix holds float covariances; a Float64 context takes them in double through jwas_hip_set_marker_covariances_f64 "
            "(or draws them with jwas_hip_sample_marker_covariances)")
M_F64_LPR_ST = "log_prior_states_matrix is for the multi-trait samplers"


def _set(name, *vals, at=0):
    def f(P, aux):
        arr = getattr(P, name)
        for i, v in enumerate(vals):
            arr[at + i] = v
    return f


def _scalar(name, v):
    return lambda P, aux: setattr(P, name, v)


def _null(name):
    return lambda P, aux: setattr(P, name, None)


def _lpr(P, aux):
    P.log_prior_states_matrix = aux["lpr"].ctypes.data_as(C.POINTER(C.c_double))


def _pi_vec(P, aux):
    P.pi_vec = aux["pi_vec"].ctypes.data_as(C.POINTER(C.c_double))


def _float_vm(P, aux):
    P.var_effect_matrix = aux["vm32"].ctypes.data_as(C.POINTER(C.c_float))


def _zero_matrix(name, t):
    return _set(name, *([0.0] * (t * t)))


def _both(*fs):
    def f(P, aux):
        for g in fs:
            g(P, aux)
    return f


# (method, t, cov: None | "none" | "set", change, code, message or (Float32 message, Float64 message); widths: which contexts run the row)
ROWS = [
    # per-marker covariances
    ("MTBayesB", 2, "none", None, EINVAL, M_COV, (32, 64)),
    ("MTBayesB", 2, "set", _scalar("independent_blocks", 1), EUNSUP, M_INDEP, (32, 64)),
    ("MTBayesB_II", 2, "set", _lpr, EUNSUP, M_COV_LPR, (32, 64)),
    ("MTBayesB", 2, "set", _both(_scalar("independent_blocks", 1), _lpr), EUNSUP, M_INDEP, (32, 64)),            # two fail: the first wins
    ("MTBayesB", 2, "none", _both(_scalar("independent_blocks", 1), _lpr), EINVAL, M_COV, (32, 64)),              # three fail
    ("MTBayesB", 2, "set", _both(_lpr, _zero_matrix("vare", 2), _zero_matrix("vare_f64", 2)), EUNSUP, M_COV_LPR, (32, 64)),
    ("MegaBayesB", 2, "none", None, EINVAL, M_COV[0], (32,)),
    ("MTBayesB", 2, "set", _float_vm, EUNSUP, M_F64_VM, (64,)),
    # the covariance matrices and the joint priors of the multi-trait samplers
    ("MTBayesC", 2, None, _both(_zero_matrix("vare", 2), _zero_matrix("vare_f64", 2)), EINVAL, M_RSING, (32, 64)),
    ("MTBayesC", 2, None, _both(_zero_matrix("var_effect", 2), _zero_matrix("var_effect_f64", 2)), EINVAL, M_GSING, (32, 64)),
    ("MTBayesC", 3, None, _both(_zero_matrix("vare", 3), _zero_matrix("vare_f64", 3), _zero_matrix("var_effect", 3),
                                _zero_matrix("var_effect_f64", 3)), EINVAL, M_RSING, (32, 64)),
    ("MTBayesC_II", 2, None, _set("log_prior_states", -INF, -INF, -INF, -INF), EINVAL, M_S2, (32, 64)),
    ("MTBayesC_II", 2, None, _set("log_prior_states", -INF, float("nan"), -INF, -INF), EINVAL, M_S2, (32, 64)),
    ("MTBayesB_II", 2, "set", _set("log_prior_states", -INF, -INF, -INF, -INF), EINVAL, M_S2, (32, 64)),
    ("MTBayesC", 3, None, _lpr, EUNSUP, M_LPR_T, (32, 64)),
    # (the order around the joint prior matrix differs per width: Float32 inverts the covariances first)
    ("MTBayesC", 3, None, _both(_lpr, _zero_matrix("vare", 3), _zero_matrix("vare_f64", 3)), (EINVAL, EUNSUP), (M_RSING, M_LPR_T), (32, 64)),
    ("BayesC", 1, None, _lpr, EINVAL, M_F64_LPR_ST, (64,)),
    # constraint = true
    ("MegaBayesC", 2, None, _set("vare", 0.0, at=3), EINVAL, M_VARE, (32,)),
    ("MegaBayesC", 2, None, _set("var_effect", -1.0, at=0), EINVAL, M_VARG, (32,)),
    ("MegaBayesC", 2, None, _set("pi_classes", 1.5, at=1), EINVAL, M_PI01, (32,)),
    ("MegaBayesC", 2, None, _both(_set("pi_classes", -0.5, at=0), _set("vare", 0.0, at=3)), EINVAL, M_PI01, (32,)),      # (trait 0 before trait 1)
    # single trait
    ("BayesC", 1, None, _both(_set("vare", 0.0), _set("vare_f64", 0.0)), EINVAL, M_VARE, (32, 64)),
    ("BayesC", 1, None, _both(_set("var_effect", 0.0), _set("var_effect_f64", 0.0)), EINVAL, M_VARG, (32, 64)),
    ("BayesC", 1, None, _both(_set("vare", -1.0), _set("vare_f64", -1.0), _set("var_effect", 0.0), _set("var_effect_f64", 0.0)), EINVAL, M_VARE, (32, 64)),
    ("BayesB", 1, None, _both(_null("var_effect_vec"), _null("var_effect_vec_f64")), EINVAL, M_BVEC, (32, 64)),
    ("BayesR", 1, None, _both(_set("var_effect", 0.0), _set("var_effect_f64", 0.0)), EINVAL, M_SIGMA, (32, 64)),
    ("BayesR", 1, None, _set("pi_classes", 0.96, -0.01, 0.04, 0.01), EINVAL, M_NEG, (32, 64)),
    ("BayesR", 1, None, _set("pi_classes", 0.9, 0.05, 0.03, 0.01), EINVAL, M_SUM, (32, 64)),
    ("BayesR", 1, None, _set("pi_classes", 0.9, -0.05, 0.03, 0.01), EINVAL, M_NEG, (32, 64)),                     # negative AND a sum off 1
    ("BayesR", 1, None, _both(_set("var_effect", 0.0), _set("var_effect_f64", 0.0), _set("pi_classes", 0.9, -0.05, 0.03, 0.01)), EINVAL, M_SIGMA, (32, 64)),
    ("BayesR", 1, None, _both(_set("vare", 0.0), _set("vare_f64", 0.0), _set("var_effect", 0.0), _set("var_effect_f64", 0.0)), EINVAL, M_VARE, (32, 64)),
]
# one 1024-marker block: the limits on the block size
BIG_ROWS = [
    ("MTBayesB", 3, "none", None, EINVAL, M_COV[0], (32,)),                                                         # (the missing covariances first)
    ("MTBayesB", 3, "set", None, EUNSUP, "per-marker effect covariances need block_size * ntraits <= 2048 (got 1024 x 3)", (32,)),
    ("MTBayesC", 2, None, _lpr, EUNSUP, "marker-specific joint priors need a block size <= 512 (got 1024)", (32,)),
    ("MTBayesC", 3, None, None, EUNSUP, "Float64 contexts need block size x traits <= 2048 (got 1024 x 3)", (64,)),
    ("MTBayesC", 3, None, _lpr, EUNSUP, "Float64 contexts need block size x traits <= 2048 (got 1024 x 3)", (64,)),
]
# every (method, t) of the tables sweeps once with the unchanged parameters: a row's refusal is its change's
VALID = sorted({(m, t) for m, t, *_ in ROWS})


class Ctx:
    def __init__(self, precision, p, bs):
        import jwas_jl_amd as J
        from jwas_jl_amd import _lib
        self._lib, self.precision, self.p = _lib, precision, p
        self.dtype = np.float64 if precision == 64 else np.float32
        d = make_dataset(n=N, p=p, ncausal=4, seed=9)
        self.y = (d["y"] - d["y"].mean()).astype(self.dtype)
        self.hip = J.HipEngine(0, precision=precision)
        self.hip.load_dense(np.asfortranarray(d["X"].astype(self.dtype)))
        self.hip.setup_blocks(bs, *(() if precision == 64 else ("f64",)))

    def params(self, method, t, cov):
        """Valid parameters of one sweep of (method, t) on a fresh chain, and the arrays they point to."""
        hip, p, L = self.hip, self.p, self._lib
        rng = np.random.default_rng(t)
        hip.init_state(method, t)
        for k in range(t):
            hip.set_residual(self.y, k)
        P = L.SweepParams()
        P.method, P.ntraits, P.nreps, P.iteration, P.seed = hip.method, t, 1, 1, 5
        R = 0.5 * (np.eye(t) + 0.2 * (1 - np.eye(t)))
        G = 0.01 * (np.eye(t) + 0.3 * (1 - np.eye(t)))
        for i in range(t * t):
            P.vare[i] = P.vare_f64[i] = R.flat[i]
            P.var_effect[i] = P.var_effect_f64[i] = G.flat[i]
        P.pi = 0.9
        for k, v in enumerate((0.95, 0.03, 0.015, 0.005)):
            P.pi_classes[k] = v
        for k, v in enumerate((0.0, 0.01, 0.1, 1.0)):
            P.gamma[k] = v
        aux = {"lpr": np.log(rng.dirichlet(np.ones(1 << t) * 2, size=p)), "pi_vec": np.full(p, 0.9),
               "vm32": np.ascontiguousarray(np.broadcast_to(G.astype(np.float32), (p, t, t))),
               "vv": np.full(p, 0.01, dtype=self.dtype)}
        if method.startswith("MT"):
            for k in range(1 << t):
                P.log_prior_states[k] = np.log(1.0 / (1 << t))
        if method.startswith("Mega"):
            for k in range(t):
                P.pi_classes[k] = 0.9
        if method == "BayesB":
            if self.precision == 64:
                P.var_effect_vec_f64 = aux["vv"].ctypes.data_as(C.POINTER(C.c_double))
            else:
                P.var_effect_vec = aux["vv"].ctypes.data_as(C.POINTER(C.c_float))
        if cov == "set":                            # resident covariances (a new chain has none)
            hip.sample_marker_covariances(t + 3.0, G * 3.0, seed=1, iteration=1)
        return P, aux

    def sweep(self, P):
        S = self._lib.SweepStats()
        rc = self.hip._L.jwas_hip_sweep(self.hip._h, C.byref(P), C.byref(S))
        return rc, self.hip._L.jwas_hip_last_error(self.hip._h).decode()


@pytest.fixture(scope="module", params=[32, 64])
def ctxs(request):
    small, big = Ctx(request.param, P_SMALL, 64), Ctx(request.param, P_BIG, 1024)
    yield small, big
    small.hip.close(); big.hip.close()


def _check(ctx, rows):
    w = 0 if ctx.precision == 32 else 1
    ran = 0
    for method, t, cov, change, code, msg, widths in rows:
        if ctx.precision not in widths:
            continue
        P, aux = ctx.params(method, t, cov)
        if change:
            change(P, aux)
        rc, err = ctx.sweep(P)
        want = (code[w] if isinstance(code, tuple) else code, msg[w] if isinstance(msg, tuple) else msg)
        assert (rc, err) == want, (method, t, cov, ctx.precision)
        ran += 1
    return ran


def test_unchanged_parameters_sweep(ctxs):
    small, _ = ctxs
    for method, t in VALID:
        if small.precision == 64 and method.startswith("Mega"):
            continue
        P, _aux = small.params(method, t, "set" if "BayesB" in method and t > 1 else None)
        rc, err = small.sweep(P)
        assert rc == 0, (method, t, err)


def test_every_refusal_and_which_one_wins(ctxs):
    small, big = ctxs
    assert _check(small, ROWS) == sum(small.precision in r[-1] for r in ROWS)
    assert _check(big, BIG_ROWS) == sum(big.precision in r[-1] for r in BIG_ROWS)


def test_sweep_guards_before_the_fill(ctxs):
    small, _ = ctxs
    P, _aux = small.params("BayesC", 1, None)
    P.method = 2
    assert small.sweep(P) == (EINVAL, "sweep method/ntraits (2/1) differ from init_state (0/1)")
    P, _aux = small.params("MTBayesC", 2, None)
    P.ntraits = 3
    assert small.sweep(P) == (EINVAL, "sweep method/ntraits (3/3) differ from init_state (3/2)")


def test_open_annotation_session_takes_no_prior_pointer(ctxs):
    small, _ = ctxs
    P, aux = small.params("BayesC", 1, None)
    D = np.ones((small.p, 2)); D[:, 1] = np.arange(small.p) % 2
    small.hip.annot_begin("BayesC", D, np.zeros(2), 1.0, np.full(small.p, 0.9))
    _pi_vec(P, aux)
    assert small.sweep(P) == (EINVAL, M_ANNOT)
    P.pi_vec = None
    rc, err = small.sweep(P)                      # (the resident table stands in)
    assert rc == 0, err
    small.hip.annot_end()
