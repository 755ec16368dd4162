"""The replayed calls behind tests/golden/session_golden.json: one small run of every device session (liabilities, location
parameters, missing traits, annotation priors, structural equation models), each in a Float32 and a Float64 context -- and, as
BLOCK_CASES behind tests/golden/block_session_golden.json, of the sessions that sweep blocks of markers themselves (mega-trait models,
several BayesR chains, random regression, GBLUP) -- and, as MTJ_CASES behind tests/golden/mtj_session_golden.json, of the joint multi-trait
session with 5 and 8 traits -- and, as OUTPUT_CASES behind tests/golden/output_side_golden.json, of the output side
of a context: state, residual and posterior transfer, X alpha on training and output rows, sparse samples, window sums, the GWAS session,
marker covariances, in both precisions and on packed storage, with their guards.

run_case(name, precision) returns what the fixture records for that run:

    "inputs"    SHA-256 over the raw bytes of every generated input (a mismatch here is the test's data, not the library)
    "values"    the small outputs in full, every double as its repr
    "digests"   SHA-256 of the raw bytes of every large output
    "errors"    (code, message) of one entry point called after _end, and (Float32) of _begin on a sharded context

tests/golden/make_session_golden.py writes these records with the library of the commit the fixture pins;
tests/test_gpu_session_golden.py replays them on the current library and requires equality."""
import hashlib

import numpy as np

CASES = ("liability", "locpar", "mtmiss", "annot_BayesC", "annot_BayesR", "annot_tree", "sem")
PRECISIONS = (32, 64)


class _Record:
    def __init__(self):
        self.inputs = hashlib.sha256()
        self.values, self.digests, self.errors = {}, {}, []

    def given(self, *arrays):
        for a in arrays:
            self.inputs.update(np.ascontiguousarray(a).tobytes())

    def small(self, name, v):
        self.values[name] = [repr(float(x)) for x in np.asarray(v, dtype=np.float64).ravel()]

    def large(self, name, a):
        self.digests[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    def error(self, fn, *a, **kw):
        from jwas_jl_amd._lib import JwasHipError
        try:
            fn(*a, **kw)
        except JwasHipError as e:
            self.errors.append([e.code, e.message])
        else:
            self.errors.append([0, ""])

    def sharded(self, hip, fn, *a, **kw):
        """fn on a context that drives a (one-rank loopback) shard: every session refuses it.  (A Float64 context takes no
        communicator: nothing to refuse there.)"""
        if hip.precision == 64:
            return
        hip.comm_init_loopback(0, 0, 1)
        try:
            self.error(fn, *a, **kw)
        finally:
            hip.comm_destroy()

    def done(self):
        return {"inputs": self.inputs.hexdigest(), "values": self.values, "digests": self.digests, "errors": self.errors}


def _engine(precision, n, p, method, t, rec, seed):
    import jwas_jl_amd as J
    rng = np.random.default_rng(seed)
    dtype = np.float64 if precision == 64 else np.float32
    X = np.asfortranarray(rng.integers(0, 3, (n, p)).astype(dtype))
    r0 = (rng.standard_normal((t, n)) * 1.3 + 0.2).astype(dtype)
    rec.given(X, r0)
    hip = J.HipEngine(0, precision=precision)
    hip.load_dense(X)
    hip.setup_blocks(64, "f64")
    hip.init_state(method, t)
    for k in range(t):
        hip.set_residual(r0[k], k)
    return hip, rng


def _residuals(hip, rec, t, tag):
    for k in range(t):
        rec.large(f"{tag}residual{k}", hip.get_residual(k))


# ---- liabilities: n = 700 (three 256-row workgroups, the last ragged), a 3-category trait with missing codes and a censored one ----
def _liability(precision, rec):
    n, t = 700, 2
    hip, rng = _engine(precision, n, 64, "MTBayesC", t, rec, 101)
    try:
        codes = rng.integers(0, 4, n).astype(np.int32)                  # 0 = missing
        lower = rng.standard_normal(n)
        upper = lower + rng.random(n)
        exact = np.arange(n) % 11 == 5
        upper[exact] = lower[exact]                                     # exact records
        lower[(np.arange(n) % 7 == 0) & ~exact] = -np.inf
        upper[(np.arange(n) % 7 == 3) & ~exact] = np.inf
        rec.given(codes, lower, upper)
        R = np.array([[1.0, 0.25], [0.25, 1.5]])
        hip.liability_begin()
        hip.set_categorical(0, codes, [-np.inf, 0.0, 1.0, np.inf])
        hip.set_censored(1, lower, upper)
        hip.liability_init(seed=17, R=R)
        below, above = hip.liability_minmax(0)
        rec.small("minmax_init", np.concatenate([below, above]))
        hip.liability_sample(iteration=1, seed=17, ngibbs=2, R=R)
        below, above = hip.liability_minmax(0)
        rec.small("minmax_before", np.concatenate([below, above]))
        hip.set_thresholds(0, [-np.inf, 0.0, 0.5 * (below[2] + above[2]), np.inf])
        below, above = hip.liability_minmax(0)
        rec.small("minmax_after", np.concatenate([below, above]))
        hip.liability_sample(iteration=2, seed=17, ngibbs=2, R=R)
        below, above = hip.liability_minmax(0)
        rec.small("minmax_last", np.concatenate([below, above]))
        for k in range(t):
            rec.large(f"liabilities{k}", hip.liabilities(k))
        _residuals(hip, rec, t, "")
        hip.liability_end()
        rec.error(hip.liabilities, 0)
        rec.sharded(hip, hip.liability_begin)
    finally:
        hip.close()


# ---- location parameters: n = 2 500 (the intercept spans three 1 024-record pieces), two traits ------------------------------------
def _structure_300():
    """A symmetric 300-level structure: row 0 holds 40 entries (the long-row branch), the other levels a chain."""
    nl = 300
    V = np.zeros((nl, nl))
    V[np.arange(nl), np.arange(nl)] = 2.0
    V[0, 1:40] = V[1:40, 0] = -0.03125
    for l in range(40, nl - 1):
        V[l, l + 1] = V[l + 1, l] = -0.5
    indptr, indices, values = [0], [], []
    for l in range(nl):
        cols = np.nonzero(V[l])[0]
        indices += cols.tolist()
        values += V[l, cols].tolist()
        indptr.append(len(indices))
    return nl, np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(values)


def _locpar_model(hip, rng, rec):
    n = hip.n
    x = rng.standard_normal(n)
    fac = rng.integers(-1, 40, n).astype(np.int32)                      # -1: in no level
    grp = rng.integers(0, 25, n).astype(np.int32)
    nl, indptr, indices, values = _structure_300()
    ped = rng.integers(0, nl, n).astype(np.int32)
    rec.given(x, fac, grp, ped, indptr, indices, values)
    hip.locpar_begin()
    hip.locpar_set_group_structure(1, indptr, indices, values)
    for k in range(2):
        hip.locpar_add_covariate(k)                                      # the intercept
    hip.locpar_add_covariate(0, x)
    hip.locpar_add_factor(1, fac, 40)
    hip.locpar_add_factor(0, grp, 25, random_group=0)                    # a 2-member random effect on the identity
    hip.locpar_add_factor(1, grp, 25, random_group=0)
    hip.locpar_add_factor(0, ped, nl, random_group=1)                    # a structured random effect
    return dict(Rinv=np.array([[1.25, -0.25], [-0.25, 0.625]]), Gi=[np.array([[2.0, -0.5], [-0.5, 1.5]]), np.array([[0.75]])])


def _locpar_outputs(hip, rec):
    rec.large("sol", hip.locpar_get_sol())
    m, m2 = hip.locpar_get_means()
    rec.large("mean", m)
    rec.large("mean2", m2)
    _residuals(hip, rec, 2, "")


def _locpar(precision, rec):
    hip, rng = _engine(precision, 2500, 64, "MTBayesC", 2, rec, 202)
    try:
        kw = _locpar_model(hip, rng, rec)
        for it in (1, 2, 3):
            st = hip.locpar_step(iteration=it, seed=23, **kw)
            rec.small(f"utu{it}", np.concatenate([u.ravel() for u in st["utu"]]))
            if it >= 2:
                hip.locpar_accumulate(it - 1)
        _locpar_outputs(hip, rec)
        hip.locpar_end()
        rec.error(hip.locpar_size)
        rec.sharded(hip, hip.locpar_begin)
    finally:
        hip.close()


# ---- missing traits: the model above, three observation patterns, imputation, per-record weights, one location step ------------------
def _mtmiss(precision, rec):
    hip, rng = _engine(precision, 2500, 64, "MTBayesC", 2, rec, 303)
    try:
        kw = _locpar_model(hip, rng, rec)
        codes = rng.choice([1, 2, 3], hip.n, p=[0.2, 0.2, 0.6]).astype(np.int32)
        rec.given(codes)
        # the tables of R = [[1, 0.5], [0.5, 2]] with dyadic entries (no linear algebra between the fixture and the replay)
        B, U, Ct = (np.zeros((4, 2, 2)) for _ in range(3))
        B[1, 0, 0], U[1, 0, 0], Ct[1, 0, 0] = 0.5, 1.25, 1.0
        B[2, 0, 0], U[2, 0, 0], Ct[2, 1, 1] = 0.25, 0.75, 0.5
        Ct[3] = [[1.25, -0.25], [-0.25, 0.625]]
        hip.mtmiss_begin(codes)
        hip.mtmiss_impute(iteration=1, seed=29, B=B, U=U)
        _residuals(hip, rec, 2, "imputed_")
        hip.mtmiss_set_record_weights(Ct)
        st = hip.locpar_step(iteration=1, seed=29, **kw)
        rec.small("utu_weighted", np.concatenate([u.ravel() for u in st["utu"]]))
        hip.mtmiss_set_record_weights(None)
        st = hip.locpar_step(iteration=2, seed=29, **kw)
        rec.small("utu_plain", np.concatenate([u.ravel() for u in st["utu"]]))
        hip.locpar_accumulate(1)
        _locpar_outputs(hip, rec)
        hip.mtmiss_end()
        hip.locpar_end()
        rec.error(hip.mtmiss_impute, iteration=2, seed=29, B=B, U=U)
        rec.sharded(hip, hip.mtmiss_begin, codes)
    finally:
        hip.close()


# ---- annotation priors: p = 1 100 (two 1 024-marker pieces, the second ragged), 3 columns ------------------------------------------------
def _annot(kind):
    def run(precision, rec):
        p, K = 1100, 3
        method, t = {"BayesC": ("BayesC", 1), "BayesR": ("BayesR", 1), "tree": ("MTBayesC", 2)}[kind]
        hip, rng = _engine(precision, 24, p, method, t, rec, 404)
        try:
            D = np.hstack([np.ones((p, 1)), (rng.random((p, 1)) < 0.3).astype(np.float64), rng.standard_normal((p, 1))])
            if kind == "BayesR":
                deltas = [rng.choice([1, 2, 3, 4], p, p=[0.5, 0.25, 0.15, 0.1]).astype(np.int32)]
            else:
                deltas = [(rng.random(p) < 0.4 - 0.1 * k).astype(np.float64) for k in range(t)]
            ns = 1 if kind == "BayesC" else 3
            coef0 = rng.uniform(-0.5, 0.5, K if ns == 1 else (K, ns))
            row = np.array([0.7, 0.15, 0.1, 0.05])
            start = np.full(p, 0.7) if kind == "BayesC" else np.tile(np.log(row) if kind == "tree" else row, (p, 1))
            rec.given(D, coef0, start, *deltas)
            for k, d in enumerate(deltas):
                hip.set_state(k, delta=d)
            hip.annot_begin(kind, D, coef0, 1.0, start)
            for it in (1, 2):
                st = hip.annot_step(iteration=it, seed=31, variance=[0.5, 1.0, 2.0][:ns] if ns > 1 else 0.5)
                rec.small(f"coefficients{it}", st["coefficients"])
                rec.small(f"n_active{it}", st["n_active"])
                rec.small(f"column_means{it}", st["means"])
                hip.annot_accumulate(it)
            rec.large("prior", hip.annot_prior())
            m, m2 = hip.annot_means()
            rec.large("mean", m)
            rec.large("mean2", m2)
            rec.large("liability", hip.annot_liability())
            rec.large("mu", hip.annot_mu())
            hip.annot_end()
            rec.error(hip.annot_accumulate, 3)
            rec.sharded(hip, hip.annot_begin, kind, D, coef0, 1.0, start)
        finally:
            hip.close()
    return run


# ---- structural equation models: n = 700, p = 1 100, t = 3, structure {(1,0), (2,0), (2,1)} ----------------------------------------------
def _sem(precision, rec):
    n, p, t = 700, 1100, 3
    hip, rng = _engine(precision, n, p, "MTBayesC", t, rec, 505)
    try:
        base = rng.standard_normal(n)
        y = np.stack([1.0 + 0.3 * k + 0.6 * base + rng.standard_normal(n) for k in range(t)])
        cs = np.tril(np.ones((t, t), dtype=np.int32), -1)
        lam0 = np.tril(rng.uniform(-0.8, 0.8, (t, t)), -1)
        alphas = [(rng.standard_normal((t, p)) * (rng.random((t, p)) < 0.3)).astype(hip.dtype) for _ in range(2)]
        Ks = [np.tril(rng.uniform(-1.5, 1.5, (t, t)), -1) for _ in range(2)]
        rec.given(y, cs, lam0, *alphas, *Ks)
        hip.sem_begin(y, cs)
        rec.small("gram", hip.sem_get_gram())
        hip.sem_set_lambda(lam0)
        rec.small("lambda_round_trip", hip.sem_get_lambda())
        for it in (1, 2):
            st = hip.sem_step(iteration=it, seed=37, R_diag=[1.3, 0.7, 2.1])
            for key in ("lambda", "mean", "ypr"):
                rec.small(f"{key}{it}", st[key])
            for k in range(t):
                hip.set_state(k, alpha=alphas[it - 1][k])
            hip.sem_accumulate(Ks[it - 1], it)
        rec.small("lambda_last", hip.sem_get_lambda())
        _residuals(hip, rec, t, "")
        for kind in ("indirect", "overall"):
            for k in range(t):
                for nm, v in zip(("mean", "mean2", "freq"), hip.sem_get_effects(kind, k)):
                    rec.large(f"{kind}{k}_{nm}", v)
        hip.sem_end()
        rec.error(hip.sem_get_effects, "indirect", 0)
        rec.sharded(hip, hip.sem_begin, y, cs)
    finally:
        hip.close()


# ---- the sessions with a block sweep of their own (tests/golden/block_session_golden.json) ---------------------------------------------
# n = 700 (three 256-row slices, the last ragged), p = 150 with blocks of 64 (three blocks, the last of 22 markers)
def _genotypes(precision, n, p, rec, seed):
    import jwas_jl_amd as J
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.integers(0, 3, (n, p)).astype(np.float64 if precision == 64 else np.float32))
    rec.given(X)
    hip = J.HipEngine(0, precision=precision)
    hip.load_dense(X)
    return hip, rng


def _stats(rec, tag, st):
    for key in sorted(st):
        if key != "step_ms":
            rec.small(f"{tag}_{key}", st[key])


def _state(rec, tag, state):
    for nm, v in zip(("alpha", "beta", "delta"), state):
        rec.large(f"{tag}{nm}", v)


# mega-trait: T = 9 (two trait tiles of 8, the second with one trait), first_trait = 3, missing cells, pi[0] = 0 (megaBayesC0!), 900
# output rows (more than the 768 padded training rows: the row buffer grows); then a session of one 150-marker block (bp = 256)
def _mega(precision, rec):
    n, p, T = 700, 150, 9
    hip, rng = _genotypes(precision, n, p, rec, 606)
    try:
        Xout = np.asfortranarray(rng.integers(0, 3, (900, p)).astype(hip.dtype))
        R0 = rng.standard_normal((T, n)) * 1.3 + 0.2
        missing = rng.random((T, n)) < 0.1
        rec.given(Xout, R0, missing)
        vare = 0.5 + 0.125 * np.arange(T)
        var_effect = 0.02 + 0.005 * np.arange(T)
        pi = np.array([0.0, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95])
        hip.load_output_dense(Xout)
        hip.mega_begin(T, block_size=64, first_trait=3)
        hip.mega_set_missing(missing)
        hip.mega_set_residual(R0)
        hip.mega_impute(iteration=1, seed=41, vare=vare)
        rec.large("imputed", hip.mega_get_residual())
        for it in (1, 2, 3):
            _stats(rec, f"sweep{it}", hip.mega_sweep(iteration=it, seed=41, vare=vare, var_effect=var_effect, pi=pi))
            hip.mega_accumulate(it)
        _state(rec, "", hip.mega_get_state())
        rec.large("residual", hip.mega_get_residual())
        for k in range(T):
            for nm, v in zip(("mean", "mean2", "freq"), hip.mega_posterior(k)):
                rec.large(f"posterior{k}_{nm}", v)
        rec.large("mul_alpha8", hip.mega_mul_alpha(8))
        G, xpx = hip.mega_gram(2)
        rec.large("gram2", G)
        rec.large("xpx2", xpx)
        rec.large("mul_alpha0_output_rows", hip.mega_mul_alpha(0, output_rows=True))
        hip.mega_begin(T, block_size=200, first_trait=3)
        hip.mega_set_residual(R0)
        _stats(rec, "one_block", hip.mega_sweep(iteration=1, seed=41, vare=vare, var_effect=var_effect, pi=pi))
        _state(rec, "one_block_", hip.mega_get_state())
        rec.large("one_block_residual", hip.mega_get_residual())
        hip.mega_end()
        rec.error(hip.mega_posterior, 0)
        rec.sharded(hip, hip.mega_begin, T, 64, 3)
    finally:
        hip.close()


# joint multi-trait (tests/golden/mtj_session_golden.json): t = 5 or 8, full Rinv and Ginv with dyadic entries, a Pi table over the 2^t
# joint states with some states of probability 0, 900 output rows (the row buffer grows); then a session of one 150-marker block; then
# the refusals that only the bare C ABI reaches
def _mtj(T):
    def run(precision, rec):
        n, p = 700, 150
        hip, rng = _genotypes(precision, n, p, rec, 1111)
        try:
            Xout = np.asfortranarray(rng.integers(0, 3, (900, p)).astype(hip.dtype))
            R0 = rng.standard_normal((T, n)) * 1.3 + 0.2
            log_pi = -rng.uniform(0.5, 6.0, 1 << T)
            log_pi[np.arange(1 << T) % 5 == 3] = -np.inf
            rec.given(Xout, R0, log_pi)
            rinv = np.diag(1.0 + 0.125 * np.arange(T)) + 0.0625
            ginv = np.diag(16.0 + 2.0 * np.arange(T)) - 0.5
            kw = dict(seed=61, rinv=rinv, ginv=ginv, log_pi=log_pi)
            hip.load_output_dense(Xout)
            hip.mtj_begin(T, block_size=64)
            hip.mtj_set_residual(R0)
            for it in (1, 2, 3):
                _stats(rec, f"sweep{it}", hip.mtj_sweep(iteration=it, **kw))
                hip.mtj_accumulate(it)
            _state(rec, "", hip.mtj_get_state())
            rec.large("residual", hip.mtj_get_residual())
            for k in range(T):
                for nm, v in zip(("mean", "mean2", "freq"), hip.mtj_posterior(k)):
                    rec.large(f"posterior{k}_{nm}", v)
            G, xpx = hip.mtj_gram(2)
            rec.large("gram2", G)
            rec.large("xpx2", xpx)
            rec.large(f"mul_alpha{T - 1}", hip.mtj_mul_alpha(T - 1))
            rec.large("mul_alpha0_output_rows", hip.mtj_mul_alpha(0, output_rows=True))
            hip.mtj_begin(T, block_size=200)
            hip.mtj_set_residual(R0)
            _stats(rec, "one_block", hip.mtj_sweep(iteration=1, **kw))
            _state(rec, "one_block_", hip.mtj_get_state())
            rec.large("one_block_residual", hip.mtj_get_residual())
            # the refusals of the bare ABI (the session stays open: each is refused before anything is dropped)
            B = [np.zeros(max(n, p)) for _ in range(3)]
            bad = R0[0].copy()
            bad[n - 1] = np.inf
            _raw(hip, rec, "jwas_hip_mtj_get_residual", T, B[0])
            _raw(hip, rec, "jwas_hip_mtj_posterior", -1, B[0], B[1], B[2])
            _raw(hip, rec, "jwas_hip_mtj_gram", 0, 150 * 150 - 1, np.zeros(150 * 150), None)
            _raw(hip, rec, "jwas_hip_mtj_set_residual", 0, bad)
            _raw(hip, rec, "jwas_hip_mtj_begin", 4, 64)
            _raw(hip, rec, "jwas_hip_mtj_begin", 9, 64)
            _raw(hip, rec, "jwas_hip_mtj_begin", T, 257)
            rec.large("residual_after_refusals", hip.mtj_get_residual())
            hip.mtj_end()
            rec.error(hip.mtj_posterior, 0)
            rec.sharded(hip, hip.mtj_begin, T, 64)
        finally:
            hip.close()
    return run


# K = 3 BayesR chains of one model: pi differs per chain, class 3 has probability 0 in chain 1
def _mega_chains(precision, rec):
    n, p, K = 700, 150, 3
    hip, rng = _genotypes(precision, n, p, rec, 707)
    try:
        r0 = rng.standard_normal(n) * 1.3 + 0.2
        rec.given(r0)
        vare, sigma2 = [0.5, 0.625, 0.75], [0.05, 0.0625, 0.075]
        gamma = [0.0, 0.01, 0.1, 1.0]
        pi = np.array([[0.9, 0.05, 0.03, 0.02], [0.8, 0.15, 0.0, 0.05], [0.7, 0.1, 0.1, 0.1]]).T
        hip.mega_begin(K, block_size=64, first_trait=3)
        hip.mega_set_residual(np.tile(r0, (K, 1)))
        for it in (1, 2, 3):
            _stats(rec, f"sweep{it}", hip.mega_sweep_r(iteration=it, seed=43, vare=vare, var_effect=sigma2, gamma=gamma, pi=pi))
            hip.mega_accumulate_r(it)
        _state(rec, "", hip.mega_get_state())
        rec.large("residual", hip.mega_get_residual())
        for k in range(K):
            for nm, v in zip(("mean", "mean2", "freq"), hip.mega_posterior(k)):
                rec.large(f"posterior{k}_{nm}", v)
        rec.large("psrf", hip.mega_psrf(3))
        hip.mega_end()
        rec.error(hip.mega_psrf, 3)
        rec.sharded(hip, hip.mega_begin, K, 64, 3)
    finally:
        hip.close()


# random regression: T = 5 time points, c = 2, 3, 4 coefficients (every instantiation of the sampler), one state with prior 0
def _rrm(c):
    def run(precision, rec):
        n, p, T = 700, 150, 5
        hip, rng = _genotypes(precision, n, p, rec, 808)
        try:
            Phi = rng.uniform(-1.0, 1.0, (T, c))
            observed = rng.random((T, n)) < 0.8
            W0 = rng.standard_normal((T, n)) * 1.3 + 0.2
            rec.given(Phi, observed, W0)
            G = 0.0625 * np.eye(c) + 0.015625
            log_pi = -1.0 - 0.25 * np.arange(1 << c)
            log_pi[2] = -np.inf
            hip.rrm_begin(Phi, observed, block_size=64)
            hip.rrm_set_residual(W0)
            for it in (1, 2, 3):
                _stats(rec, f"sweep{it}", hip.rrm_sweep(iteration=it, seed=47, vare=0.75, G=G, log_pi=log_pi))
                hip.rrm_accumulate(it)
            _state(rec, "", hip.rrm_get_state())
            rec.large("residual", hip.rrm_get_residual())
            for q in range(c):
                for nm, v in zip(("mean", "mean2", "freq"), hip.rrm_posterior(q)):
                    rec.large(f"posterior{q}_{nm}", v)
            rec.large("mul_alpha", hip.rrm_mul_alpha(c - 1))
            rec.large("m", hip.rrm_m())
            rec.large("gram2", hip.rrm_gram(2))
            hip.rrm_end()
            rec.error(hip.rrm_posterior, 0)
            rec.sharded(hip, hip.rrm_begin, Phi, observed, 64)
        finally:
            hip.close()
    return run


# GBLUP: n = 300, a random dense n x n matrix in the place of the eigenvectors (the replay pins bits; a LAPACK factorisation here would
# tie the inputs to the BLAS build).  The diagonal three-trait step draws with first_trait = 1: first_trait + T <= 4 is the entry
# point's own limit.
def _gblup(t, diagonal, first_trait):
    def run(precision, rec):
        n = 300
        rng = np.random.default_rng(909)
        dtype = np.float64 if precision == 64 else np.float32
        L = np.asfortranarray((rng.standard_normal((n, n)) / 16.0).astype(dtype))
        D = rng.uniform(0.05, 4.0, n)
        r0 = (rng.standard_normal((t, n)) * 1.3 + 0.2).astype(dtype)
        rec.given(L, D, r0)
        vare = (np.diag([0.75, 1.0, 1.25]) + 0.125)[:t, :t]
        G = (np.diag([0.5, 0.375, 0.625]) + 0.0625)[:t, :t]
        import jwas_jl_amd as J
        hip = J.HipEngine(0, precision=precision)
        try:
            hip.load_dense(L)
            hip.init_state("BayesC" if t == 1 else "MTBayesC", t)
            hip.gblup_begin(D)
            for k in range(t):
                hip.set_residual(r0[k], k)
            for it in (1, 2):
                _stats(rec, f"step{it}", hip.gblup_step(iteration=it, seed=53, vare=vare, G=G, diagonal=diagonal, first_trait=first_trait))
                rec.large(f"rhs{it}", hip.gblup_rhs())
            for k in range(t):
                alpha, beta, _ = hip.get_state(k)
                rec.large(f"alpha{k}", alpha)
                rec.large(f"beta{k}", beta)
            _residuals(hip, rec, t, "")
            hip.gblup_end()
            rec.error(hip.gblup_rhs)
            rec.sharded(hip, hip.gblup_begin, D)
        finally:
            hip.close()
    return run


# ---- the output side (tests/golden/output_side_golden.json): state, residual and posterior transfer, X alpha, output rows, sparse
# samples, window sums, the GWAS session, marker covariances ------------------------------------------------------------------------------
# n = 300 training rows (two 256-row slices, 212 pad rows), 70 output rows (one slice), p = 1 100 (two trips of the 1 024-wide
# compaction walk, a 76-marker tail).  Effect vectors: empty, 37 nonzeros (two batches of 16, one of 4, one single: every branch of the
# batched list), 400 nonzeros (4 nnz > p: the Float32 dense branch).
OUT_N, OUT_ROWS, OUT_P = 300, 70, 1100
OUT_NNZ = (("empty", 0), ("sparse", 37), ("dense", 400))


def _out_engine(precision, rec, seed, method=None, t=1, p=OUT_P, output_rows=True):
    hip, rng = _genotypes(precision, OUT_N, p, rec, seed)
    if output_rows:
        Xout = np.asfortranarray(rng.integers(0, 3, (OUT_ROWS, p)).astype(hip.dtype))
        rec.given(Xout)
        hip.load_output_dense(Xout)
    hip.setup_blocks(64, "f64")
    if method:
        hip.init_state(method, t)
    return hip, rng


def _effects(rng, p, nnz, dtype):
    """(ascending idx, val, the dense vector): nnz nonzero effects among p markers."""
    idx = np.sort(rng.choice(p, nnz, replace=False)).astype(np.int32)
    val = (rng.standard_normal(nnz) + 2.0).astype(dtype)                 # (never zero)
    a = np.zeros(p, dtype=dtype)
    a[idx] = val
    return idx, val, a


def _raw(hip, rec, name, *args):
    """One entry point through the bare C ABI: records (code, message)."""
    import ctypes as C
    rc = getattr(hip._L, name)(hip._h, *[a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args])
    rec.errors.append([int(rc), hip._L.jwas_hip_last_error(hip._h).decode() if rc else ""])
    return rc


def _out_context(method, t):
    def run(precision, rec):
        import ctypes as C
        hip, rng = _out_engine(precision, rec, 1001, method, t)
        try:
            n, p = hip.n, hip.p
            r0 = (rng.standard_normal((t, n)) * 1.3 + 0.2).astype(hip.dtype)
            rec.given(r0)
            rec.large("xpx", hip.xpx())
            for k in range(t):
                hip.set_residual(r0[k], k)
                rec.large(f"residual_round_trip{k}", hip.get_residual(k))
                for tag, nnz in OUT_NNZ:
                    idx, val, a = _effects(rng, p, nnz, hip.dtype)
                    b = rng.standard_normal(p).astype(hip.dtype)
                    d = rng.integers(1, 5, p).astype(np.int32) if method == "BayesR" else (a != 0).astype(hip.dtype)
                    rec.given(a, b, d)
                    hip.set_state(k, alpha=a, beta=b, delta=d)
                    _state(rec, f"{tag}{k}_", hip.get_state(k))
                    rec.large(f"{tag}{k}_mul_alpha", hip.mul_alpha(k))
                    rec.large(f"{tag}{k}_mul_alpha_output", hip.mul_alpha_output(k))
                    si, sv = hip.alpha_sparse(k)
                    assert np.array_equal(si, idx) and np.array_equal(sv, val), "alpha_sparse is not the list that was set"
                    rec.large(f"{tag}{k}_sparse_idx", si)
                    rec.large(f"{tag}{k}_sparse_val", sv)
                    if tag == "sparse" and k == 0:                       # a capacity that is too small: the error, nnz_out still filled
                        ci, cv, cn = np.zeros(10, dtype=np.int32), np.zeros(10, dtype=hip.dtype), C.c_int64(-1)
                        _raw(hip, rec, "jwas_hip_get_alpha_sparse" + ("_f64" if precision == 64 else ""), k, 10, ci, cv, C.byref(cn))
                        rec.small("sparse_nnz_out_when_too_small", [cn.value])
                    hip.sub_xalpha(k)
                    rec.large(f"{tag}{k}_residual_sub_xalpha", hip.get_residual(k))
            for ns in (1, 2, 3):
                for k in range(t):
                    _, _, a = _effects(rng, p, 37 * ns, hip.dtype)
                    d = rng.integers(1, 5, p).astype(np.int32) if method == "BayesR" else (a != 0).astype(hip.dtype)
                    rec.given(a, d)
                    hip.set_state(k, alpha=a, delta=d)
                hip.accumulate(ns)
            for k in range(t):
                for nm, v in zip(("mean", "mean2", "freq"), hip.posterior(k)):
                    rec.large(f"posterior{k}_{nm}", v)
        finally:
            hip.close()
    return run


# window sums: windows of 0, 1, 7, 8, 9 and 20 list entries (the empty window, the batch boundary of 8, a tail)
def _out_windows(precision, rec):
    hip, rng = _out_engine(precision, rec, 1002)
    try:
        counts = [0, 1, 7, 8, 9, 20]
        wptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        idx = rng.choice(hip.p, int(wptr[-1]), replace=False).astype(np.int32)
        v1, v2 = (rng.standard_normal(idx.size).astype(hip.dtype) for _ in range(2))
        rec.given(wptr, idx, v1, v2)
        for rows, out in (("training", False), ("output", True)):
            rec.small(f"{rows}_sums", np.concatenate(hip.window_sums(wptr, idx, v1, use_output_rows=out)))
            rec.small(f"{rows}_sums2", np.concatenate(hip.window_sums2(wptr, idx, v1, v2, use_output_rows=out)))
    finally:
        hip.close()


def _gwas_windows(p, width):
    cs = np.arange(0, p, width, dtype=np.int32)
    ce = np.minimum(cs + width, p).astype(np.int32)
    return np.concatenate([cs, [p // 2]]).astype(np.int32), np.concatenate([ce, [p // 2]]).astype(np.int32)      # (the last one empty)


def _gwas_session(hip, rec, tag, cs, ce, samples, local_ebv, out_rows):
    """One session over `samples`; every sample's sums must equal window_sums' over the same lists (entry 0 = all markers)."""
    hip.gwas_begin(cs, ce, local_ebv=local_ebv, use_output_rows=out_rows)
    rec.small(f"{tag}_geometry", [hip.gwas_geometry()[k] for k in ("nslices", "windows_per_chunk", "nchunks")])
    for i, (idx, val) in enumerate(samples):
        s, q = hip.gwas_sample(idx, val)
        rec.small(f"{tag}_sample{i}", np.concatenate([s, q]))
        lo, hi = np.searchsorted(idx, cs), np.searchsorted(idx, ce)
        pieces = [np.arange(idx.size)] + [np.arange(a, b) for a, b in zip(lo, hi)]
        wptr = np.concatenate([[0], np.cumsum([x.size for x in pieces])]).astype(np.int32)
        sel = np.concatenate(pieces).astype(np.int64)
        ws, wq = hip.window_sums(wptr, idx[sel], val[sel], use_output_rows=out_rows)
        assert np.array_equal(ws, s) and np.array_equal(wq, q), f"{tag}: the session's sums of sample {i} differ from window_sums'"
    if local_ebv:
        ebv, ns = hip.gwas_local_ebv()
        rec.large(f"{tag}_local_ebv", ebv)
        rec.small(f"{tag}_nsamples", [ns])
    hip.gwas_end()


def _out_gwas(precision, rec):
    hip, rng = _out_engine(precision, rec, 1003)
    try:
        cs, ce = _gwas_windows(hip.p, 100)
        samples = [_effects(rng, hip.p, nnz, hip.dtype)[:2] for nnz in (37, 0, 400)]
        rec.given(cs, ce, *[x for s in samples for x in s])
        for out_rows in (False, True):
            for local_ebv in (True, False):
                _gwas_session(hip, rec, f"{'output' if out_rows else 'training'}_{'ebv' if local_ebv else 'plain'}", cs, ce, samples, local_ebv, out_rows)
    finally:
        hip.close()
    # p = 4 500, a sample of 4 200 nonzeros: the session's list grows past its first 4 096 entries
    hip, rng = _out_engine(precision, rec, 1004, p=4500, output_rows=False)
    try:
        cs, ce = _gwas_windows(hip.p, 500)
        samples = [_effects(rng, hip.p, nnz, hip.dtype)[:2] for nnz in (37, 4200, 37)]
        rec.given(cs, ce, *[x for s in samples for x in s])
        _gwas_session(hip, rec, "grown", cs, ce, samples, True, False)
    finally:
        hip.close()


# per-marker effect covariances: MTBayesB at t = 2, 3 (Float32: sample, get; Float64: set, get, sample, get); MEGABAYESB, Float32 only,
# draws the diagonal
def _out_markercov(method, t):
    def run(precision, rec):
        hip, rng = _genotypes(precision, 24, OUT_P, rec, 1005)
        try:
            hip.init_state(method, t)
            for k in range(t):
                b = rng.standard_normal(hip.p).astype(hip.dtype)
                rec.given(b)
                hip.set_state(k, beta=b)
            scale = (np.diag([0.5, 0.375, 0.625]) + 0.0625)[:t, :t]
            if precision == 64:
                V = np.ascontiguousarray(rng.uniform(0.5, 2.0, (hip.p, t, t)))
                rec.given(V)
                _raw(hip, rec, "jwas_hip_set_marker_covariances_f64", V)
                assert rec.errors.pop() == [0, ""]
                rec.large("set_then_get", hip.marker_covariances())
            for it in (1, 2):
                hip.sample_marker_covariances(t + 3.0, scale, seed=59, iteration=it, marker_offset=100)
                rec.large(f"drawn{it}", hip.marker_covariances())
        finally:
            hip.close()
    return run


# 2-bit packed storage (Float32 only): the PackedCols view under mul_alpha, window_sums and the GWAS session
def _out_packed(precision, rec):
    import jwas_jl_amd as J
    from jwas_jl_amd import streaming as S
    rng = np.random.default_rng(1006)
    codes = rng.integers(0, 4, (OUT_N, OUT_P)).astype(np.uint8)          # (3 = missing)
    means = rng.uniform(0.2, 1.8, OUT_P).astype(np.float32)
    rec.given(codes, means)
    hip = J.HipEngine(0)
    try:
        hip.load_packed2bit(S.pack_2bit(codes), OUT_N, means, centered=True)
        hip.setup_blocks(64, "f64")
        hip.init_state("BayesC")
        samples = []
        for tag, nnz in OUT_NNZ:
            idx, val, a = _effects(rng, hip.p, nnz, hip.dtype)
            rec.given(a)
            samples.append((idx, val))
            hip.set_state(0, alpha=a)
            rec.large(f"{tag}_mul_alpha", hip.mul_alpha(0))
        counts = [0, 1, 7, 8, 9, 20]
        wptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        idx = rng.choice(hip.p, int(wptr[-1]), replace=False).astype(np.int32)
        v1, v2 = (rng.standard_normal(idx.size).astype(hip.dtype) for _ in range(2))
        rec.given(wptr, idx, v1, v2)
        rec.small("sums", np.concatenate(hip.window_sums(wptr, idx, v1)))
        rec.small("sums2", np.concatenate(hip.window_sums2(wptr, idx, v1, v2)))
        cs, ce = _gwas_windows(hip.p, 100)
        _gwas_session(hip, rec, "ebv", cs, ce, [samples[1], samples[0], samples[2]], True, False)
    finally:
        hip.close()


# the guards: every entry point of the other precision, a trait out of range, calls before init_state, output rows that do not exist, a
# GWAS sample after a reload.  Through the bare C ABI with buffers large enough for a call that a broken guard lets through.
_OUT_TWINS = ("get_xpx", "set_state", "get_state", "set_residual", "get_residual", "mul_alpha", "get_alpha_sparse", "mul_alpha_output",
              "window_sums", "window_sums2", "gwas_sample", "get_marker_covariances", "get_posterior")


def _out_guards(precision, rec):
    import ctypes as C
    import jwas_jl_amd as J
    hip, rng = _out_engine(precision, rec, 1007, "BayesC", 1, output_rows=False)
    X2 = np.asfortranarray(rng.integers(0, 3, (OUT_N, OUT_P)).astype(hip.dtype))
    Xout = np.asfortranarray(rng.integers(0, 3, (OUT_ROWS, OUT_P)).astype(hip.dtype))
    rec.given(X2, Xout)
    other, own = ("", "_f64") if precision == 64 else ("_f64", "")
    B = [np.zeros(16 * OUT_P) for _ in range(5)]                         # (8 bytes x 16 p each: any output of either precision fits)
    I = np.zeros(OUT_P, dtype=np.int32)
    wptr, nnz = np.array([0, 0], dtype=np.int32), C.c_int64(0)

    def surface(sfx, trait):                                             # the entry points that take a trait
        f = lambda nm: f"jwas_hip_{nm}{sfx}"
        _raw(hip, rec, f("set_state"), trait, B[0], B[1], B[2])
        _raw(hip, rec, f("get_state"), trait, B[0], B[1], B[2])
        _raw(hip, rec, f("set_residual"), trait, B[0])
        _raw(hip, rec, f("get_residual"), trait, B[0])
        _raw(hip, rec, f("mul_alpha"), trait, B[0])
        _raw(hip, rec, f("get_alpha_sparse"), trait, OUT_P, I, B[0], C.byref(nnz))
        _raw(hip, rec, f("mul_alpha_output"), trait, B[0])
        _raw(hip, rec, f("get_posterior"), trait, B[0], B[1], B[2])
    try:
        surface(other, 0)                                                # the other precision's entry points
        _raw(hip, rec, "jwas_hip_get_xpx" + other, B[0])
        _raw(hip, rec, "jwas_hip_load_output_dense_f" + ("32" if precision == 64 else "64"), Xout, OUT_ROWS, OUT_P, OUT_ROWS)
        _raw(hip, rec, "jwas_hip_window_sums" + other, 0, 1, wptr, I, B[0], B[1], B[2])
        _raw(hip, rec, "jwas_hip_window_sums2" + other, 0, 1, wptr, I, B[0], B[1], B[2], B[3], B[4], B[0], B[1])
        _raw(hip, rec, "jwas_hip_gwas_sample" + other, 0, I, B[0], B[1], B[2])
        _raw(hip, rec, "jwas_hip_get_marker_covariances" + other, B[0])
        if precision == 32:
            _raw(hip, rec, "jwas_hip_set_marker_covariances_f64", B[0])
        for trait in (1, -1):                                            # a trait out of range
            surface(own, trait)
            _raw(hip, rec, "jwas_hip_residual_sub_xalpha", trait)
        # output rows that do not exist
        _raw(hip, rec, "jwas_hip_mul_alpha_output" + own, 0, B[0])
        _raw(hip, rec, "jwas_hip_window_sums" + own, 1, 1, wptr, I, B[0], B[1], B[2])
        _raw(hip, rec, "jwas_hip_window_sums2" + own, 1, 1, wptr, I, B[0], B[1], B[2], B[3], B[4], B[0], B[1])
        cs, ce = _gwas_windows(hip.p, 100)
        rec.error(hip.gwas_begin, cs, ce, use_output_rows=True)
        # arguments and sessions
        rec.error(hip.accumulate, 0.5)
        rec.error(hip.marker_covariances)
        rec.error(hip.sample_marker_covariances, 4.0, np.eye(1), seed=1, iteration=1)
        rec.error(hip.gwas_sample, I[:0], B[0][:0].astype(hip.dtype))    # no session
        hip.gwas_begin(cs, ce)
        rec.error(hip.gwas_local_ebv)                                    # begun without local_ebv
        rec.error(hip.gwas_sample, np.array([5, 5], dtype=np.int32), np.ones(2, dtype=hip.dtype))      # not ascending
        rec.error(hip.gwas_sample, np.array([OUT_P], dtype=np.int32), np.ones(1, dtype=hip.dtype))     # out of range
        hip.load_dense(X2)                                               # a reload ends the session
        rec.error(hip.gwas_sample, I[:0], B[0][:0].astype(hip.dtype))
        hip.load_output_dense(Xout)
        hip.gwas_begin(cs, ce, use_output_rows=True)
        hip.load_output_dense(Xout)                                      # ... and so do new output rows
        rec.error(hip.gwas_sample, I[:0], B[0][:0].astype(hip.dtype))
        # before init_state (the reload above ended the chain)
        surface(own, 0)
        _raw(hip, rec, "jwas_hip_residual_sub_xalpha", 0)
        rec.error(hip.accumulate, 1)
    finally:
        hip.close()


OUTPUT_CASES = ("out_BayesC", "out_MTBayesC", "out_BayesR", "out_windows", "out_gwas", "out_markercov_t2", "out_markercov_t3",
                "out_markercov_mega", "out_packed", "out_guards")
OUTPUT_F32_ONLY = ("out_markercov_mega", "out_packed")


def output_keys():
    """(name, precision) of every record of tests/golden/output_side_golden.json."""
    return [(name, prec) for name in OUTPUT_CASES for prec in PRECISIONS if prec == 32 or name not in OUTPUT_F32_ONLY]


MTJ_CASES = ("mtj_t5", "mtj_t8")
MTJ_GUARDS = 7                           # the raw refusals of a record of MTJ_CASES, before the two that every session records
BLOCK_CASES = ("mega", "mega_chains", "rrm_c2", "rrm_c3", "rrm_c4", "gblup_t1", "gblup_t3_joint", "gblup_t3_diag")

_RUN = {"liability": _liability, "locpar": _locpar, "mtmiss": _mtmiss, "sem": _sem,
        "annot_BayesC": _annot("BayesC"), "annot_BayesR": _annot("BayesR"), "annot_tree": _annot("tree"),
        "mega": _mega, "mtj_t5": _mtj(5), "mtj_t8": _mtj(8), "mega_chains": _mega_chains, "rrm_c2": _rrm(2), "rrm_c3": _rrm(3), "rrm_c4": _rrm(4),
        "gblup_t1": _gblup(1, True, 0), "gblup_t3_joint": _gblup(3, False, 0), "gblup_t3_diag": _gblup(3, True, 1),
        "out_BayesC": _out_context("BayesC", 1), "out_MTBayesC": _out_context("MTBayesC", 3), "out_BayesR": _out_context("BayesR", 1),
        "out_windows": _out_windows, "out_gwas": _out_gwas, "out_markercov_t2": _out_markercov("MTBayesB", 2),
        "out_markercov_t3": _out_markercov("MTBayesB", 3), "out_markercov_mega": _out_markercov("MegaBayesB", 3), "out_packed": _out_packed,
        "out_guards": _out_guards}


def run_case(name, precision):
    rec = _Record()
    _RUN[name](precision, rec)
    return rec.done()
