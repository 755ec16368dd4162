"""The replayed calls behind tests/golden/session_golden.json: one small run of every device session (liabilities, location
parameters, missing traits, annotation priors, structural equation models), each in a Float32 and a Float64 context -- and, as
BLOCK_CASES behind tests/golden/block_session_golden.json, of the sessions that sweep blocks of markers themselves (mega-trait models,
several BayesR chains, random regression, GBLUP).

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


BLOCK_CASES = ("mega", "mega_chains", "rrm_c2", "rrm_c3", "rrm_c4", "gblup_t1", "gblup_t3_joint", "gblup_t3_diag")

_RUN = {"liability": _liability, "locpar": _locpar, "mtmiss": _mtmiss, "sem": _sem,
        "annot_BayesC": _annot("BayesC"), "annot_BayesR": _annot("BayesR"), "annot_tree": _annot("tree"),
        "mega": _mega, "mega_chains": _mega_chains, "rrm_c2": _rrm(2), "rrm_c3": _rrm(3), "rrm_c4": _rrm(4),
        "gblup_t1": _gblup(1, True, 0), "gblup_t3_joint": _gblup(3, False, 0), "gblup_t3_diag": _gblup(3, True, 1)}


def run_case(name, precision):
    rec = _Record()
    _RUN[name](precision, rec)
    return rec.done()
