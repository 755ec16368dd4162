"""Unconstrained multi-trait BayesC with 5 to 8 traits: runMCMC on a model with constraint=False (the default) in both get_genotypes
and build_model -- the host side of the reference's Gibbs sampler I (_MTBayesABC_samplerI!, markers/BayesianAlphabet/MTBayesABC.jl:57-127)
with a full marker-effect covariance G common to all markers, a full residual covariance R and Pi over the 2^t joint inclusion
states.  The marker sweep runs on the device (csrc/mtjoint.hpp, HipEngine.mtj_*) on the block form of the mega-trait session.  A
driver of its own beside megatrait.py (constraint=True, 5 to 64 traits); mcmc.py keeps every model of 1 to 4 traits.

Per iteration, the order of mcmc.py:
  1. location parameters on the downloaded residual: one Gibbs scan of the multi-trait equations kron(inv(R), X'X), as mcmc.py's
     host scan for 2 to 4 traits (the conditional of trait k reads the other traits' residuals through inv(R))                (host)
  2. marker effects of every trait: engine.mtj_sweep(inv(R), inv(G), log pi)                                                  (DEVICE)
  3. pi ~ Dirichlet(state counts + 1) when estimatePi                                                                          (host)
  4. G ~ InvWishart(df + p, scale + sum_j beta_j beta_j'),  R ~ InvWishart(df + n, scale + E E')                              (host)
  5. every output_samples_frequency after burn-in: running means (device for the markers), the sample files
BayesC (estimatePi true or false) and RR-BLUP (all mass on the all-ones state, estimatePi false); Float32 or double_precision=True
(the session's arithmetic is double in both); dense storage; complete records.  Everything else raises (validate), before anything
is written."""
import time

import numpy as np

from ._lib import MEGA_MAX_BLOCK, MTJ_MAX_TRAITS, MTJ_MIN_TRAITS
from .chain_output import MultiTraitOutputs, pi_labels, timing, write_id_files
from .mcmc import _design, _gibbs, genetic2marker
from .session_driver import align_records, open_engine, phenotype_records, refuse_beyond_four_traits, refuse_engine

MTJ_METHODS = ("mtj_begin", "mtj_set_residual", "mtj_get_residual", "mtj_get_state", "mtj_sweep", "mtj_accumulate", "mtj_posterior",
               "mtj_mul_alpha", "mtj_end")
DEFAULT_BLOCK = 256


def routes(model):
    """The models this driver takes or refuses: more than 4 traits with constraint=False on BOTH sides.  (One side only keeps the
    mega-trait driver's error.)"""
    return (model.nModels >= MTJ_MIN_TRAITS and len(model.M) >= 1 and not bool(model.R.constraint)
            and not any(bool(Mi.G.constraint) for Mi in model.M))


def inv_gauss_jordan(A):
    """inv(A) of a small matrix in double: Gauss-Jordan with partial pivoting in the operation order of the library's inv_small
    (csrc/ctx.hpp), so that every engine receives the same bits."""
    A = np.asarray(A, dtype=np.float64)
    t = A.shape[0]
    M = np.hstack([A.copy(), np.eye(t)])
    for c in range(t):
        piv = c
        for i in range(c + 1, t):
            if abs(M[i, c]) > abs(M[piv, c]):
                piv = i
        if M[piv, c] == 0.0:
            raise ValueError("the covariance matrix is singular")
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for i in range(t):
            if i != c and M[i, c] != 0.0:
                M[i] = M[i] - M[i, c] * M[c]
    return M[:, t:].copy()


def pi_states(pi, t):
    """Mi.pi -> the 2^t probabilities of the joint states (state index = sum_k delta_k << k), as mcmc.py for 2 to 4 traits: the scalar
    default puts all mass on the all-ones state, a Dict maps 0/1 vectors to probabilities, a vector of 2^t values is taken as it is."""
    ns = 1 << t
    if isinstance(pi, dict):
        tab = np.zeros(ns)
        for key, val in pi.items():
            key = tuple(float(v) for v in key)
            if len(key) != t or any(v not in (0.0, 1.0) for v in key):
                raise ValueError(f"Pi keys must be 0/1 vectors of length {t} (got {key})")
            tab[sum(1 << k for k in range(t) if key[k] == 1.0)] = float(val)
    elif np.ndim(pi) == 0:
        if float(pi) != 0.0:
            raise ValueError(f"Pi of an unconstrained model of {t} traits must be a Dict over the joint states or a vector of {ns} probabilities.")
        tab = np.zeros(ns)
        tab[ns - 1] = 1.0
    else:
        tab = np.asarray(pi, dtype=np.float64).reshape(-1).copy()
        if tab.size != ns:
            raise ValueError(f"Pi must hold one probability per joint state ({ns}), got {tab.size} values.")
    if np.any(tab < 0.0) or abs(tab.sum() - 1.0) > 1e-6:
        raise ValueError("Summation of probabilities of Pi is not equal to one.")
    return tab


def validate(model, df, *, fast_blocks=False, independent_blocks=False, causal_structure=False, RRM=False, location_parameters="auto",
             heterogeneous_residuals=False, starting_value=False, block_size=None, single_step_analysis=False, annotation_priors="host",
             engine=None):
    """Everything the joint session does not run raises here, naming the argument, before any device work or folder creation."""
    t = model.nModels
    if engine is not None and not isinstance(engine, (list, tuple)):
        refuse_engine(engine, MTJ_METHODS, lambda missing: f"without the joint multi-trait session, models with more than 4 traits ({t}) run on the "
                      "device with constraint=True in BOTH get_genotypes and build_model only; this engine lacks " + missing
                      + " and the package has no CPU fallback")
    if t > MTJ_MAX_TRAITS:
        raise NotImplementedError(f"models with more than {MTJ_MAX_TRAITS} traits (t = {t}) run on the device with constraint=True in BOTH "
                                  "get_genotypes and build_model only: the joint session holds 2^t states, t <= 8")
    if len(model.M) > 1:
        raise NotImplementedError(f"several genotype categories with more than 4 traits ({t}) stay on the reference")
    Mi = model.M[0]
    if Mi.method not in ("BayesC", "RR-BLUP"):
        raise NotImplementedError(f"method={Mi.method} with more than 4 traits stays on the reference (the device runs BayesC and RR-BLUP)")
    sampler = getattr(Mi, "multi_trait_sampler", "I")
    if sampler == "II" or (sampler == "auto" and isinstance(Mi.pi, dict) and len(Mi.pi) != (1 << t)):
        raise NotImplementedError("multi_trait_sampler=:II (or a Dict Pi that does not list all 2^t joint states) with more than 4 traits "
                                  "stays on the reference: the device runs Gibbs sampler I")
    if isinstance(Mi.pi, dict) and len(Mi.pi) != (1 << t):
        raise NotImplementedError(f"a Dict Pi that does not list all 2^t = {1 << t} joint states selects sampler II (multi_trait_sampler), "
                                  "which stays on the reference with more than 4 traits")
    refuse_beyond_four_traits(model, Mi, one_pass="sampler I is one plain pass per iteration", annotation_priors=annotation_priors,
                              independent_blocks=independent_blocks, fast_blocks=fast_blocks, heterogeneous_residuals=heterogeneous_residuals,
                              location_parameters=location_parameters, causal_structure=causal_structure, RRM=RRM,
                              single_step_analysis=single_step_analysis, starting_value=starting_value)
    if block_size is not None and not 1 <= int(block_size) <= MEGA_MAX_BLOCK:
        raise ValueError(f"block_size must be in [1, {MEGA_MAX_BLOCK}] for models with more than 4 traits.")
    pi_states(0.0 if Mi.method == "RR-BLUP" else Mi.pi, t)
    # records that miss some traits: sampleMissingResiduals under a full R is not on this path
    traits = [tr for tr in model.lhsVec if tr in df.columns]
    if len(traits) == t:
        obs = np.isfinite(df[traits].to_numpy(dtype=np.float64))
        some = obs.any(axis=1)
        if not obs[some].all():
            raise NotImplementedError("missing_phenotypes: records that miss some traits, with more than 4 traits and full covariances, "
                                      "stay on the reference (complete records only)")


def joint_priors(model, phenovar, ftype=np.float32):
    """The starting values and the priors of the full covariances: the defaults of input_data_validation.jl:296-350 and
    tools4genotypes.jl:353-478, as mcmc.py:600-720 for 2 to 4 traits.  Returns a dict: vare, R_df, R_scale, G, G_df, G_scale (t x t)
    and pi (2^t)."""
    Mi, R, t = model.M[0], model.R, model.nModels
    phenovar = np.asarray(phenovar, dtype=np.float64)
    if R.val is False or R.val is None:
        R.val = np.diag(phenovar * 0.5).astype(ftype)
        R.scale = np.asarray(R.val, dtype=np.float64) * (float(R.df) - t - 1)
    if Mi.G.val is False and Mi.genetic_variance.val is False:
        Mi.genetic_variance.val = np.diag(phenovar * 0.5)
    if Mi.method == "RR-BLUP":                                           # input_data_validation.jl:24-31: BayesC with every marker in the model
        pi, Mi.estimatePi = pi_states(0.0, t), False
    else:
        pi = pi_states(Mi.pi, t)
    if Mi.G.val is False:
        Vg = np.atleast_2d(np.asarray(Mi.genetic_variance.val, dtype=np.float64))
        if Vg.shape != (t, t):
            raise ValueError(f"The genomic covariance matrix is not a {t} by {t} matrix.")
        with np.errstate(divide="ignore", invalid="ignore"):
            Mi.G.val = genetic2marker(Mi, pi, "BayesC", t)
        if not np.all(np.isfinite(Mi.G.val)) or np.any(np.linalg.eigvalsh(Mi.G.val) <= 0):
            raise ValueError("Marker effects covariance matrix is not postive definite! Please modify the argument: Pi.")
    Gdf = float(Mi.G.df)
    Mi.G.scale = np.asarray(Mi.G.val, dtype=np.float64) * (Gdf - t - 1)  # tools4genotypes.jl:414-418
    return {"vare": np.asarray(R.val, dtype=ftype).astype(np.float64), "R_df": float(R.df), "R_scale": np.asarray(R.scale, dtype=np.float64),
            "G": np.asarray(Mi.G.val, dtype=ftype).astype(np.float64), "G_df": Gdf, "G_scale": np.asarray(Mi.G.scale, dtype=np.float64), "pi": pi}


def log_pi(pi):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(pi, dtype=np.float64))                 # (0 -> -inf: the state is never entered)


def draw_covariance(rng, df, S, ftype):
    """InvWishart(df, S) with S made symmetric, rounded to the element type of the run."""
    from scipy.stats import invwishart
    t = S.shape[0]
    return np.asarray(invwishart.rvs(df=df, scale=(S + S.T) / 2, random_state=rng), dtype=ftype).reshape(t, t).astype(np.float64)


def run_mtjoint(model, df, *, chain_length, burnin, output_samples_frequency, seed, double_precision, outputEBV, output_heritability,
                output_folder, printout_frequency, device=0, block_size=None, engine=None, printout_model_info=True,
                output_samples_for_all_parameters=False):
    Mi = model.M[0]
    t = model.nModels
    ftype = np.float64 if double_precision else np.float32
    if not double_precision and getattr(Mi.genotypes, "dtype", None) == np.float64:
        raise NotImplementedError("Float64 genotypes (get_genotypes(double_precision=true)) run with runMCMC(double_precision=true)")
    seed_int = 0 if seed is False else int(seed)
    rng = np.random.default_rng(seed_int)
    traits = list(model.lhsVec)
    bs = int(block_size) if block_size is not None else DEFAULT_BLOCK

    # ---- align phenotypes and genotypes (input_data_validation.jl:198-294, tools4genotypes.jl:288-323)
    idcol, ph, Yall = phenotype_records(df, traits)
    ph, rows, X, out_ids, out_rows, out_same = align_records(model, Mi, idcol, ph, Yall, ftype, outputEBV)
    n, p = X.shape
    write_id_files(output_folder, ph[idcol], Mi.obsID)
    Y = np.stack([ph[tr].to_numpy(dtype=np.float64) for tr in traits]).astype(ftype).astype(np.float64)     # t x n, complete (validate)
    phenovar = np.array([np.var(Y[k], ddof=1) for k in range(t)])

    # ---- priors
    pr = joint_priors(model, phenovar, ftype)
    vare, Gval, pi = pr["vare"].copy(), pr["G"].copy(), pr["pi"].copy()
    Rdf, Rscale, Gdf, Gscale = pr["R_df"], pr["R_scale"], pr["G_df"], pr["G_scale"]
    if printout_model_info:
        print(f"Multi-trait analysis: {t} traits, Gibbs sampler I with full marker-effect and residual covariances.")
        print("The mean of the prior for the marker effects covariance matrix is:")
        print(np.round(Gval, 6))

    # ---- location parameters on the host: the multi-trait equations kron(inv(R), X'X)
    Xf, labels = _design(model, ph, idcol)
    q = [x.shape[1] for x in Xf]
    off = np.concatenate([[0], np.cumsum(q)]).astype(int)
    sol = np.zeros(int(off[-1]))
    lhs_blocks = [[Xf[k].T @ Xf[l] for l in range(t)] for k in range(t)]

    # ---- the device session
    engine, own_engine = open_engine(engine, device, double_precision, X, Mi, out_rows)
    engine.mtj_begin(t, bs)
    engine.mtj_set_residual(Y)                                           # ycorr = y: every starting value is zero

    # ---- accumulators and sample files
    out = MultiTraitOutputs(model, output_folder, labels, off, sol, vare, Gval, pi if Mi.estimatePi else None, out_ids,
                            double_precision=double_precision, heritability=output_heritability,
                            marker_samples=output_samples_for_all_parameters or p <= 20000, diagonal_only=False)
    t_sweep, t0 = 0.0, time.time()
    with out.files:
        out.open()
        for it in range(1, chain_length + 1):
            Rinv = inv_gauss_jordan(vare)
            if off[-1]:                                                  # 1. location parameters (mcmc.py's multi-trait host scan)
                res = engine.mtj_get_residual()
                rr = [res[k] + Xf[k] @ sol[off[k]:off[k + 1]] for k in range(t)]
                A = np.block([[Rinv[k, l] * lhs_blocks[k][l] for l in range(t)] for k in range(t)])
                b = np.concatenate([Xf[k].T @ sum(Rinv[k, l] * rr[l] for l in range(t)) for k in range(t)])
                _gibbs(A, sol, b, rng, None)
                engine.mtj_set_residual(np.stack([rr[k] - Xf[k] @ sol[off[k]:off[k + 1]] for k in range(t)]))
            st = engine.mtj_sweep(iteration=it, seed=seed_int, rinv=Rinv, ginv=inv_gauss_jordan(Gval), log_pi=log_pi(pi))      # 2. (DEVICE)
            t_sweep += st["step_ms"]
            if Mi.estimatePi:                                            # 3. mcmc.py:1384
                pi = rng.dirichlet(st["state_counts"] + 1.0)
            if Mi.G.estimate_variance:                                   # 4. mcmc.py:1416-1420
                Gval = draw_covariance(rng, Gdf + p, Gscale + st["beta_ss"], ftype)
            if model.R.estimate_variance:                                # mcmc.py:1461-1463
                vare = draw_covariance(rng, Rdf + n, Rscale + st["resid_cp"], ftype)
            if it > burnin and (it - burnin) % output_samples_frequency == 0:      # 5. save
                ks = (it - burnin) / output_samples_frequency
                engine.mtj_accumulate(ks)
                out.save(ks, sol, vare, Gval, pi, engine.mtj_get_state()[0],
                         [np.asarray(engine.mtj_mul_alpha(k, output_rows=not out_same), dtype=np.float64) for k in range(t)] if outputEBV else None)
            if it % printout_frequency == 0 and it > burnin:
                out.print_means(it)
    wall = time.time() - t0

    # ---- results (output.jl:108-212)
    res = out.tables(engine.mtj_posterior, pi_labels(t, "BayesC"))
    res["_timing"] = timing(wall, t_sweep, chain_length, bs, n, p, ntraits=t)
    engine.mtj_end()
    if own_engine:
        engine.close()
    return res
