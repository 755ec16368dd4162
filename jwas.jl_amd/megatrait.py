"""Mega-trait models: runMCMC on a model with 5 to 64 traits and constraint=true on both sides -- the host side of the reference's
megaBayesABC! / megaBayesC0! path (markers/BayesianAlphabet/BayesABC.jl:1-8; MCMC_BayesianAlphabet.jl:233-234,261-262): t independent
single-trait chains over one genotype matrix, with the marker sweep of ALL traits in one pass over the genotypes on the device
(csrc/mega.hpp, HipEngine.mega_*).  A driver of its own beside rrm.py and multigeno.py; mcmc.py keeps every model of 1 to 4 traits.

Per iteration, the order of mcmc.py:
  1. missing residuals: engine.mega_impute -- N(0, vare_kk) per missing cell, sampleMissingResiduals under a diagonal R          (DEVICE)
  2. location parameters, trait by trait, on the downloaded residual (MCMC_BayesianAlphabet.jl:196-220)                            (host)
  3. marker effects of every trait: engine.mega_sweep                                                                             (DEVICE)
  4. one pi per trait: samplePi(sum(delta_i), p) (MCMC_BayesianAlphabet.jl:299)                                                    (host)
  5. the diagonal marker-effect and residual variances (variance_components.jl:104-109 and the constraint branch of
     sample_marker_effect_variance)                                                                                               (host)
  6. every output_samples_frequency after burn-in: running means (device for the markers), the sample files
BayesC (estimatePi true or false) and RR-BLUP; Float32 or double_precision=True (the session's arithmetic is double in both; the
genotypes are stored in the context's element type); dense storage; complete records or records that miss some traits.  Everything
else raises (validate), before anything is written.

Speed (scripts/mega_bench.py, one MI355X, 20 000 x 100 000 Float32, pi = 0.95, blocks of 256): 22.9 ms per sweep at 4 traits, 25.3 at 8,
26.0 at 16, 31.3 at 32, 39.4 at 64, against 14.8 ms per 4 traits on the existing MegaBayesC sweep -- per trait the session is SLOWER
than that path below about 7 traits (0.65 of its speed at 4; interpolated between the measured 4 and 8, the two meet between 6 and
7 traits), 1.17 times as fast at 8 and 6.0 times at 64.  A model of 5 traits therefore pays about a quarter more per sweep here
than 5/4 of a four-trait sweep on the old kernel; it gets one run and one set of outputs instead of two."""
import time

import numpy as np

from ._lib import MEGA_MAX_BLOCK, MEGA_MAX_TRAITS
from .chain_output import MultiTraitOutputs, timing, write_id_files
from .mcmc import _design, _gibbs
from .session_driver import align_records, open_engine, phenotype_records, refuse_beyond_four_traits, refuse_engine

MEGA_METHODS = ("mega_begin", "mega_set_missing", "mega_set_residual", "mega_get_residual", "mega_get_state", "mega_impute", "mega_sweep",
                "mega_accumulate", "mega_posterior", "mega_mul_alpha", "mega_end")
MIN_TRAITS = 5                           # models of 1 to 4 traits stay on mcmc.py
DEFAULT_BLOCK = 256                      # the fastest of 64 / 128 / 256 at every number of traits measured (NOTES.md, "Mega-trait models")


def routes(model):
    """The models this driver takes or refuses: more than 4 traits."""
    return model.nModels >= MIN_TRAITS


def validate(model, df, *, fast_blocks=False, independent_blocks=False, causal_structure=False, RRM=False, location_parameters="auto",
             heterogeneous_residuals=False, starting_value=False, block_size=None, single_step_analysis=False, annotation_priors="host",
             engine=None):
    """Everything the device path does not run with more than 4 traits raises here, naming the argument, before any device work or
    folder creation."""
    t = model.nModels
    if t > MEGA_MAX_TRAITS:
        raise NotImplementedError(f"the device path runs at most {MEGA_MAX_TRAITS} traits (the model has {t} traits)")
    if not model.M:
        raise NotImplementedError("models without a genotype term have no marker sweep: use the reference")
    if len(model.M) > 1:
        raise NotImplementedError(f"several genotype categories with more than 4 traits ({t}) stay on the reference")
    Mi = model.M[0]
    if not (bool(Mi.G.constraint) and bool(model.R.constraint)):
        raise NotImplementedError(f"models with more than 4 traits ({t}) run on the device with constraint=True only (independent single-trait "
                                  "chains, megaBayesABC!): set constraint=True in BOTH get_genotypes and build_model; the joint "
                                  "2^t-state samplers stay on the reference")
    if Mi.method not in ("BayesC", "RR-BLUP"):
        raise NotImplementedError(f"method={Mi.method} with more than 4 traits stays on the reference (the device runs BayesC and RR-BLUP)")
    refuse_beyond_four_traits(model, Mi, one_pass="megaBayesABC! is one plain pass per iteration", annotation_priors=annotation_priors,
                              independent_blocks=independent_blocks, fast_blocks=fast_blocks, heterogeneous_residuals=heterogeneous_residuals,
                              location_parameters=location_parameters, causal_structure=causal_structure, RRM=RRM,
                              single_step_analysis=single_step_analysis, starting_value=starting_value)
    if isinstance(Mi.pi, dict):
        raise NotImplementedError("a Dict Pi over the joint states does not apply to constraint=True with more than 4 traits: pass one Pi, or one per trait")
    if np.ndim(Mi.pi) > 0 and np.size(Mi.pi) != t:
        raise ValueError(f"Pi must be a scalar or hold one value per trait ({t}), got {np.size(Mi.pi)} values.")
    if block_size is not None and not 1 <= int(block_size) <= MEGA_MAX_BLOCK:
        raise ValueError(f"block_size must be in [1, {MEGA_MAX_BLOCK}] for models with more than 4 traits.")
    if engine is not None:
        refuse_engine(engine, MEGA_METHODS, lambda missing: "models with more than 4 traits need an engine with the mega-trait sweep (" + missing
                      + " missing); the package has no CPU fallback")


def constraint_priors(model, phenovar, ftype=np.float32):
    """The starting values and the priors of the diagonal variances: the defaults of input_data_validation.jl:296-350 and
    tools4genotypes.jl:353-478, then R_constraint! and G_constraint! (input_data_validation.jl:530-559).  Returns a dict of
    per-trait vectors: vare, R_df, R_scale, G, G_df, G_scale, pi."""
    Mi, R, t = model.M[0], model.R, model.nModels
    phenovar = np.asarray(phenovar, dtype=np.float64)
    if R.val is False or R.val is None:                                  # input_data_validation.jl:296-350
        R.val = np.diag(phenovar * 0.5).astype(ftype)
        R.scale = np.asarray(R.val, dtype=np.float64) * (float(R.df) - t - 1)
    if Mi.G.val is False and Mi.genetic_variance.val is False:
        Mi.genetic_variance.val = np.diag(phenovar * 0.5)
    method, pi = Mi.method, Mi.pi
    if method == "RR-BLUP":                                              # input_data_validation.jl:24-31
        pi, Mi.estimatePi = 0.0, False
    pi_t = np.full(t, float(pi)) if np.ndim(pi) == 0 else np.asarray(pi, dtype=np.float64).reshape(-1).copy()
    if np.any(pi_t < 0.0) or np.any(pi_t >= 1.0):
        raise ValueError("Pi must be in [0, 1).")
    if Mi.G.val is False:                                                # genetic2marker, tools4genotypes.jl:426-438: the diagonal of
        Vg = np.atleast_2d(np.asarray(Mi.genetic_variance.val, dtype=np.float64))      # Vg ./ (sum2pq Pr(delta_i = 1, delta_j = 1))
        if Vg.shape != (t, t):
            raise ValueError(f"The genomic covariance matrix is not a {t} by {t} matrix.")
        Mi.G.val = np.diag(np.diag(Vg) / (Mi.sum2pq * (1.0 - pi_t)))
        if not np.all(np.isfinite(np.diag(Mi.G.val))) or np.any(np.diag(Mi.G.val) <= 0):
            raise ValueError("Marker effects covariance matrix is not postive definite! Please modify the argument: Pi.")
    Gdf = float(Mi.G.df)
    Mi.G.scale = np.asarray(Mi.G.val, dtype=np.float64) * (Gdf - t - 1)                                   # tools4genotypes.jl:414-418
    Rdf = float(R.df) - t                                                # R_constraint!
    R.scale = np.diag(np.diag(np.asarray(R.scale, dtype=np.float64)) / (Rdf - 1)) * (Rdf - 2) / Rdf
    R.val = np.diag(np.diag(np.asarray(R.val, dtype=ftype)))
    Gdf -= t                                                             # G_constraint!
    Mi.G.scale = np.diag(np.diag(np.asarray(Mi.G.scale, dtype=np.float64)) / (Gdf - 1)) * (Gdf - 2) / Gdf
    Mi.G.val = np.diag(np.diag(np.asarray(Mi.G.val, dtype=ftype)))
    return {"vare": np.diag(R.val).astype(np.float64), "R_df": Rdf, "R_scale": np.diag(R.scale).copy(),
            "G": np.diag(Mi.G.val).astype(np.float64), "G_df": Gdf, "G_scale": np.diag(Mi.G.scale).copy(), "pi": pi_t}


def run_megatrait(model, df, *, chain_length, burnin, output_samples_frequency, seed, double_precision, outputEBV, output_heritability,
                  output_folder, printout_frequency, missing_phenotypes=True, device=0, block_size=None, engine=None, printout_model_info=True,
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
    anyobs = np.isfinite(Yall).any(axis=0)
    if not np.isfinite(Yall[:, anyobs]).all() and not missing_phenotypes:
        raise ValueError("phenotypes are missing for some traits of some individuals; missing_phenotypes=false does not allow that")
    ph, rows, X, out_ids, out_rows, out_same = align_records(model, Mi, idcol, ph, Yall, ftype, outputEBV)
    n, p = X.shape
    write_id_files(output_folder, ph[idcol], Mi.obsID)
    Y = np.stack([ph[tr].to_numpy(dtype=np.float64) for tr in traits])  # t x n
    observed = np.isfinite(Y)
    has_missing = not observed.all()
    phenovar = np.array([np.var(Y[k][observed[k]].astype(ftype).astype(np.float64), ddof=1) for k in range(t)])
    Y = np.where(observed, Y, 0.0).astype(ftype).astype(np.float64)      # imputed before first use (residual.jl:52-73)

    # ---- priors
    pr = constraint_priors(model, phenovar, ftype)
    vare, Gval, pi_t = pr["vare"].copy(), pr["G"].copy(), pr["pi"].copy()
    Rdf, Rscale, Gdf, Gscale = pr["R_df"], pr["R_scale"], pr["G_df"], pr["G_scale"]
    if printout_model_info:
        print(f"Mega-trait analysis: {t} traits, constraint=true (independent single-trait chains over one genotype matrix).")
        print("The mean of the prior for the marker effects variances is:")
        print(np.round(Gval, 6))

    # ---- location parameters on the host, trait by trait
    Xf, labels = _design(model, ph, idcol)
    q = [x.shape[1] for x in Xf]
    off = np.concatenate([[0], np.cumsum(q)]).astype(int)
    sol = np.zeros(int(off[-1]))
    lhs = [x.T @ x for x in Xf]

    # ---- the device session
    engine, own_engine = open_engine(engine, device, double_precision, X, Mi, out_rows)
    engine.mega_begin(t, bs, 0)
    if has_missing:
        engine.mega_set_missing(~observed)
    engine.mega_set_residual(Y)                                          # ycorr = y: every starting value is zero

    # ---- accumulators and sample files: the variances are vectors here; the outputs hold them as the diagonal of a t x t matrix
    out = MultiTraitOutputs(model, output_folder, labels, off, sol, np.diag(vare), np.diag(Gval), pi_t if Mi.estimatePi else None, out_ids,
                            double_precision=double_precision, heritability=output_heritability,
                            marker_samples=output_samples_for_all_parameters or p <= 20000, diagonal_only=True)
    t_sweep, t0 = 0.0, time.time()
    with out.files:
        out.open()
        for it in range(1, chain_length + 1):
            if has_missing:                                              # 1. missing residuals (DEVICE)
                engine.mega_impute(iteration=it, seed=seed_int, vare=vare)
            if off[-1]:                                                  # 2. location parameters, trait by trait
                Rres = engine.mega_get_residual()
                for k in range(t):
                    if q[k]:
                        sk = sol[off[k]:off[k + 1]]
                        r = Rres[k] + Xf[k] @ sk
                        _gibbs(lhs[k], sk, Xf[k].T @ r, rng, float(vare[k]))
                        Rres[k] = r - Xf[k] @ sk
                engine.mega_set_residual(Rres)
            st = engine.mega_sweep(iteration=it, seed=seed_int, vare=vare, var_effect=Gval, pi=pi_t)      # 3. marker effects (DEVICE)
            t_sweep += st["step_ms"]
            if Mi.estimatePi:                                            # 4. samplePi per trait
                pi_t = np.array([rng.beta(p - st["sum_delta"][k] + 1.0, st["sum_delta"][k] + 1.0) for k in range(t)])
            if Mi.G.estimate_variance:                                   # 5. diagonal variances (variance_components.jl:104-109)
                Gval = np.array([(st["beta_ss"][k] + Gdf * Gscale[k]) / rng.chisquare(p + Gdf) for k in range(t)]).astype(ftype).astype(np.float64)
            if model.R.estimate_variance:
                vare = np.array([(st["resid_ss"][k] + Rdf * Rscale[k]) / rng.chisquare(n + Rdf) for k in range(t)]).astype(ftype).astype(np.float64)
            if it > burnin and (it - burnin) % output_samples_frequency == 0:      # 6. save
                ks = (it - burnin) / output_samples_frequency
                engine.mega_accumulate(ks)
                out.save(ks, sol, np.diag(vare), np.diag(Gval), pi_t, engine.mega_get_state()[0],
                         [np.asarray(engine.mega_mul_alpha(k, output_rows=not out_same), dtype=np.float64) for k in range(t)] if outputEBV else None)
            if it % printout_frequency == 0 and it > burnin:
                out.print_means(it)
    wall = time.time() - t0

    # ---- results (output.jl:108-212)
    res = out.tables(engine.mega_posterior, traits)
    res["_timing"] = timing(wall, t_sweep, chain_length, bs, n, p, ntraits=t)
    engine.mega_end()
    if own_engine:
        engine.close()
    return res
