"""Random regression models: runMCMC(model, df; RRM=Phi) -- the host side of RRM/MCMC_BayesianAlphabet_RRM.jl, a driver of its own
as in the reference, with the marker sweep (BayesABCRRM!, RRM/RRM.jl:101-158) on the device (csrc/rrm.hpp, HipEngine.rrm_*).

Longitudinal records: the first column of df holds the IDs, the column `time` the time point of every record, Phi (T x c) one row
per distinct time point (ascending) -- generatefullPhi builds the normalised Legendre columns.  Every marker carries c regression
coefficients; the "traits" of the outputs are the coefficients "1" ... "c" (MCMC_BayesianAlphabet_RRM.jl:19).

Per iteration, the reference's order (MCMC_BayesianAlphabet_RRM.jl:109-236):
  1. location parameters: the host scan on the records of rrm_get_residual / rrm_set_residual                (:113-116, host)
  2. marker effects: engine.rrm_sweep(...)                                                                    (:123-144, DEVICE)
  3. pi ~ Dirichlet(state counts + 1)                                                                         (:147-153, host)
  4. residual variance = (sum W^2 + df scale) / chi2(N_obs + df)                                              (:165-166, host)
  5. G ~ InverseWishart(df + p, scale + beta'beta)                                                            (:171-178, host)
  6. every output_samples_frequency after burn-in: running means (device for the markers), the sample files  (:194-236)
One trait, BayesC, estimatePi true or false, both precisions (the session's arithmetic is double in both; the genotypes are stored
in the context's element type).  Everything else raises (validate)."""
import time

import numpy as np

from ._lib import RRM_MAX_BLOCK, RRM_MAX_COEFF, RRM_MAX_TIMES, RRM_MIN_COEFF
from .chain_output import (GeneticVarianceSamples, Running, SampleFiles, covariance_table, ebv_tables, location_table,
                           marker_effects_table, pi_table, print_posterior_means, state_labels, write_tables)
from .mcmc import _design, _gibbs, genetic2marker

RRM_METHODS = ("rrm_begin", "rrm_set_residual", "rrm_get_residual", "rrm_sweep", "rrm_accumulate", "rrm_posterior", "rrm_mul_alpha", "rrm_end")


def generatefullPhi(timevec, ncoeff=3):
    """RRM.jl:24-39: one row per distinct time point (ascending), column k the normalised Legendre polynomial of degree k on the
    time points standardised to [-1, 1]: sqrt((2k + 1) / 2) P_k(q)."""
    times = np.sort(np.unique(np.asarray(timevec, dtype=np.float64)))
    if times.size < 2:
        raise ValueError("generatefullPhi needs at least two distinct time points.")
    ncoeff = int(ncoeff)
    if ncoeff < 1:
        raise ValueError("ncoeff must be >= 1.")
    q = 2.0 * (times - times[0]) / (times[-1] - times[0]) - 1.0
    Phi = np.empty((times.size, ncoeff))
    for k in range(ncoeff):                                              # Bonnet's recursion
        if k == 0:
            P, Pm = np.ones_like(q), None
        elif k == 1:
            P, Pm = q.copy(), P
        else:
            P, Pm = ((2 * k - 1) * q * P - (k - 1) * Pm) / k, P
        Phi[:, k] = np.sqrt((2 * k + 1) / 2.0) * P
    return Phi


def is_phi(RRM):
    """runMCMC(...; RRM): a 2-D numeric array is the Phi of a random regression model."""
    if isinstance(RRM, (bool, str)) or RRM is None:
        return False
    try:
        a = np.asarray(RRM)
    except Exception:
        return False
    return a.ndim == 2 and a.dtype != object and np.issubdtype(a.dtype, np.number) and not np.issubdtype(a.dtype, np.bool_)


def validate(model, df, Phi, *, fast_blocks=False, independent_blocks=False, causal_structure=False, location_parameters="auto",
             heterogeneous_residuals=False, starting_value=False, block_size=None, engine=None):
    """Everything the device path of RRM does not run raises here, before anything is written.  Returns Phi as T x c doubles."""
    Phi = np.ascontiguousarray(Phi, dtype=np.float64)
    T, c = Phi.shape
    if model.nModels != 1:
        raise NotImplementedError("RRM runs with one trait (the records of one longitudinal trait); multi-trait RRM stays on the reference")
    if not model.M:
        raise NotImplementedError("models without a genotype term have no marker sweep: use the reference")
    Mi = model.M[0]
    if Mi.method != "BayesC":
        raise NotImplementedError(f"RRM on the device runs BayesC only (got {Mi.method}); BayesA/B/R, RR-BLUP and BayesL stay on the reference")
    if not RRM_MIN_COEFF <= c <= RRM_MAX_COEFF:
        raise ValueError(f"RRM: the number of regression coefficients (columns of Phi) must be in [{RRM_MIN_COEFF}, {RRM_MAX_COEFF}], got {c}.")
    if not 1 <= T <= RRM_MAX_TIMES:
        raise ValueError(f"RRM: the number of time points (rows of Phi) must be in [1, {RRM_MAX_TIMES}], got {T}.")
    if not np.all(np.isfinite(Phi)):
        raise ValueError("RRM: Phi must be finite.")
    if isinstance(fast_blocks, (list, tuple, np.ndarray)):
        raise NotImplementedError("RRM runs on uniform blocks: fast_blocks as a vector of block starts is not supported")
    if independent_blocks:
        raise NotImplementedError("RRM does not run with independent_blocks")
    if getattr(model, "rndTrmVec", []):
        raise NotImplementedError("RRM with set_random effects stays on the reference")
    if any(tt != "continuous" for tt in model.traits_type):
        raise NotImplementedError("RRM with categorical or censored traits stays on the reference")
    if causal_structure is not False and causal_structure is not None:
        raise ValueError("RRM and causal_structure cannot be combined.")
    if Mi.annotations is not False:
        raise NotImplementedError("RRM with marker annotations stays on the reference")
    if Mi.alpha is not False or (starting_value is not False and starting_value is not None):
        raise NotImplementedError("RRM with marker starting values stays on the reference")
    if getattr(Mi, "storage_mode", "dense") == "stream":
        raise ValueError("storage=:stream MVP does not support random regression model (RRM).")         # input_data_validation.jl:97-98
    if heterogeneous_residuals:
        raise NotImplementedError("RRM does not run with heterogeneous_residuals (residual weights)")
    if location_parameters == "device":
        raise NotImplementedError('RRM samples its location parameters on the host: location_parameters="device" is not supported')
    if block_size is not None and not 1 <= int(block_size) <= RRM_MAX_BLOCK:
        raise ValueError(f"RRM: block_size must be in [1, {RRM_MAX_BLOCK}].")
    eng_ = engine if engine is not None else (Mi.device_backend if getattr(Mi, "storage_mode", "dense") == "device" else None)
    if eng_ is not None:
        missing = [m for m in RRM_METHODS if not hasattr(eng_, m)]
        if missing:
            raise NotImplementedError("RRM needs an engine with the random-regression sweep (" + ", ".join(missing) + " missing); the package has no CPU fallback")
        if hasattr(eng_, "comm_info") and eng_.comm_info()[1] > 1:
            raise NotImplementedError("RRM is not driven from marker or row shards")
    if getattr(Mi, "storage_mode", "dense") == "device":
        raise NotImplementedError("RRM needs the genotype rows of the phenotyped individuals on the host (get_genotypes), not device_genotypes")
    cols = [str(cn).strip() for cn in df.columns]
    if "time" not in cols:
        raise ValueError("RRM: the phenotype data need a column named time.")
    times = np.unique(np.asarray(df[df.columns[cols.index("time")]], dtype=np.float64))
    if times.size != T:
        raise ValueError(f"RRM: the time column holds {times.size} distinct time points but Phi has {T} rows.")
    return Phi


def _state_index(key):
    return sum((1 << q) for q, v in enumerate(key) if float(v) == 1.0)


def _prior_pi(Mi, c):
    """tools4genotypes.jl:357-373: without Pi all mass is on the all-ones state; a Dict maps 0/1 tuples (coefficient q at position q)."""
    ns = 1 << c
    if isinstance(Mi.pi, dict):
        pi = np.zeros(ns)
        for key, v in Mi.pi.items():
            if len(key) != c:
                raise ValueError(f"RRM: the keys of Pi must have {c} entries.")
            pi[_state_index(key)] = float(v)
    elif np.ndim(Mi.pi) == 0 and float(Mi.pi) == 0.0:
        pi = np.zeros(ns)
        pi[ns - 1] = 1.0
    else:
        pi = np.asarray(Mi.pi, dtype=np.float64).reshape(-1)
        if pi.size != ns:
            raise ValueError(f"RRM: Pi must be a Dict or hold {ns} values (one per state).")
    if abs(pi.sum() - 1.0) > 1e-8 or np.any(pi < 0):
        raise ValueError("Summation of probabilities of Pi is not equal to one.")
    return pi


def run_rrm(model, df, Phi, *, chain_length, burnin, output_samples_frequency, seed, double_precision, outputEBV, output_heritability,
            output_folder, printout_frequency, device=0, block_size=None, engine=None, printout_model_info=True):
    import pandas as pd
    from scipy.stats import invwishart
    Mi = model.M[0]
    T, c = Phi.shape
    ftype = np.float64 if double_precision else np.float32
    seed_int = 0 if seed is False else int(seed)
    rng = np.random.default_rng(seed_int)
    trait = model.lhsVec[0]
    coef_names = [str(q + 1) for q in range(c)]                          # MCMC_BayesianAlphabet_RRM.jl:19
    name = Mi.name

    # ---- records: sorted by time, then ID (input_data_validation.jl:254-256); IDs in first-appearance order (:22-27)
    df = df.rename(columns={cn: str(cn).strip() for cn in df.columns})
    idcol = df.columns[0]
    df = df.assign(**{idcol: df[idcol].astype(str).str.strip()})
    if trait not in df.columns:
        raise ValueError(f"{trait} is not found in the phenotype data.")
    df = df[np.isfinite(df[trait].astype(np.float64))]                   # records with a missing phenotype carry no information
    df = df.sort_values(["time", idcol], kind="stable").reset_index(drop=True)
    if df.duplicated([idcol, "time"]).any():
        raise ValueError("RRM: an individual has more than one record at a time point.")
    ids = list(pd.unique(df[idcol]))
    times = np.sort(df["time"].astype(np.float64).unique())
    if times.size != T:
        raise ValueError(f"RRM: the time column holds {times.size} distinct time points but Phi has {T} rows.")
    index = {g: i for i, g in enumerate(Mi.obsID)}
    unknown = [g for g in ids if g not in index]
    if unknown:
        raise ValueError(f"{unknown[0]} is not found!")                  # mkmat_incidence_factor, tools4genotypes.jl:340-344
    n, p = len(ids), Mi.nMarkers
    X = np.asfortranarray(np.asarray(Mi.genotypes)[[index[g] for g in ids], :].astype(ftype))
    rec_i = df[idcol].map({g: i for i, g in enumerate(ids)}).to_numpy(dtype=np.int64)
    rec_t = np.searchsorted(times, df["time"].to_numpy(dtype=np.float64))
    obs = np.zeros((T, n), dtype=bool)
    obs[rec_t, rec_i] = True
    y = df[trait].to_numpy(dtype=np.float64)
    nobs = y.size

    # ---- priors (input_data_validation.jl:296-350, tools4genotypes.jl:353-424)
    R = model.R
    Rdf = float(R.df)
    vary = float(np.var(y, ddof=1))
    if R.val is False or R.val is None:
        vare = vary * 0.5
        R.scale = vare * (Rdf - 2) / Rdf
    else:
        vare = float(R.val)
    if Mi.G.val is False and Mi.genetic_variance.val is False:
        Mi.genetic_variance.val = np.diag(np.full(c, vary * 0.5))        # :322-323
    pi = _prior_pi(Mi, c)
    Gdf = float(Mi.G.df)
    if Mi.G.val is False:
        gv = np.asarray(Mi.genetic_variance.val, dtype=np.float64)
        Mi.genetic_variance.val = np.diag(np.full(c, float(gv))) if gv.ndim == 0 or gv.size == 1 else gv
        if np.shape(Mi.genetic_variance.val) != (c, c):
            raise ValueError(f"The genomic covariance matrix is not a {c} by {c} matrix.")
        with np.errstate(divide="ignore", invalid="ignore"):
            Gval = genetic2marker(Mi, pi, "BayesC", t=c)
    else:
        gv = np.asarray(Mi.G.val, dtype=np.float64)
        Gval = np.diag(np.full(c, float(gv))) if gv.ndim == 0 or gv.size == 1 else gv
        if Gval.shape != (c, c):
            raise ValueError(f"The marker effects covariance matrix is not a {c} by {c} matrix.")
    Gval = np.asarray(Gval, dtype=np.float64)
    try:
        if not np.all(np.isfinite(Gval)):
            raise np.linalg.LinAlgError
        np.linalg.cholesky(Gval)
    except np.linalg.LinAlgError:
        raise ValueError("Marker effects covariance matrix is not postive definite! Please modify the argument: Pi.")      # :387-389
    Gval = (Gval + Gval.T) / 2
    Mi.G.scale = Gval * (Gdf - 2.0)                                      # :414-418 (Mi.ntraits = 1)
    if printout_model_info:
        print("The prior for marker effects covariance matrix is calculated from genetic covariance matrix and Π.")
        print("The mean of the prior for the marker effects covariance matrix is:")
        print(np.round(Gval, 6))

    # ---- location parameters on the host (MCMC_BayesianAlphabet_RRM.jl:113-116)
    Xf, labels = _design(model, df, idcol)
    Xf0 = Xf[0]
    q = Xf0.shape[1]
    sol = np.zeros(q)
    lhs = Xf0.T @ Xf0

    # ---- the device session
    own_engine = engine is None
    if own_engine:
        from .engine import HipEngine
        engine = HipEngine(device, precision=64 if double_precision else 32)
    out_ids = list(ids) if model.output_ID is False else [g for g in model.output_ID]
    if outputEBV:
        missing_out = [g for g in out_ids if g not in ids]
        if missing_out:
            raise NotImplementedError("RRM: outputEBV IDs without records (EBVs of individuals outside the phenotyped set) stay on the reference")
        out_rows = np.array([ids.index(g) for g in out_ids], dtype=np.int64)
    engine.load_dense(X)
    engine.rrm_begin(Phi, obs, int(block_size) if block_size is not None else 64)
    W0 = np.zeros((T, n))
    W0[rec_t, rec_i] = y                                                 # yfull = T'ycorr, starting values zero (:62-63)
    engine.rrm_set_residual(W0)

    # ---- accumulators and sample files (output.jl:320-437)
    run_sol, run_vare, run_varg = Running(sol), Running(vare), Running(Gval)
    run_pi = Running(pi) if Mi.estimatePi else None
    ebv_run = [Running(np.zeros(len(out_ids))) for _ in range(c)] if outputEBV else None
    cnames = [f"{a}_{b}" for a in coef_names for b in coef_names]
    fmt = "%.17g" if double_precision else "%.9g"                        # run_rrm: the marker rows follow the precision of the run
    genvar = None
    files = SampleFiles(output_folder)
    t_sweep, t0 = 0.0, time.time()
    with files:
        files.open("residual_variance", ["1"])                           # run_rrm: the column is named "1" (the other drivers: the trait)
        files.open(f"marker_effects_variances_{name}", cnames)
        files.open(f"pi_{name}", state_labels(c))
        for cn in coef_names:
            files.open(f"marker_effects_{name}_{cn}", Mi.markerID)
        if outputEBV:
            for cn in coef_names:
                files.open(f"EBV_{cn}", out_ids)
            if output_heritability:
                genvar = GeneticVarianceSamples(files, cnames)           # (no heritability for RRM: output.jl:360-364)
        for it in range(1, chain_length + 1):
            if q:                                                        # 1. location parameters
                W = engine.rrm_get_residual()
                r = W[rec_t, rec_i] + Xf0 @ sol
                _gibbs(lhs, sol, Xf0.T @ r, rng, float(vare))
                W[rec_t, rec_i] = r - Xf0 @ sol
                engine.rrm_set_residual(W)
            with np.errstate(divide="ignore"):                           # 2. marker effects (DEVICE)
                st = engine.rrm_sweep(iteration=it, seed=seed_int, vare=float(vare), G=Gval, log_pi=np.log(pi))
            t_sweep += st["step_ms"]
            if Mi.estimatePi:                                            # 3. samplePi
                pi = rng.dirichlet(st["state_counts"] + 1.0)
            if R.estimate_variance:                                      # 4. sample_variance(ycorr, length(ycorr), df, scale)
                vare = float((st["resid_ss"] + Rdf * R.scale) / rng.chisquare(nobs + Rdf))
            if Mi.G.estimate_variance:                                   # 5. sample_variance(beta, nMarkers, df, scale)
                S = np.asarray(Mi.G.scale, dtype=np.float64) + st["beta_ss"]
                Gval = np.asarray(invwishart.rvs(df=Gdf + p, scale=(S + S.T) / 2, random_state=rng), dtype=np.float64).reshape(c, c)
                Gval = (Gval + Gval.T) / 2
            if it > burnin and (it - burnin) % output_samples_frequency == 0:      # 6. save
                k = (it - burnin) / output_samples_frequency
                run_sol.add(sol, k)
                run_vare.add(vare, k)
                run_varg.add(Gval, k)
                if run_pi is not None:
                    run_pi.add(pi, k)
                engine.rrm_accumulate(k)
                files.row("residual_variance", [vare])
                files.row(f"marker_effects_variances_{name}", Gval.ravel())
                files.row(f"pi_{name}", pi)
                alpha = engine.rrm_get_state()[0]
                for qq, cn in enumerate(coef_names):
                    files.effects_row(f"marker_effects_{name}_{cn}", alpha[qq].astype(ftype), fmt)
                if outputEBV:
                    ebvs = [np.asarray(engine.rrm_mul_alpha(qq), dtype=np.float64)[out_rows] for qq in range(c)]
                    for qq, cn in enumerate(coef_names):
                        ebv_run[qq].add(ebvs[qq], k)
                        files.row(f"EBV_{cn}", ebvs[qq])
                    if genvar is not None:
                        genvar.add(ebvs)
            if it % printout_frequency == 0 and it > burnin:
                print_posterior_means(it, run_vare.mean)
    wall = time.time() - t0

    # ---- results (output.jl:108-212)
    out = {"location parameters": location_table(labels, [0], run_sol.mean, run_sol.sd()),
           "residual variance": covariance_table(["1"], run_vare)}
    # run_rrm: the SD from the moments as the session returns them (doubles)
    out[f"marker effects {name}"] = marker_effects_table([(cn, Mi.markerID) + tuple(engine.rrm_posterior(qq)) for qq, cn in enumerate(coef_names)],
                                                         sd_in_double=False)
    out[f"marker effects variance {name}"] = covariance_table(cnames, run_varg)
    if run_pi is not None:
        out[f"pi_{name}"] = pi_table(run_pi, state_labels(c))
    if outputEBV:
        out.update(ebv_tables(coef_names, out_ids, ebv_run))
        if genvar is not None:
            out.update(genvar.tables())
    write_tables(out, output_folder)
    out["_timing"] = {"wall_s": wall, "device_sweep_ms_total": t_sweep, "iterations": chain_length, "block_size": int(block_size) if block_size is not None else 64,
                      "n": n, "p": p, "ntimes": T, "ncoeff": c, "nrecords": nobs}
    engine.rrm_end()
    if own_engine:
        engine.close()
    return out
