"""Several chains of one single-trait model in one device session: runMCMC(..., chains=K) with K in 2..64, and the potential scale
reduction factor of Gelman and Rubin over the chains.  A driver of its own beside megatrait.py, on the same session (csrc/mega.hpp,
HipEngine.mega_*): a chain is a trait whose record is the same, so the genotypes are uploaded once, x'x and the block Grams are
formed once, and one pass over a block of the genotypes serves the right-hand sides of ALL chains.

Per iteration, the order of mcmc.run_chain, chain by chain on the host and all chains at once on the device:
  1. location parameters of every chain on its downloaded residual (MCMC_BayesianAlphabet.jl:196-220)                           (host)
  2. marker effects of every chain: engine.mega_sweep (BayesC, RR-BLUP) or engine.mega_sweep_r (BayesR)                          (DEVICE)
  3. pi: Beta(p - sum delta + 1, sum delta + 1) for BayesC, dirichlet(class counts + 1) for BayesR                               (host)
  4. the marker-effect variance: BayesC (alpha'alpha + df scale) / chi2(sum delta + df); BayesR (ssq + df scale) / chi2(nnz + df)   (host)
  5. the residual variance (r'r + df scale) / chi2(n + df)                                                                      (host)
  6. every output_samples_frequency after burn-in: running means (device for the markers), the sample files of every chain
Draws.  Chain k has the Philox trait id first_chain + k on the device; its host draws come from
np.random.default_rng([seed, first_chain + k]) in the order above.  Chain k of a K-chain run therefore equals that chain run alone
(chains=2, first_chain=k takes its first chain) in every output file.  The priors are those of the single-chain driver
(genetic2marker, the default variances of input_data_validation.jl:296-350).

ALL CHAINS START FROM THE REFERENCE'S STARTING STATE (effects 0, the prior means of the variances, the given Pi).  The potential
scale reduction factor was designed for over-dispersed starting points; with equal starts it can only detect chains that drift
apart, not a mode that every chain missed.  Over-dispersed starting values are out of scope here (starting_value raises).

Scope: one trait, one genotype category; BayesC (estimatePi true or false), RR-BLUP, BayesR with the default or a given gamma
(bayesr_gamma); dense Float32 or Float64 genotypes, the session's arithmetic in double; uniform blocks of at most 256 markers
(block_size, default 256); location parameters on the host; outputEBV(model, IDs).  Everything else raises NotImplementedError naming
the argument (validate), before any engine call and before the folder is written.

Output: output_folder/chain_<id>/ holds the reference's files of each chain (id = first_chain + k); output_folder/PSRF.txt one row per
marker effect (k_mega_psrf, on the device from the running moments) plus the scalar parameters (pi or the four class probabilities,
the marker-effect variance, the residual variance: the same formula on the host from the saved samples); PSRF_summary.txt the
maximum, the 99th percentile and the count above 1.1 over the markers with a finite value; the usual tables pooled over the chains
(the mean of the chain means, the SD from the pooled second moment) at the top level."""
import os
import time

import numpy as np

from ._lib import MEGA_MAX_BLOCK, MEGA_MAX_TRAITS
from .chain_output import (GeneticVarianceSamples, Running, SampleFiles, covariance_table, ebv_tables, location_table,
                           marker_effects_table, pi_labels, pi_table, print_posterior_means, term_sample_columns, timing, write_id_files,
                           write_tables)
from .mcmc import BAYESR_GAMMA, _design, _gibbs, genetic2marker
from .session_driver import align_records, not_false, open_engine, phenotype_records

CHAIN_METHODS = ("mega_begin", "mega_set_residual", "mega_get_residual", "mega_get_state", "mega_sweep", "mega_sweep_r", "mega_accumulate",
                 "mega_accumulate_r", "mega_psrf", "mega_posterior", "mega_mul_alpha", "mega_end")
MAX_CHAINS = MEGA_MAX_TRAITS
DEFAULT_BLOCK = 256
PSRF_THRESHOLD = 1.1


def check_chains(chains):
    """chains as runMCMC takes it: 1 (today's path) or 2..64."""
    if isinstance(chains, bool) or not isinstance(chains, (int, np.integer)) or not 1 <= int(chains) <= MAX_CHAINS:
        raise ValueError(f"chains must be an integer in [1, {MAX_CHAINS}] (got {chains!r}).")
    return int(chains)


def validate(model, df, *, chains, first_chain=0, fast_blocks=False, independent_blocks=False, causal_structure=False, RRM=False,
             location_parameters="auto", heterogeneous_residuals=False, starting_value=False, block_size=None, single_step_analysis=False,
             annotation_priors="host", bayesr_gamma=None, engine=None):
    """Everything the several-chain driver does not run raises here, naming the argument, before any device work or folder creation."""
    if isinstance(first_chain, bool) or not isinstance(first_chain, (int, np.integer)) or int(first_chain) < 0 or int(first_chain) + chains > (1 << 24):
        raise ValueError("first_chain must be an integer >= 0 with first_chain + chains <= 2^24.")
    if model.nModels != 1:
        raise NotImplementedError(f"chains={chains} runs single-trait models (the model has {model.nModels} traits)")
    if not model.M:
        raise NotImplementedError("models without a genotype term have no marker sweep: use the reference")
    if len(model.M) > 1:
        raise NotImplementedError(f"chains={chains} with several genotype categories is not supported")
    Mi = model.M[0]
    if Mi.method not in ("BayesC", "RR-BLUP", "BayesR"):
        raise NotImplementedError(f"chains={chains} with method={Mi.method} is not supported (the session runs BayesC, RR-BLUP and BayesR)")
    if Mi.annotations is not False:
        raise NotImplementedError(f"chains={chains} with annotations is not supported")
    if annotation_priors != "host":
        raise NotImplementedError(f'annotation_priors="device" does not apply to chains={chains}')
    mode = getattr(Mi, "storage_mode", "dense")
    if mode == "stream":
        raise NotImplementedError(f"chains={chains} with storage=:stream is not supported (dense storage only)")
    if mode == "device":
        raise NotImplementedError(f"chains={chains} with device_genotypes is not supported: pass the genotypes through get_genotypes")
    if independent_blocks:
        raise NotImplementedError(f"chains={chains} with independent_blocks is not supported")
    if fast_blocks is not False:
        raise NotImplementedError(f"chains={chains} with fast_blocks is not supported (one plain pass per iteration)")
    if heterogeneous_residuals:
        raise NotImplementedError(f"chains={chains} with heterogeneous_residuals (residual weights) is not supported")
    if location_parameters == "device":
        raise NotImplementedError(f'chains={chains} with location_parameters="device" is not supported: they are sampled on the host')
    if getattr(model, "rndTrmVec", []):
        raise NotImplementedError(f"chains={chains} with set_random effects is not supported")
    if any(tt != "continuous" for tt in model.traits_type):
        raise NotImplementedError(f"chains={chains} with categorical_trait / censored_trait is not supported")
    if not_false(causal_structure):
        raise NotImplementedError(f"chains={chains} with causal_structure is not supported")
    if not_false(RRM):
        raise NotImplementedError(f"chains={chains} with RRM is not supported")
    if not_false(single_step_analysis):
        raise NotImplementedError(f"chains={chains} with single_step_analysis is not supported")
    if Mi.alpha is not False or not_false(starting_value):
        raise NotImplementedError(f"chains={chains} with starting_value (marker or location-parameter starting values) is not supported: "
                                  "every chain starts from the reference's starting state")
    if getattr(Mi.G, "estimate_scale", False):
        raise NotImplementedError(f"chains={chains} with estimate_scale is not supported")
    if isinstance(Mi.pi, dict):
        raise NotImplementedError("a Dict Pi is for multi-trait analyses only")
    if Mi.method == "BayesR":
        if not (np.ndim(Mi.pi) == 0 and (Mi.pi is False or float(Mi.pi) == 0.0)) and np.shape(Mi.pi) != (4,):
            raise ValueError("BayesR Pi must have length 4.")
    elif np.ndim(Mi.pi) != 0:
        raise NotImplementedError(f"chains={chains} with a marker-level Pi is not supported")
    if bayesr_gamma is not None:
        if Mi.method != "BayesR":
            raise ValueError("bayesr_gamma applies to method=BayesR only.")
        g = np.asarray(bayesr_gamma, dtype=np.float64)
        if g.shape != (4,) or g[0] != 0.0 or not np.all(np.isfinite(g[1:]) & (g[1:] > 0)):
            raise ValueError("bayesr_gamma must hold 4 values: 0 for the null class, then three positive finite multipliers.")
    if block_size is not None and not 1 <= int(block_size) <= MEGA_MAX_BLOCK:
        raise ValueError(f"block_size must be in [1, {MEGA_MAX_BLOCK}] for chains={chains}.")
    if engine is not None:
        missing = [m for m in CHAIN_METHODS if not hasattr(engine, m)]
        if missing:
            raise NotImplementedError(f"chains={chains} needs an engine with the several-chain session (" + ", ".join(missing)
                                      + " missing); the package has no CPU fallback")
        if hasattr(engine, "comm_info") and engine.comm_info()[1] > 1:
            raise NotImplementedError(f"chains={chains} is not driven from marker or row shards")


def psrf_rows(x):
    """The potential scale reduction factor of scalar parameters from their saved samples, x [K x N x q] -> q values: the formula
    of k_mega_psrf (csrc/mega.hpp) from the sample means m_k and means of squares q_k; NaN where W == 0 or with fewer than 2 samples."""
    x = np.asarray(x, dtype=np.float64)
    K, N = x.shape[0], x.shape[1]
    if N < 2:
        return np.full(x.shape[2], np.nan)
    m, q = x.mean(axis=1), (x * x).mean(axis=1)
    W = (N / (N - 1.0) * (q - m * m)).sum(axis=0) / K
    BN = ((m - m.sum(axis=0) / K) ** 2).sum(axis=0) / (K - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(W == 0.0, np.nan, np.sqrt(((N - 1.0) / N * W + BN) / W))


def _pooled(runs):
    """A Running whose mean is the mean of the chain means and whose second moment is the mean of theirs."""
    out = Running(runs[0].mean)
    out.mean = np.mean([r.mean for r in runs], axis=0)
    out.mean2 = np.mean([r.mean2 for r in runs], axis=0)
    return out


class _Chain:
    """The host state of one chain."""

    def __init__(self, cid, seed_int, folder, sol, vare, Gval, pi, nout):
        self.id = cid
        self.rng = np.random.default_rng([seed_int, cid])
        self.folder = folder
        self.sol, self.vare, self.Gval, self.pi = sol.copy(), float(vare), float(Gval), np.array(pi, dtype=np.float64)
        self.run_sol, self.run_vare, self.run_varg = Running(sol), Running(np.zeros(1)), Running(np.zeros(1))
        self.run_pi = Running(np.atleast_1d(self.pi))
        self.ebv_run = Running(np.zeros(nout)) if nout is not None else None
        self.saved = []                                                 # per saved sample: pi..., the effect variance, the residual variance
        self.genvar = None


def run_chains(model, df, *, chains, first_chain=0, chain_length, burnin, output_samples_frequency, seed, double_precision, outputEBV,
               output_heritability, output_folder, printout_frequency, device=0, block_size=None, bayesr_gamma=None, engine=None,
               printout_model_info=True, output_samples_for_all_parameters=False):
    import pandas as pd
    Mi = model.M[0]
    K, first = int(chains), int(first_chain)
    ftype = np.float64 if double_precision else np.float32
    if not double_precision and getattr(Mi.genotypes, "dtype", None) == np.float64:
        raise NotImplementedError("Float64 genotypes (get_genotypes(double_precision=true)) run with runMCMC(double_precision=true)")
    seed_int = 0 if seed is False else int(seed)
    name, trait = Mi.name, model.lhsVec[0]
    bs = int(block_size) if block_size is not None else DEFAULT_BLOCK
    method = Mi.method
    bayesr = method == "BayesR"
    gamma = np.asarray(BAYESR_GAMMA if bayesr_gamma is None else bayesr_gamma, dtype=np.float64)

    # ---- align phenotypes and genotypes (input_data_validation.jl:198-294, tools4genotypes.jl:288-323)
    idcol, ph, Yall = phenotype_records(df, [trait])
    ph, rows, X, out_ids, out_rows, out_same = align_records(model, Mi, idcol, ph, Yall, ftype, outputEBV)
    n, p = X.shape
    y = ph[trait].to_numpy(dtype=ftype)
    phenovar = float(np.var(y.astype(np.float64), ddof=1))
    y = y.astype(np.float64)

    # ---- priors, as the single-chain driver forms them (input_data_validation.jl:296-350, tools4genotypes.jl:353-478)
    R = model.R
    if R.val is False or R.val is None:
        R.val = ftype(phenovar * 0.5)
        R.scale = float(R.val) * (float(R.df) - 2) / float(R.df)
    if Mi.G.val is False and Mi.genetic_variance.val is False:
        Mi.genetic_variance.val = phenovar * 0.5
    pi = Mi.pi
    if bayesr and np.ndim(pi) == 0:                                      # :375-377
        pi = np.array([0.95, 0.03, 0.015, 0.005])
    if method == "RR-BLUP":                                              # input_data_validation.jl:24-31
        if not (pi is False or pi == 0.0):
            print("RR-BLUP runs with π = false.")
        pi, Mi.estimatePi = 0.0, False
    if bayesr:
        pi = np.asarray(pi, dtype=np.float64)
        if np.any(pi < 0.0) or abs(pi.sum() - 1.0) > 1e-8:
            raise ValueError("BayesR Pi must hold 4 probabilities that sum to 1.")
    elif not 0.0 <= float(pi) < 1.0:
        raise ValueError("Pi must be in [0, 1).")
    if Mi.G.val is False:
        if bayesr and bayesr_gamma is not None:                          # genetic2marker's BayesR branch with the given gamma
            denom = Mi.sum2pq * float((gamma * pi).sum())
            if not denom > 0:
                raise ValueError("BayesR implied variance denominator must be positive.")
            Mi.G.val = float(Mi.genetic_variance.val) / denom
        else:
            Mi.G.val = genetic2marker(Mi, pi, "BayesR" if bayesr else "BayesC", 1)
        if not Mi.G.val > 0:
            raise ValueError("Marker effects variance is negative!")
    Gdf, Rdf = float(Mi.G.df), float(R.df)
    Mi.G.scale = np.float64(Mi.G.val) * (Gdf - 2) / Gdf                  # :414-418
    vare0, Gval0 = float(ftype(R.val)), float(ftype(Mi.G.val))
    if printout_model_info:
        print(f"{K} chains of one model ({method}), Philox ids {first} .. {first + K - 1}, in one device session.")
        print(f"The prior mean of the marker-effect variance is {Gval0:.6g}, of the residual variance {vare0:.6g}.")

    # ---- location parameters on the host
    Xf, labels = _design(model, ph, idcol)
    Xf0 = Xf[0]
    q = Xf0.shape[1]
    off = np.array([0, q])
    lhs = Xf0.T @ Xf0

    # ---- the device session
    engine, own_engine = open_engine(engine, device, double_precision, X, Mi, out_rows)
    engine.mega_begin(K, bs, first)
    engine.mega_set_residual(np.tile(y, (K, 1)))                         # ycorr = y in every chain: every starting value is zero

    # ---- chains, accumulators and sample files (output.jl:320-437)
    os.makedirs(output_folder, exist_ok=True)
    ch = []
    for k in range(K):
        folder = os.path.join(output_folder, f"chain_{first + k}")
        os.makedirs(folder)
        write_id_files(folder, ph[idcol], Mi.obsID)
        ch.append(_Chain(first + k, seed_int, folder, np.zeros(q), vare0, Gval0, pi, len(out_ids) if outputEBV else None))
    write_id_files(output_folder, ph[idcol], Mi.obsID)
    cov = [trait]
    npi = 4 if bayesr else 1
    term_cols = term_sample_columns(model, labels, off)
    write_marker_samples = output_samples_for_all_parameters or p <= 20000
    fmt = "%.17g" if double_precision else "%.9g"
    accumulate = engine.mega_accumulate_r if bayesr else engine.mega_accumulate
    nsaved = 0
    t_sweep, t0 = 0.0, time.time()
    files = [SampleFiles(c.folder) for c in ch]
    try:
        writers = []
        for c, f in zip(ch, files):
            f.open("residual_variance", cov)
            f.open(f"marker_effects_variances_{name}", ["1"])
            if Mi.estimatePi:
                f.open(f"pi_{name}", [f"pi{i + 1}" for i in range(npi)] if npi > 1 else ["pi"])
            if outputEBV and output_heritability:
                c.genvar = GeneticVarianceSamples(f, cov, [trait])
            for key_, (_, header) in term_cols.items():
                f.open(key_, header)
            if write_marker_samples:
                f.open(f"marker_effects_{name}_{trait}", Mi.markerID)
            writers.append(f.marker_writer(f"marker_effects_{name}_{trait}", Mi.markerID))
        for it in range(1, chain_length + 1):
            if q:                                                        # 1. location parameters, chain by chain
                Rres = engine.mega_get_residual()
                for k, c in enumerate(ch):
                    r = Rres[k] + Xf0 @ c.sol
                    _gibbs(lhs, c.sol, Xf0.T @ r, c.rng, c.vare)
                    Rres[k] = r - Xf0 @ c.sol
                engine.mega_set_residual(Rres)
            vare_k, G_k = np.array([c.vare for c in ch]), np.array([c.Gval for c in ch])
            if bayesr:                                                   # 2. marker effects of every chain (DEVICE)
                st = engine.mega_sweep_r(iteration=it, seed=seed_int, vare=vare_k, var_effect=G_k, gamma=np.repeat(gamma[:, None], K, axis=1),
                                         pi=np.stack([c.pi for c in ch], axis=1))
            else:
                st = engine.mega_sweep(iteration=it, seed=seed_int, vare=vare_k, var_effect=G_k, pi=np.array([float(c.pi) for c in ch]))
            t_sweep += st["step_ms"]
            for k, c in enumerate(ch):
                if Mi.estimatePi:                                        # 3. pi
                    if bayesr:
                        c.pi = c.rng.dirichlet(st["class_counts"][:, k] + 1.0)
                    else:
                        c.pi = np.array(c.rng.beta(p - st["sum_delta"][k] + 1.0, st["sum_delta"][k] + 1.0))
                if Mi.G.estimate_variance:                               # 4. the marker-effect variance (variance_components.jl:151-189)
                    if bayesr:
                        c.Gval = float(ftype((st["ssq"][k] + Gdf * Mi.G.scale) / c.rng.chisquare(st["nnz"][k] + Gdf)))
                    else:
                        c.Gval = float(ftype((st["alpha_ss"][k] + Gdf * Mi.G.scale) / c.rng.chisquare(st["sum_delta"][k] + Gdf)))
                if R.estimate_variance:                                  # 5. the residual variance (variance_components.jl:60-66)
                    c.vare = float(ftype((st["resid_ss"][k] + Rdf * R.scale) / c.rng.chisquare(n + Rdf)))
            if it > burnin and (it - burnin) % output_samples_frequency == 0:      # 6. save
                ks = (it - burnin) / output_samples_frequency
                nsaved = int(ks)
                accumulate(ks)
                alpha = engine.mega_get_state()[0]
                for k, (c, f) in enumerate(zip(ch, files)):
                    c.run_sol.add(c.sol, ks)
                    c.run_vare.add([c.vare], ks)
                    c.run_varg.add([c.Gval], ks)
                    c.saved.append(np.concatenate([np.atleast_1d(c.pi), [c.Gval, c.vare]]))
                    if Mi.estimatePi:
                        c.run_pi.add(np.atleast_1d(c.pi), ks)
                        f.row(f"pi_{name}", np.atleast_1d(c.pi))
                    for key_, (cols, _) in term_cols.items():
                        f.row(key_, c.sol[cols])
                    f.row("residual_variance", [c.vare])
                    f.row(f"marker_effects_variances_{name}", [c.Gval])
                    a = alpha[k].astype(ftype)
                    si = np.flatnonzero(a).astype(np.int32)
                    writers[k].append(si, a[si])
                    if write_marker_samples:
                        f.effects_row(f"marker_effects_{name}_{trait}", a, fmt)
                    if outputEBV:                                        # getEBV, output.jl:281-306
                        ebv = np.asarray(engine.mega_mul_alpha(k, output_rows=not out_same), dtype=np.float64)
                        c.ebv_run.add(ebv, ks)
                        if c.genvar is not None:
                            c.genvar.add([ebv], np.array([c.vare]))
            if it % printout_frequency == 0 and it > burnin:
                print_posterior_means(it, np.array([c.run_vare.mean[0] for c in ch]))
    finally:
        for f in files:
            f.close()
    wall = time.time() - t0

    # ---- the tables of every chain, the pooled tables, the potential scale reduction factor (output.jl:108-212)
    def tables(run_sol, run_vare, run_varg, run_pi, post, ebv_run):
        out = {"location parameters": location_table(labels, off, run_sol.mean, run_sol.sd()), "residual variance": covariance_table(cov, run_vare)}
        out[f"marker effects {name}"] = marker_effects_table([(trait, Mi.markerID) + tuple(post)], sd_in_double=False)
        out[f"marker effects variance {name}"] = covariance_table(cov, run_varg)
        if Mi.estimatePi:
            out[f"pi_{name}"] = pi_table(run_pi, pi_labels(1, method))
        if outputEBV:
            out.update(ebv_tables([trait], out_ids, [ebv_run]))
        return out

    posts = [tuple(engine.mega_posterior(k)) for k in range(K)]
    results = []
    for k, c in enumerate(ch):
        out_k = tables(c.run_sol, c.run_vare, c.run_varg, c.run_pi, posts[k], c.ebv_run)
        if c.genvar is not None:
            out_k.update(c.genvar.tables())
        write_tables(out_k, c.folder)
        results.append(out_k)
    pooled_post = tuple(np.mean([pk[i] for pk in posts], axis=0) for i in range(3))
    out = tables(_pooled([c.run_sol for c in ch]), _pooled([c.run_vare for c in ch]), _pooled([c.run_varg for c in ch]),
                 _pooled([c.run_pi for c in ch]), pooled_post, _pooled([c.ebv_run for c in ch]) if outputEBV else None)
    if ch[0].genvar is not None:                                         # the samples of all chains as one (mean of the means; the SD from
        for key in ch[0].genvar.samples:                                 # the pooled second moment)
            s = np.array([row for c in ch for row in c.genvar.samples[key]])
            if len(s):
                out[key] = pd.DataFrame({"Covariance": ch[0].genvar.names[key], "Estimate": s.mean(axis=0),
                                         "SD": np.sqrt(np.abs((s * s).mean(axis=0) - s.mean(axis=0) ** 2))})
    write_tables(out, output_folder)

    scalar_names = ([f"pi_{name}:{lab}" for lab in pi_labels(1, method)] if Mi.estimatePi else []) + \
        [f"marker_effects_variance_{name}", "residual_variance"]
    if nsaved >= 2:
        r_markers = np.asarray(engine.mega_psrf(nsaved), dtype=np.float64)
        samples = np.array([c.saved for c in ch])                        # K x N x (npi + 2)
        r_scalar = psrf_rows(samples if Mi.estimatePi else samples[:, :, -2:])
    else:                                                                # the statistic needs two saved samples of every chain
        r_markers, r_scalar = np.full(p, np.nan), np.full(len(scalar_names), np.nan)
    psrf = pd.DataFrame({"Parameter": [f"marker_effect_{name}:{m}" for m in Mi.markerID] + scalar_names,
                         "PSRF": np.concatenate([r_markers, r_scalar])})
    fin = r_markers[np.isfinite(r_markers)]
    summary = pd.DataFrame({"Statistic": ["chains", "saved_samples", "markers_with_finite_PSRF", "max", "percentile_99", f"count_above_{PSRF_THRESHOLD}"],
                            "Value": [float(K), float(nsaved), float(fin.size), float(fin.max()) if fin.size else np.nan,
                                      float(np.percentile(fin, 99)) if fin.size else np.nan, float((fin > PSRF_THRESHOLD).sum())]})
    psrf.to_csv(os.path.join(output_folder, "PSRF.txt"), index=False)
    summary.to_csv(os.path.join(output_folder, "PSRF_summary.txt"), index=False)
    out["chains"], out["PSRF"], out["PSRF_summary"] = results, psrf, summary
    out["_timing"] = timing(wall, t_sweep, chain_length, bs, n, p, chains=K, first_chain=first)
    engine.mega_end()
    if own_engine:
        engine.close()
    return out
