"""Single-step analysis: runMCMC(model, df, single_step_analysis=True, pedigree=ped) (SSBRrun, single_step/SSBR.jl:8-54, and the
single-step branches of input_data_validation.jl:170-174,187-195,235-249).

Single-step Bayesian regression combines genotyped and non-genotyped relatives in one model: the genotypes of the non-genotyped
pedigree members are imputed from their genotyped relatives, M_n = A^nn \\ (-A^ng M_g), and the model gains two terms per trait --
J, a covariate that centres the imputed genotypes (make_JVecs, SSBR.jl:146-159), and ϵ, the imputation residual: a random effect over
the non-genotyped individuals with covariance (A^nn)^-1 (x) G, G the total genetic variance (SSBR.jl:23-53).

What runs where.  The host orders the pedigree as [non-genotyped; genotyped] (calc_Ai), forms A-inverse and factorises A^nn once
(scipy's SuperLU).  The imputation itself -- the one heavy step -- runs on the device as a sparse solve with many right-hand sides
(csrc/ssbr.hpp, engine.ss_*): of the genotypes only the g x chunk blocks of the genotyped individuals cross PCIe, the imputed
n_pheno x p matrix is written straight into the resident sweep matrix and the rows of the output IDs into the resident output matrix.
(The matrices themselves: a Float32 sweep matrix is allocated on the device; the output matrix and a Float64 sweep matrix are
allocated by uploading host zeros, for want of an allocating entry point -- host memory and one upload of their size.)  J comes from the
same solve (ss_solve_host).  The chain is then mcmc.run_chain on the device-resident matrix with the location parameters on the
device: J is a covariate of the location path, ϵ a structured random effect sampled colour by colour over the graph of A^nn.
"""
import numpy as np

SS_METHODS = ("ss_begin", "ss_set_rows", "ss_impute", "ss_solve_host", "ss_end")
MARKERS_PER_CHUNK = 8192                # upper bound of a chunk; the session's byte budget may lower it


class SingleStep:
    """What run_chain reads of a prepared single-step analysis: the output IDs and the J / ϵ parts of their EBVs."""

    def __init__(self, out_ids, J_out, eps_level_out):
        self.out_ids = list(out_ids)
        self.J_out = J_out                      # [n_out] J of every output ID (None: fitting_J_vector=False)
        self.eps_level_out = eps_level_out      # [n_out] level of ϵ of every output ID, -1 = genotyped

    def ebv_terms(self, labels_k):
        """(term, columns of the trait's solutions, coefficients) over the output IDs: EBV += coefficient * sol[column]
        (getEBV over mme.output_X[trait:J] and [trait:ϵ], output.jl:281-306; SSBR.jl:39-47)."""
        effects = [eff for _, eff, _ in labels_k]
        if self.J_out is not None and "J" in effects:
            yield "J", np.full(len(self.out_ids), effects.index("J"), dtype=np.int64), self.J_out
        if "ϵ" in effects:
            lev = self.eps_level_out
            yield "ϵ", effects.index("ϵ") + np.maximum(lev, 0), (lev >= 0).astype(np.float64)


def pedigree_blocks(ped, genotyped_ids):
    """calc_Ai (SSBR.jl:71-79): the pedigree ordered as [non-genotyped; genotyped] and the blocks A^nn (CSC), A^ng (CSR) of A-inverse.
    Returns (non, gen, Ai_nn, Ai_ng): non / gen are pedigree indices in pedigree order."""
    from .single_step import a_inverse
    gset = set(genotyped_ids)
    non = [i for i, v in enumerate(ped.ids) if v not in gset]
    gen = [i for i, v in enumerate(ped.ids) if v in gset]
    Ai = a_inverse(ped, np.array(non + gen, dtype=np.int64))
    nn = len(non)
    return non, gen, Ai[:nn, :nn].tocsc(), Ai[:nn, nn:].tocsr()


def factorize(Ai_nn):
    """The sparse LU of A^nn.  A^nn is symmetric positive definite: symmetric-mode options (a minimum-degree ordering of A' + A, no
    off-diagonal pivoting) keep the fill low.  The device solve does not rely on them."""
    import scipy.sparse.linalg as spla
    return spla.splu(Ai_nn.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))


def epsilon_structure(Ai_nn):
    """V^-1 of ϵ the way the reference keeps the Vinv of a random effect -- rounded through Float32 (random_effects.jl:184) -- as an
    exactly symmetric CSR matrix of doubles with ascending columns."""
    A = Ai_nn.tocsr().astype(np.float32).astype(np.float64)
    A = ((A + A.T) * 0.5).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def _strip_terms(model):
    """A model that has been through a single-step run carries its J / ϵ terms: they are rebuilt for this run's data."""
    for tl in model.modelTerms:
        tl[:] = [mt for mt in tl if mt.name not in ("J", "ϵ")]
    model.rndTrmVec = [re_ for re_ in model.rndTrmVec if re_.name != "ϵ"]
    model.covVec = [v for v in model.covVec if v != "J"]
    model.outputSamplesVec = [(tr, trm) for tr, trm in model.outputSamplesVec if trm not in ("J", "ϵ")]


def validate(model, df, ped, *, fitting_J_vector, location_parameters, double_precision, outputEBV, engine):
    """Everything that can be refused before a folder exists or an engine is touched.  Returns the plan prepare() carries out."""
    from .api import _is_false
    from .single_step import Pedigree
    if not isinstance(ped, Pedigree):
        raise TypeError("runMCMC(...; single_step_analysis=true, pedigree=ped): pedigree must be a single_step.Pedigree (get_pedigree)")
    if not isinstance(fitting_J_vector, (bool, np.bool_)):
        raise ValueError("fitting_J_vector must be true or false.")
    Mi = model.M[0]
    if getattr(Mi, "storage_mode", "dense") == "stream":
        raise ValueError("storage=:stream MVP does not support single_step_analysis.")          # input_data_validation.jl:94-95
    if getattr(Mi, "storage_mode", "dense") == "device":
        raise NotImplementedError("single_step_analysis with device_genotypes input: the imputation reads the genotyped individuals' matrix "
                                  "on the host (get_genotypes)")
    if location_parameters == "host":
        raise NotImplementedError('single_step_analysis runs the location parameters on the device (J and ϵ are terms of that path): '
                                  'location_parameters="host" is not available')
    if model.ped is not False or any(re_.randomType == "A" for re_ in model.rndTrmVec):
        raise NotImplementedError("single_step_analysis with a pedigree random effect of set_random(model, trm, ped, G) in the same model: the "
                                  "device path holds one structured effect per model, and ϵ is it")
    if any(tt != "continuous" for tt in getattr(model, "traits_type", [])):
        raise NotImplementedError("single_step_analysis with categorical_trait / censored_trait stays on the reference")
    if Mi.alpha is not False:
        raise NotImplementedError("single_step_analysis with marker starting values (get_genotypes(starting_value=...)) stays on the reference")
    if engine is not None:
        if hasattr(engine, "comm_info") and engine.comm_info()[1] > 1:
            raise NotImplementedError("single_step_analysis is not driven from marker or row shards")
        missing = [m for m in SS_METHODS if not hasattr(engine, m)]
        if missing:
            raise NotImplementedError("single_step_analysis needs an engine with the imputation session (" + ", ".join(missing)
                                      + " missing); the package has no CPU fallback")
    if not double_precision and getattr(Mi.genotypes, "dtype", None) == np.float64:
        raise NotImplementedError("Float64 genotypes (get_genotypes(double_precision=true)) run with runMCMC(double_precision=true); "
                                  "the mixed Float64 / Float32 chain stays on the reference")
    if not set(Mi.obsID) <= set(ped.ids):                                                       # input_data_validation.jl:213-218
        raise ValueError("Not all genotyped individuals are found in pedigree!")
    if _is_false(Mi.genetic_variance.val):                                                       # SSBR.jl:18-20
        raise ValueError("Please input the genetic variance using add_genotypes()")
    idcol = df.columns[0]
    ph = df.copy()
    ph[idcol] = ph[idcol].astype(str).str.strip()
    pheno_ids = list(ph[idcol])
    inped = ph[idcol].isin(set(ped.ids)).to_numpy()
    notice = None
    if not inped.all():                                                                          # :235-243
        ph = ph.loc[inped].reset_index(drop=True)
        notice = (f"In this incomplete genomic data (single-step) or PBLUP analysis, {int((~inped).sum())} phenotyped individuals are not "
                  "included in the pedigree. These are removed from the analysis.")
    if set(pheno_ids) <= set(Mi.obsID):                                                          # :244-248
        raise ValueError("All phenotyped individuals arer genotyped. Do not run single step analysis.")
    for tr in model.lhsVec:
        if tr not in ph.columns:
            raise ValueError(f"Phenotypes for {tr} are not found in the data.")
    obs = np.stack([np.isfinite(ph[tr].to_numpy(dtype=np.float64)) for tr in model.lhsVec], axis=1)
    if (obs.any(axis=1) & ~obs.all(axis=1)).any():
        raise NotImplementedError("single_step_analysis with records that miss some traits (missing_phenotypes) stays on the reference: the "
                                  "device-resident matrix holds complete records")
    ph = ph.loc[obs.all(axis=1)].reset_index(drop=True)                                           # (records without phenotypes: :396-404)
    if len(ph) == 0:
        raise ValueError("no individual of the pedigree has phenotypes")
    out_ids = None
    if outputEBV:                                                                                # check_outputID, :150-195
        out_ids = list(ped.ids) if getattr(model, "output_ID", False) is False else list(model.output_ID)
        if not set(out_ids) <= set(ped.ids):
            print("Testing individuals are not a subset of individuals in pedigree (incomplete genomic data (single-step) or PBLUP). "
                  "Only output EBV for tesing individuals in the pedigree.")
            out_ids = [i for i in out_ids if i in ped.index]
        if not out_ids:
            raise ValueError("none of the individuals of outputEBV(model, IDs) is in the pedigree")
    return dict(ph=ph, idcol=idcol, out_ids=out_ids, notice=notice, fitting_J=bool(fitting_J_vector))


def prepare(model, plan, ped, engine, *, double_precision, memory_guard="error", memory_guard_ratio=0.80):
    """impute_genotypes, make_JVecs and the model terms of SSBRrun (SSBR.jl:8-54).  `engine` ends up holding the imputed matrices.
    Returns (phenotype frame with the J and ϵ columns, the Genotypes object over the resident matrix, SingleStep)."""
    from .api import Genotypes, ModelTerm, RandomEffect, Variance
    Mi = model.M[0]
    ph, idcol, out_ids = plan["ph"], plan["idcol"], plan["out_ids"]
    if plan["notice"]:
        print(plan["notice"])
    dtype = np.float64 if double_precision else np.float32
    print("calculating A inverse")
    non, gen, Ai_nn, Ai_ng = pedigree_blocks(ped, Mi.obsID)
    nn, g = len(non), len(gen)
    where = {int(i): k for k, i in enumerate(non + gen)}                                        # pedigree index -> row of [M_n; M_g]
    rec_ids = list(ph[idcol])
    prow = np.array([where[ped.index[v]] for v in rec_ids], dtype=np.int32)
    prow_out = None if out_ids is None else np.array([where[ped.index[v]] for v in out_ids], dtype=np.int32)
    gidx = {v: i for i, v in enumerate(Mi.obsID)}
    mg_rows = np.array([gidx[ped.ids[i]] for i in gen], dtype=np.int64)                          # Z * genotypes (SSBR.jl:87-88)
    n, p = len(rec_ids), Mi.nMarkers
    lu = factorize(Ai_nn)
    chunk = min(MARKERS_PER_CHUNK, -(-p // 64) * 64)
    if memory_guard != "off" and hasattr(engine, "device_info") and hasattr(engine, "ss_estimate_bytes"):
        el = 8 if double_precision else 4
        need = (engine.ss_estimate_bytes(nn, g, lu.L.nnz, lu.U.nnz, Ai_ng.nnz, chunk) + el * p * (-(-n // 256) * 256)
                + (0 if out_ids is None else el * p * (-(-len(out_ids) // 256) * 256)))
        free = engine.device_info()["hbm_free"]
        if need > memory_guard_ratio * free:
            msg = f"single-step imputation needs {need / 1e9:.2f} GB of HBM, more than {memory_guard_ratio:.2f} x free ({free / 1e9:.2f} GB)"
            if memory_guard == "error":
                raise MemoryError(msg)
            print("WARNING: " + msg)
    print(f"imputing missing genotypes for {Mi.name}")
    if not double_precision and hasattr(engine, "alloc_dense"):
        engine.alloc_dense(n, p)
    else:
        engine.load_dense(np.zeros((n, p), dtype=dtype, order="F"))
    if out_ids is not None:
        engine.load_output_dense(np.zeros((len(out_ids), p), dtype=dtype, order="F"))
    ldc = engine.ss_begin(lu, Ai_ng, markers_per_chunk=chunk)
    try:
        engine.ss_set_rows("sweep", prow)
        if out_ids is not None:
            engine.ss_set_rows("output", prow_out)
        G = Mi.genotypes
        for j0 in range(0, p, ldc):                                                              # SSBR.jl:122-131
            engine.ss_impute(j0, np.asfortranarray(G[mg_rows, j0:min(p, j0 + ldc)], dtype=dtype))
        J_rec = J_out = None
        if plan["fitting_J"]:                                                                    # make_JVecs, SSBR.jl:146-159
            rows = prow if prow_out is None else np.concatenate([prow, prow_out])
            J = engine.ss_solve_host(-np.ones((g, 1)), rows)[:, 0]
            J_rec, J_out = J[:n], (None if prow_out is None else J[n:])
    finally:
        engine.ss_end()
    print(f"completed imputing genotypes for {Mi.name}")
    geno = Genotypes(rec_ids, Mi.markerID, n, p, Mi.alleleFreq, Mi.sum2pq, Mi.centered, np.zeros((n, 0), dtype=dtype))    # SSBR.jl:137-140
    geno.storage_mode, geno.device_backend = "device", engine
    for k in ("G", "genetic_variance", "method", "estimatePi", "pi", "multi_trait_sampler", "name", "ntraits", "trait_names", "annotations", "alpha"):
        setattr(geno, k, getattr(Mi, k))
    # the model terms (SSBR.jl:23-53): ϵ, then J; their data columns
    _strip_terms(model)
    ph = ph.copy()
    non_ids = [ped.ids[i] for i in non]
    nonset = set(non_ids)
    ph["ϵ"] = [v if v in nonset else "missing" for v in rec_ids]                                 # :28-31
    traits = list(range(model.nModels))
    for k, tr in enumerate(model.lhsVec):
        model.modelTerms[k].append(ModelTerm(tr, "ϵ"))
    if plan["fitting_J"]:
        ph["J"] = J_rec
        for k, tr in enumerate(model.lhsVec):
            mt = ModelTerm(tr, "J")
            mt.kind = "covariate"
            model.modelTerms[k].append(mt)
        model.covVec.append("J")
    t = model.nModels
    Gm = np.atleast_2d(np.asarray(Mi.genetic_variance.val, dtype=np.float64))                  # total_single_step_genetic_variance (:56-62)
    if Gm.shape != (t, t):
        raise ValueError(f"The genomic covariance matrix is not a {t} by {t} matrix.")
    dfk = np.float32(4.0) + t                                                                    # set_random's defaults (random_effects.jl:182-185)
    Gi = np.linalg.inv(Gm.astype(np.float32))
    Gi = (Gi + Gi.T) / 2
    var = Variance(Gi, dfk, Gm * (float(dfk) - t - 1), True, False, False)
    model.rndTrmVec.append(RandomEffect("ϵ", [f"{tr}:ϵ" for tr in model.lhsVec], traits, var, "V", epsilon_structure(Ai_nn), non_ids))      # :37
    for trm in (("J",) if plan["fitting_J"] else ()) + ("ϵ",):                                   # outputMCMCsamples(mme, "J") / ("ϵ") (:48-53)
        for tr in model.lhsVec:
            if (tr, trm) not in model.outputSamplesVec:
                model.outputSamplesVec.append((tr, trm))
    lev = {v: i for i, v in enumerate(non_ids)}
    ss = None if out_ids is None else SingleStep(out_ids, J_out, np.array([lev.get(v, -1) for v in out_ids], dtype=np.int64))
    if ss is None:
        ss = SingleStep([], None, np.zeros(0, dtype=np.int64))
    return ph, geno, ss


def run_single_step(model, df, ped, plan, *, double_precision, device, engine, memory_guard, memory_guard_ratio, chain_kwargs):
    """SSBRrun, then the chain (JWAS.jl:404-413 -> MCMC_BayesianAlphabet.jl) on the device-resident imputed matrix."""
    from .mcmc import run_chain
    own = engine is None
    if own:
        from .engine import HipEngine
        engine = HipEngine(device, precision=64 if double_precision else 32)
    Mi = model.M[0]
    try:
        ph, geno, ss = prepare(model, plan, ped, engine, double_precision=double_precision, memory_guard=memory_guard,
                               memory_guard_ratio=memory_guard_ratio)
        model.M = [geno]
        return run_chain(model, ph, double_precision=double_precision, device=device, engine=None, memory_guard=memory_guard,
                         memory_guard_ratio=memory_guard_ratio, location_parameters="device", single_step=ss, **chain_kwargs)
    finally:
        model.M = [Mi]
        if own:
            engine.close()
