"""Several genotype categories in one model: build_model("y = intercept + geno1 + geno2") -- the host side of
MCMC_BayesianAlphabet.jl:184-421 for C >= 2 entries of mme.M, a driver of its own (as rrm.py is for RRM) so that mcmc.run_chain, whose
chains are pinned bit for bit, stays as it is.

Every category is a sweep engine of its own (its genotypes, Grams, effects, running means); the ONE residual of the model moves between
them on the device (engine.residual_handover, jwas_hip_residual_handover).  Exactly one engine owns the current residual at any time,
_Residual.move is the only place it changes hands, and nothing reads a residual from an engine that is not the owner.

Per iteration, the reference's order:
  1. location parameters on the host, from the owner's residual                                           (:196-220)
  2. for every category i, in the order of mme.M                                                          (:224-337)
       the residual moves to category i; engine_i.sweep(..., marker_offset = sum_{k<i} p_k)               (DEVICE)
       pi_i, the marker-effect variance of category i, its prior scale if estimate_scale                  (host, the one numpy generator)
  3. residual variance from the last category's resid_ss                                                  (:363-370)
  4. every output_samples_frequency after burn-in: running means (each engine's accumulate), EBV = sum_i X_out,i alpha_i (output.jl:300-304)
marker_offset keeps the categories' counter ranges disjoint: with it, two categories on the `block` form are one chain on [X1 X2] with a
block start at p1 in every bit; without it category 2 would reuse category 1's draws.

Block size per category: block_size if given, else the non-adaptive default run_chain computes for that p and storage.  The adaptive
512 / 1024 switching, grouped launches, ping-pong pairs and the section solve stay off here (a performance follow-up).  Everything outside
the scope below raises NotImplementedError in validate(), before any device work."""
import time

import numpy as np

from .chain_output import (GeneticVarianceSamples, Running, SampleFiles, covariance_table, ebv_tables, host_blas_limit, location_table,
                           marker_effects_table, pi_labels, pi_table, print_posterior_means, resolve_output_ids, sparse_effects,
                           term_sample_columns, write_id_files, write_tables)
from .mcmc import _design, _gibbs, genetic2marker, host_location_step
from .session_driver import not_false

MAX_TRAITS = 4


def validate(model, df, *, fast_blocks=False, independent_blocks=False, location_parameters="auto", causal_structure=False,
             RRM=False, starting_value=False, double_precision=False, engines=None):
    """What the device path does not run with several genotype categories raises here, each message naming the feature.  Returns
    the engines as a list (None: one HipEngine per category is created by the run)."""
    M = model.M
    t = model.nModels
    names = [Mi.name for Mi in M]
    what = f"with several genotype categories ({', '.join(names)})"
    if fast_blocks is not False or independent_blocks:
        raise NotImplementedError(f"fast_blocks / independent_blocks {what} stay on the reference (which reads only the first category there)")
    if location_parameters == "device":
        raise NotImplementedError(f'location_parameters="device" {what} is not supported: the location parameters are sampled on the host')
    if getattr(model, "rndTrmVec", []):
        raise NotImplementedError(f"set_random effects {what} stay on the reference")
    if any(tt != "continuous" for tt in getattr(model, "traits_type", [])):
        raise NotImplementedError(f"categorical or censored traits {what} stay on the reference")
    if not_false(causal_structure):
        raise NotImplementedError(f"causal_structure {what} stays on the reference")
    if not_false(RRM):
        raise NotImplementedError(f"RRM {what} stays on the reference")
    if any(getattr(Mi, "annotations", False) is not False for Mi in M):
        raise NotImplementedError(f"marker annotations {what} stay on the reference")
    if any(Mi.alpha is not False for Mi in M) or not (isinstance(starting_value, bool) and not starting_value):
        raise NotImplementedError(f"marker starting values (and starting values of location parameters) {what} stay on the reference")
    if any(Mi.G.constraint for Mi in M) or model.R.constraint:
        raise NotImplementedError(f"constraint=true {what} stays on the reference")
    if any(getattr(Mi, "storage_mode", "dense") == "device" for Mi in M):
        raise NotImplementedError(f"device_genotypes engines {what} are not supported: use get_genotypes")
    if t > MAX_TRAITS:
        raise NotImplementedError(f"more than {MAX_TRAITS} traits {what} are not supported")
    if t > 1:
        bad = [Mi.method for Mi in M if Mi.method not in ("BayesC", "RR-BLUP")]
        if bad:
            raise NotImplementedError(f"multi-trait {'/'.join(sorted(set(bad)))} {what}: multi-trait BayesA/B/L stay on the reference "
                                      "(BayesC under samplers I and II and RR-BLUP run)")
        Y = np.stack([np.asarray(df[tr], dtype=np.float64) for tr in model.lhsVec if tr in df.columns])
        if Y.shape[0] == t:
            obs = np.isfinite(Y)
            if (obs.any(axis=0) & ~obs.all(axis=0)).any():
                raise NotImplementedError(f"missing traits (records that miss the phenotype of some traits) {what} stay on the reference")
    for Mi in M:
        f64 = getattr(Mi.genotypes, "dtype", None) == np.float64
        stream = getattr(Mi, "storage_mode", "dense") == "stream"
        if double_precision and (stream or not f64):
            raise NotImplementedError(f"double_precision=true {what} needs every category dense and Float64 "
                                      f"(get_genotypes(double_precision=true)); {Mi.name} is not")
        if not double_precision and f64:
            raise NotImplementedError("Float64 genotypes (get_genotypes(double_precision=true)) run with runMCMC(double_precision=true); "
                                      "the mixed Float64 / Float32 chain stays on the reference")
    if engines is not None:
        if not isinstance(engines, (list, tuple)) or len(engines) != len(M):
            raise ValueError(f"_engine must be a list with one engine per genotype category ({len(M)})")
        if len({id(e) for e in engines}) != len(engines):
            raise ValueError("_engine: every genotype category needs an engine of its own")
        for e in engines:
            if not hasattr(e, "residual_handover"):
                raise NotImplementedError("several genotype categories need engines with residual_handover; the package has no CPU fallback")
            if hasattr(e, "comm_info") and e.comm_info()[1] > 1:
                raise NotImplementedError(f"marker shards {what} are not supported")
        engines = list(engines)
    for Mi in M[1:]:                                                      # input_data_validation.jl:209-212
        if list(Mi.obsID) != list(M[0].obsID):
            raise ValueError("genotypic information is not provided for same individuals")
    return engines


def default_block_size(method, t, pi, p, estimate_pi, double_precision):
    """The non-adaptive block size run_chain picks when none is given (method and pi after the method rewrites): dense priors keep the
    block Gram in LDS (128 markers; 512 for a prior that includes every marker; 256 for multi-trait sampler-I chains), sparse ones run
    512-marker blocks; a Float64 context runs 512."""
    if double_precision:
        bs = 512
    else:
        if t > 1:
            dense = float(np.asarray(pi, dtype=np.float64)[(1 << t) - 1]) > 0.5
        elif method == "BayesR":
            dense = float(np.asarray(pi, dtype=np.float64)[0]) < 0.5
        else:
            dense = float(np.mean(pi)) < 0.5
        all_in = t == 1 and method in ("BayesC", "BayesB") and np.ndim(pi) == 0 and float(pi) == 0.0 and not estimate_pi
        bs = (512 if all_in else (256 if t > 1 else 128)) if dense else 512
    while bs > 64 and p <= bs:
        bs //= 2
    return bs


class _Category:
    """The chain's state of one genotype category: what run_chain keeps in locals for its single Mi."""

    def __init__(self, Mi, t, ftype, offset):
        self.Mi, self.name, self.t, self.ftype, self.offset = Mi, Mi.name, t, ftype, int(offset)
        self.p = Mi.nMarkers
        self.stream = getattr(Mi, "storage_mode", "dense") == "stream"
        self.engine = None
        self.lasso = False

    def set_priors(self, varg, rng, printout):
        """Pi defaults, the method rewrites and genetic2marker of this category (tools4genotypes.jl:353-418; as run_chain)."""
        Mi, t, ftype = self.Mi, self.t, self.ftype
        method = Mi.method
        if Mi.G.val is False and Mi.genetic_variance.val is False:       # input_data_validation.jl:316-327: varg = h2 var(y) / C
            Mi.genetic_variance.val = varg[0, 0] if t == 1 else varg
        pi = Mi.pi
        if isinstance(pi, dict):
            if t == 1:
                raise ValueError("a Dict Pi is for multi-trait analyses only")
            tab = np.zeros(1 << t)
            for key, val in pi.items():
                key = tuple(float(v) for v in key)
                if len(key) != t or any(v not in (0.0, 1.0) for v in key):
                    raise ValueError(f"Pi keys must be 0/1 vectors of length {t} (got {key})")
                tab[sum(1 << k for k in range(t) if key[k] == 1.0)] = float(val)
            if abs(tab.sum() - 1.0) > 1e-6:
                raise ValueError("Summation of probabilities of Pi is not equal to one.")
            pi = tab
        if t > 1 and np.isscalar(pi) and pi == 0.0:                      # tools4genotypes.jl:357-373
            pi = np.zeros(1 << t)
            pi[(1 << t) - 1] = 1.0
        if method == "BayesR" and np.isscalar(pi) and pi == 0.0:         # :375-377
            pi = np.array([0.95, 0.03, 0.015, 0.005])
        if method == "BayesA":                                           # input_data_validation.jl:33-36
            method, Mi.estimatePi, pi = "BayesB", False, 0.0
        self.lasso = method == "BayesL"
        if self.lasso:                                                   # BayesL!: the BayesB update with pi = 0, var_j = G gamma_j
            if not (np.isscalar(pi) and (pi is False or pi == 0.0)):
                print("BayesL runs with π = false.")
            elif Mi.estimatePi:
                print("BayesL runs with estimatePi = false.")
            method, pi, Mi.estimatePi = "BayesB", 0.0, False
        if method == "RR-BLUP":                                          # the BayesC update with pi = 0
            if not (np.isscalar(pi) and (pi is False or pi == 0.0)):
                print("RR-BLUP runs with π = false.")
            elif Mi.estimatePi:
                print("RR-BLUP runs with estimatePi = false.")
            method, Mi.estimatePi = "BayesC", False
            pi = 0.0 if t == 1 else np.eye(1, 1 << t, (1 << t) - 1).ravel()
        if t > 1 and np.shape(pi) != (1 << t,):
            raise ValueError(f"Pi of {self.name} must hold one value per joint state ({1 << t}).")
        if Mi.G.val is False:
            Mi.G.val = genetic2marker(Mi, pi, method, t)
            if (t == 1 and not Mi.G.val > 0) or (t > 1 and (not np.all(np.isfinite(Mi.G.val)) or np.any(np.linalg.eigvalsh(Mi.G.val) <= 0))):
                raise ValueError("Marker effects variance is negative!" if t == 1 else
                                 "Marker effects covariance matrix is not postive definite! Please modify the argument: Pi.")
            if printout:
                print(f"The prior for marker effects variance of {self.name} is calculated from the genetic variance and π.")
        self.Gdf = Gdf = float(Mi.G.df)
        Mi.G.scale = (np.float64(Mi.G.val) * (Gdf - 2) / Gdf) if t == 1 else np.asarray(Mi.G.val, dtype=np.float64) * (Gdf - t - 1)
        sampler = getattr(Mi, "multi_trait_sampler", "I")
        if t > 1 and sampler == "auto":
            sampler = "I" if (len(Mi.pi) if isinstance(Mi.pi, dict) else (1 << t)) == (1 << t) else "II"
        self.init_method = ("MTBayesC_II" if sampler == "II" else "MTBayesC") if t > 1 else method
        self.method = method
        self.Gval = ftype(Mi.G.val) if t == 1 else np.asarray(Mi.G.val, dtype=ftype)
        self.Gvec = None
        if self.lasso:                                                   # MCMC_BayesianAlphabet.jl:70-81
            self.Gval = ftype(self.Gval / 8)
            Mi.G.scale = Mi.G.scale / 8
            self.gamma_l = rng.gamma(1.0, 8.0, size=self.p)
            self.Gvec = (np.float64(self.Gval) * self.gamma_l).astype(ftype)
        elif method == "BayesB":
            self.Gvec = np.full(self.p, self.Gval, dtype=ftype)
        self.pervar = method == "BayesB" and not self.lasso
        if t == 1 and method in ("BayesC", "BayesB") and np.ndim(pi) == 0:
            pi = float(pi)
        self.pi = pi

    def sweep_kw(self):
        if self.t > 1:
            with np.errstate(divide="ignore"):
                return dict(var_effect=self.Gval, log_prior_states=np.log(np.asarray(self.pi, dtype=np.float64)))
        if self.method == "BayesR":
            return dict(var_effect=self.Gval, pi_classes=np.asarray(self.pi, dtype=np.float64))
        if self.method == "BayesB":
            return dict(var_effect=self.Gval, var_effect_vec=self.Gvec, pi=self.pi)
        return dict(var_effect=self.Gval, pi=self.pi)

    def draw_hyper(self, st, rng):
        """pi, the marker-effect variance and its prior scale from this category's sweep: steps 3, 4, 4b of run_chain."""
        Mi, t, ftype, p, Gdf = self.Mi, self.t, self.ftype, self.p, self.Gdf
        if Mi.estimatePi:                                                # Pi.jl:7-42
            if t > 1:
                self.pi = rng.dirichlet(st["state_counts"] + 1.0)
            elif self.method == "BayesR":
                self.pi = rng.dirichlet(st["class_counts"] + 1.0)
            else:
                self.pi = float(rng.beta(p - st["sum_delta"][0] + 1.0, st["sum_delta"][0] + 1.0))
        if Mi.G.estimate_variance:                                       # variance_components.jl:151-189
            if t > 1:
                from scipy.stats import invwishart
                S = np.asarray(Mi.G.scale, dtype=np.float64) + st["beta_ss"]
                self.Gval = np.asarray(invwishart.rvs(df=Gdf + p, scale=(S + S.T) / 2, random_state=rng), dtype=ftype).reshape(t, t)
            elif self.method == "BayesR":
                self.Gval = ftype((st["bayesr_ssq"] + Gdf * Mi.G.scale) / rng.chisquare(st["bayesr_nnz"] + Gdf))
            elif self.lasso:
                a64 = self.engine.get_state(0)[0].astype(np.float64)
                self.Gval = ftype((np.dot(a64 / self.gamma_l, a64) + Gdf * Mi.G.scale) / rng.chisquare(p + Gdf))
                Q = a64 * a64 / np.float64(self.Gval)
                cand = 1.0 / rng.gamma(0.5, 4.0, size=p)
                with np.errstate(over="ignore"):
                    accept = rng.random(p) < np.exp(Q / 4.0 * (2.0 / self.gamma_l - cand))
                self.gamma_l[accept] = 2.0 / cand[accept]
                self.Gvec = (np.float64(self.Gval) * self.gamma_l).astype(ftype)
            elif self.method == "BayesB":
                beta = self.engine.get_state(0)[1].astype(np.float64)
                self.Gvec = ((beta * beta + Gdf * Mi.G.scale) / rng.chisquare(1.0 + Gdf, size=p)).astype(ftype)
            else:
                self.Gval = ftype((ftype(st["alpha_ss"][0, 0]) + Gdf * Mi.G.scale) / rng.chisquare(st["sum_delta"][0] + Gdf))
        if Mi.G.estimate_scale and t == 1:                               # MCMC_BayesianAlphabet.jl:328-336
            gv = self.Gvec.astype(np.float64) if self.pervar else np.atleast_1d(np.float64(self.Gval))
            Mi.G.scale = float(rng.gamma(gv.size * Gdf / 2 + 1, 1.0 / (np.sum(Gdf / (2 * gv)) + 1)))


class _Residual:
    """The one residual of the model and the engine that owns it."""

    def __init__(self, engines):
        self.engines, self.owner = engines, 0

    def move(self, i):
        """The residual moves to engine i (a no-op when it is there already): the only place it changes hands."""
        if i != self.owner:
            self.engines[i].residual_handover(self.engines[self.owner])
            self.owner = i
        return self.engines[i]

    @property
    def engine(self):
        return self.engines[self.owner]


def memory_need(cats, n, t, double_precision, n_out_rows):
    """HBM the categories need together: every context's estimate plus the output matrices."""
    from .engine import HipEngine
    need = 0
    for c in cats:
        need += HipEngine.estimate_bytes(n, c.p, t, c.block_size, "stream" if c.stream else "dense") * (2 if double_precision else 1)
        if n_out_rows:
            need += (8 if double_precision else 4) * ((n_out_rows + 255) // 256 * 256) * c.p
    return need


def run_multigeno(model, df, *, chain_length, burnin, output_samples_frequency, seed, heterogeneous_residuals=False,
                  double_precision=False, outputEBV=True, output_heritability=True, output_folder, printout_frequency,
                  memory_guard="error", memory_guard_ratio=0.80, device=0, block_size=None, gram_mode="mfma", engines=None,
                  printout_model_info=True, output_samples_for_all_parameters=False):
    M = model.M
    C, t = len(M), model.nModels
    ftype = np.float64 if double_precision else np.float32
    seed_int = 0 if seed is False else int(seed)
    rng = np.random.default_rng(seed_int)                                # every host draw, in the order of the module docstring

    # ---- align phenotypes and genotypes once, for every category (input_data_validation.jl:198-294)
    idcol = df.columns[0]
    ph = df.copy()
    ph[idcol] = ph[idcol].astype(str)
    for tr in model.lhsVec:
        if tr not in ph.columns:
            raise ValueError(f"Phenotypes for {tr} are not found in the data.")
    obsY = np.stack([np.isfinite(ph[tr].to_numpy(dtype=np.float64)) for tr in model.lhsVec])
    usable = obsY.all(axis=0)                                            # (complete records only: validate refused partial ones)
    obsID = list(M[0].obsID)
    any_stream = any(getattr(Mi, "storage_mode", "dense") == "stream" for Mi in M)
    if any_stream:
        if not usable.all() or list(ph[idcol]) != obsID:
            raise ValueError("storage=:stream MVP requires exact genotype/phenotype ID match and order. "
                             "Please reorder phenotypes to match genotype IDs.")
        print("storage=:stream is enabled; genotype alignment is skipped and original ID order is used.")
        rows = np.arange(len(obsID), dtype=np.int64)
    else:
        geno_index = {g: i for i, g in enumerate(obsID)}
        genotyped = ph[idcol].isin(geno_index).to_numpy()
        if not genotyped.all():
            print(f"In this complete genomic data (non-single-step) analyis, {int((~genotyped).sum())} phenotyped individuals are not "
                  "genotyped. These are removed from the analysis.")
        ph = ph.loc[usable & genotyped].reset_index(drop=True)
        if len(ph) == 0:
            raise ValueError("no individual has both phenotypes and genotypes")
        rows = np.array([geno_index[i] for i in ph[idcol]], dtype=np.int64)
    n = len(rows)
    identity = n == len(obsID) and np.array_equal(rows, np.arange(n))
    out_ids, out_rows, out_same = None, None, True
    if outputEBV:
        out_ids, out_same = resolve_output_ids(model, obsID, ph[idcol])
        if not out_same:
            if any_stream:
                raise NotImplementedError("storage=:stream reports EBVs for the genotyped individuals in file order "
                                          "(outputEBV(model, IDs) lists stay on the reference)")
            gi = {g: i for i, g in enumerate(obsID)}
            out_rows = np.array([gi[i] for i in out_ids], dtype=np.int64)
    for Mi in M:
        if getattr(Mi, "storage_mode", "dense") == "dense":
            Mi.output_rows = out_rows if (outputEBV and not out_same) else rows
    write_id_files(output_folder, ph[idcol], obsID)
    Y = np.stack([ph[tr].to_numpy(dtype=ftype) for tr in model.lhsVec])       # t x n
    phenovar = np.array([np.var(Y[k].astype(np.float64), ddof=1) for k in range(t)])
    invw = None
    if heterogeneous_residuals:                                          # build_MME.jl:305-310
        if "weights" not in ph.columns:
            raise ValueError("heterogeneous_residuals=true requires a column named weights in the phenotype data.")
        invw = (1.0 / ph["weights"].to_numpy(dtype=np.float64)).astype(ftype)
        if not np.all(np.isfinite(invw) & (invw > 0)):
            raise ValueError("weights must be positive and finite.")
    w64 = np.ones(n) if invw is None else invw.astype(np.float64)

    # ---- default priors (input_data_validation.jl:296-350): genetic_random_count = length(mme.M)
    varg = np.diag(phenovar) * 0.5 / C
    vare0 = np.diag(phenovar) * 0.5
    R = model.R
    if R.val is False:
        R.val = ftype(vare0[0, 0]) if t == 1 else vare0.astype(ftype)
        R.scale = float(R.val) * (float(R.df) - 2) / float(R.df) if t == 1 else np.asarray(R.val, dtype=np.float64) * (float(R.df) - t - 1)
    Rdf = float(R.df)
    cats, offset = [], 0
    for Mi in M:
        c = _Category(Mi, t, ftype, offset)
        c.set_priors(varg, rng, printout_model_info)
        c.block_size = int(block_size) if block_size is not None else default_block_size(c.method, t, c.pi, c.p, bool(Mi.estimatePi), double_precision)
        if c.block_size * t > 2048 and double_precision:
            raise NotImplementedError(f"double_precision=true needs block size x traits <= 2048 on the device (got {c.block_size} x {t})")
        cats.append(c)
        offset += c.p

    # ---- engines: one per category; the memory guard looks at all of them together
    own = engines is None
    if own:
        from .engine import HipEngine
        engines = [HipEngine(device, precision=64 if double_precision else 32)]
    try:
        if memory_guard != "off" and hasattr(engines[0], "device_info"):
            need = memory_need(cats, n, t, double_precision, len(out_rows) if out_rows is not None else 0)
            free = engines[0].device_info()["hbm_free"]
            if need > memory_guard_ratio * free:                         # JWAS.jl:422-459 analogue for HBM
                msg = (f"marker path needs {need / 1e9:.2f} GB of HBM, more than {memory_guard_ratio:.2f} x free "
                       f"({free / 1e9:.2f} GB)")
                if memory_guard == "error":
                    raise MemoryError(msg)
                print("WARNING: " + msg)
        if own:
            engines += [HipEngine(device, precision=64 if double_precision else 32) for _ in range(C - 1)]
        X_out_host = [None] * C
        for c, eng in zip(cats, engines):
            c.engine = eng
            if c.stream:
                eng.load_jgb2(c.Mi.stream_backend["prefix"])
            else:
                G_ = c.Mi.genotypes
                eng.load_dense(np.asfortranarray(G_ if identity else G_[rows, :], dtype=ftype))
            if outputEBV and not out_same:                               # Mi.output_genotypes (tools4genotypes.jl:290-296)
                Xo = c.Mi.genotypes[out_rows, :]
                if hasattr(eng, "load_output_dense") and hasattr(eng, "mul_alpha_output"):
                    eng.load_output_dense(np.asfortranarray(Xo, dtype=ftype))
                else:
                    X_out_host[cats.index(c)] = np.asarray(Xo, dtype=np.float64)
            if invw is not None or getattr(eng, "_weighted", False):
                eng.set_weights(invw)                                    # the same weights on every context
            eng.setup_blocks(c.block_size, gram_mode)
            eng.init_state(c.init_method, t)
            for k in range(t):
                eng.set_state(k, alpha=np.zeros(c.p, dtype=ftype), beta=np.zeros(c.p, dtype=ftype),
                              delta=np.ones(c.p, dtype=np.int32 if c.method == "BayesR" else ftype))
        resid = _Residual(engines)
        for k in range(t):                                               # ycorr = y (sol = 0, alpha = 0): category 1 owns it first
            resid.engine.set_residual(Y[k], k)

        # ---- location parameters on the host
        Xf, labels = _design(model, ph, idcol)
        q = [len(lab) for lab in labels]
        sol = np.zeros(sum(q))
        off = np.cumsum([0] + q)
        if t > 1:
            lhs_blocks = [[Xf[k].T @ (w64[:, None] * Xf[l]) for l in range(t)] for k in range(t)]
        else:
            lhs = Xf[0].T @ (w64[:, None] * Xf[0])
        vare = ftype(R.val) if t == 1 else np.asarray(R.val, dtype=ftype)

        # ---- accumulators and sample files (output.jl:320-437)
        run_sol, run_vare = Running(sol), Running(vare)
        ebv_run = [Running(np.zeros(len(out_ids))) for _ in range(t)] if outputEBV else None
        cov = [f"{a}_{b}" for a in model.lhsVec for b in model.lhsVec] if t > 1 else [model.lhsVec[0]]
        term_cols = term_sample_columns(model, labels, off)
        genvar = None
        files = SampleFiles(output_folder)
        t_sweep, t0 = 0.0, time.time()
        # ================================ the chain =================================================
        with host_blas_limit(), files:
            files.open("residual_variance", cov)
            for c in cats:
                Mi = c.Mi
                c.run_varg = Running(c.Gval) if not c.pervar else None
                c.run_pi = Running(np.atleast_1d(np.asarray(c.pi, dtype=np.float64))) if Mi.estimatePi else None
                c.run_scale = Running(np.atleast_1d(np.float64(Mi.G.scale))) if (Mi.G.estimate_scale and t == 1) else None
                if not c.pervar:
                    files.open(f"marker_effects_variances_{c.name}", cov if t > 1 else ["1"])
                if Mi.estimatePi:
                    npi = np.size(c.pi)
                    files.open(f"pi_{c.name}", [f"pi{i + 1}" for i in range(npi)] if npi > 1 else ["pi"])
                c.text = output_samples_for_all_parameters or c.p <= 20000
                if c.text:
                    for tr in model.lhsVec:
                        files.open(f"marker_effects_{c.name}_{tr}", Mi.markerID)
                c.writers = [files.marker_writer(f"marker_effects_{c.name}_{tr}", Mi.markerID) for tr in model.lhsVec]
            if outputEBV and output_heritability:
                genvar = GeneticVarianceSamples(files, cov, list(model.lhsVec))
            for key_, (_, header) in term_cols.items():
                files.open(key_, header)
            for it in range(1, chain_length + 1):
                # 1. location parameters (MCMC_BayesianAlphabet.jl:196-220), from the residual where it is
                if sum(q):
                    eng = resid.engine
                    if t == 1:
                        host_location_step(eng, Xf[0], lhs, sol, w64, rng, vare, ftype)
                    else:
                        Rinv = np.linalg.inv(np.asarray(vare, dtype=np.float64))
                        rr = [eng.get_residual(k).astype(np.float64) + Xf[k] @ sol[off[k]:off[k + 1]] for k in range(t)]
                        A = np.block([[Rinv[k, l] * lhs_blocks[k][l] for l in range(t)] for k in range(t)])
                        b = np.concatenate([Xf[k].T @ (w64 * sum(Rinv[k, l] * rr[l] for l in range(t))) for k in range(t)])
                        _gibbs(A, sol, b, rng, None)
                        for k in range(t):
                            eng.set_residual((rr[k] - Xf[k] @ sol[off[k]:off[k + 1]]).astype(ftype), k)
                # 2. marker effects, category by category (:224-337)
                for i, c in enumerate(cats):
                    eng = resid.move(i)
                    st = eng.sweep(iteration=it, seed=seed_int, vare=vare, nreps=1, marker_offset=c.offset, **c.sweep_kw())
                    t_sweep += st["sweep_ms"]
                    c.draw_hyper(st, rng)
                # 3. residual variance from the last category's sweep: its residual is the model's (:363-370)
                if R.estimate_variance:
                    if t > 1:
                        from scipy.stats import invwishart
                        S = np.asarray(R.scale, dtype=np.float64) + st["resid_ss"]
                        vare = np.asarray(invwishart.rvs(df=Rdf + n, scale=(S + S.T) / 2, random_state=rng), dtype=ftype).reshape(t, t)
                    else:
                        vare = ftype((ftype(st["resid_ss"][0, 0]) + Rdf * R.scale) / rng.chisquare(n + Rdf))
                # 4. save (:399-413, output.jl:443-604)
                if it > burnin and (it - burnin) % output_samples_frequency == 0:
                    k = (it - burnin) / output_samples_frequency
                    run_sol.add(sol, k)
                    run_vare.add(vare, k)
                    for key_, (cols, _) in term_cols.items():
                        files.row(key_, sol[cols])
                    files.row("residual_variance", np.atleast_1d(vare).ravel())
                    ebvs = [np.zeros(len(out_ids)) for _ in range(t)] if outputEBV else None
                    for i, c in enumerate(cats):
                        eng = c.engine
                        eng.accumulate(k)
                        if c.run_varg is not None:
                            c.run_varg.add(c.Gval, k)
                            files.row(f"marker_effects_variances_{c.name}", np.atleast_1d(c.Gval).ravel())
                        if c.run_pi is not None:
                            c.run_pi.add(np.atleast_1d(c.pi), k)
                            files.row(f"pi_{c.name}", np.atleast_1d(c.pi))
                        if c.run_scale is not None:
                            c.run_scale.add(np.atleast_1d(np.float64(c.Mi.G.scale)), k)
                        for kk, tr in enumerate(model.lhsVec):
                            si, sv = sparse_effects(eng, kk)
                            c.writers[kk].append(si, sv)
                            if c.text:                                   # run_multigeno: nine digits also under double_precision
                                files.sparse_effects_row(f"marker_effects_{c.name}_{tr}", si, sv, c.p, ftype, "%.9g")
                            if outputEBV:                                # getEBV: sum over the categories (output.jl:300-304), in double
                                if X_out_host[i] is not None:
                                    e_ = X_out_host[i] @ eng.get_state(kk)[0].astype(np.float64)
                                else:
                                    e_ = eng.mul_alpha(kk) if out_same else eng.mul_alpha_output(kk)
                                ebvs[kk] += np.asarray(e_, dtype=np.float64)
                    if outputEBV:
                        for kk in range(t):
                            ebv_run[kk].add(ebvs[kk], k)
                        if genvar is not None:                           # output.jl:498-512, from the total
                            genvar.add(ebvs, np.diag(np.atleast_2d(np.asarray(vare, dtype=np.float64))))
                if it % printout_frequency == 0 and it > burnin:
                    print_posterior_means(it, run_vare.mean)
        wall = time.time() - t0

        # ---- results (output.jl:108-212)
        out = {"location parameters": location_table(labels, off, run_sol.mean, run_sol.sd()),
               "residual variance": covariance_table(cov, run_vare)}
        for c in cats:
            # run_multigeno: the SD from the moments cast to Float64 (as run_chain)
            out[f"marker effects {c.name}"] = marker_effects_table([(tr, c.Mi.markerID) + tuple(c.engine.posterior(k)) for k, tr in enumerate(model.lhsVec)],
                                                                   sd_in_double=True)
            if c.run_varg is not None:
                out[f"marker effects variance {c.name}"] = covariance_table(cov, c.run_varg)
            if c.run_pi is not None:
                out[f"pi_{c.name}"] = pi_table(c.run_pi, pi_labels(t, c.method))
            if c.run_scale is not None:
                out[f"ScaleEffectVar{c.name}"] = covariance_table([model.lhsVec[0]], c.run_scale)
        if outputEBV:
            out.update(ebv_tables(model.lhsVec, out_ids, ebv_run))
        if genvar is not None:
            out.update(genvar.tables())
        write_tables(out, output_folder)
        out["_timing"] = {"wall_s": wall, "device_sweep_ms_total": t_sweep, "iterations": chain_length,
                          "block_size": [c.block_size for c in cats], "marker_offset": [c.offset for c in cats],
                          "n": n, "p": [c.p for c in cats]}
        return out
    finally:
        if own:
            for e in engines:
                e.close()
