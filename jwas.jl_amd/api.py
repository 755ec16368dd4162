"""Host-side mirror of the reference's user API for the marker path:
get_genotypes() / build_model() / set_covariate() / runMCMC().

Same names, argument meaning and error behaviour as reworkhow/JWAS.jl v2.3.6 (files under
/root/reference/src/1.JWAS/src/):
    get_genotypes   markers/readgenotypes.jl:213-448     (dense branch)
    build_model     build_MME.jl:42-156
    set_covariate   build_MME.jl:158-181
    runMCMC         JWAS.jl:161-511  -> MCMC/MCMC_BayesianAlphabet.jl
Everything that is NOT the marker sweep stays here on the host (numpy): data ingestion and QC,
model parsing, fixed-effect Gibbs, variance-component and pi draws, output tables.  Model families
outside the hot path (prediction equations) are rejected with an
explicit error: they stay on the reference.  GBLUP runs from a relationship matrix (genomic_relationship_matrix forms it on the device,
get_genotypes(K, G, method="GBLUP") takes it; gblup.py, csrc/gblup.hpp).  Single-step analyses (single_step_analysis=True with a pedigree) have a driver of their own
(ssbr.py: the imputation on the device, csrc/ssbr.hpp, then this chain with the terms J and ϵ).  Models with several genotype categories (y = intercept + geno1 + geno2) have a driver of
their own (multigeno.py: one device context per category, the residual handed over between them).  Random regression models (RRM=Phi) have a driver of their own (rrm.py, csrc/rrm.hpp).  i.i.d. random effects (set_random) and large class factors run on the device
(mcmc.py step 1, csrc/locpar.hpp).  Categorical / censored traits run here: their liabilities are sampled
on the device (mcmc.py step 0, csrc/liability.hpp).
"""
import inspect
import os

import numpy as np

from .mcmc import run_chain
from .gwas import GWAS  # noqa: F401  (src/3.GWAS/src/GWAS.jl)
from .rrm import generatefullPhi  # noqa: F401  (RRM/RRM.jl:24-39)

# RR-BLUP: every marker is in the model with one common effect variance -- the same full conditionals as BayesC with
# pi = 0 fixed (BayesL! with gammaArray = [1.0], BayesC0L.jl:20-47, vs bayesabc_update_marker! with probDelta1 = 1;
# variance update with nloci = nMarkers, variance_components.jl:160-162), so it runs on the device's BayesC path
# BayesL (single trait): BayesL!'s update is the device's BayesB update with pi = 0 and var_j = G*gamma_j; the gamma_j
# Metropolis-Hastings step stays on the host (mcmc.py)
SUPPORTED_METHODS = ("BayesA", "BayesB", "BayesC", "BayesR", "RR-BLUP", "BayesL")
BAYESR_DEFAULT_PI = np.array([0.95, 0.03, 0.015, 0.005])      # tools4genotypes.jl:375-377
BAYESR_GAMMA = np.array([0.0, 0.01, 0.1, 1.0])                # JWAS.jl:12


class Variance:
    """types.jl:56-64"""

    def __init__(self, val, df, scale, estimate_variance=True, estimate_scale=False, constraint=False):
        self.val, self.df, self.scale = val, df, scale
        self.estimate_variance, self.estimate_scale, self.constraint = estimate_variance, estimate_scale, constraint

    def __repr__(self):
        return f"Variance(val={self.val}, df={self.df}, scale={self.scale}, estimate_variance={self.estimate_variance})"


class Genotypes:
    """types.jl:98-165 -- the fields the marker path reads."""

    def __init__(self, obsID, markerID, nObs, nMarkers, alleleFreq, sum2pq, centered, genotypes):
        self.name = False
        self.trait_names = False
        self.obsID, self.markerID = list(obsID), list(markerID)
        self.nObs, self.nMarkers = int(nObs), int(nMarkers)
        self.alleleFreq, self.sum2pq, self.centered = alleleFreq, float(sum2pq), bool(centered)
        self.genotypes = genotypes
        self.ntraits = False
        self.genetic_variance = Variance(False, False, False)
        self.G = Variance(False, False, False)
        self.method = False
        self.estimatePi = True
        self.pi = 0.0
        self.alpha = False                      # starting values
        self.storage_mode = "dense"            # "dense" | "stream" (types.jl:149-150)
        self.stream_backend = None             # metadata of the 2-bit packed backend (streaming.load_streaming_backend)
        self.multi_trait_sampler = "I"
        self.annotations = False               # annotations.MarkerAnnotations (types.jl:167-215)


def _is_false(x):
    return x is False or x is None


def get_genotypes(file, G=False, *, method="BayesC", Pi=0.0, estimatePi=True,
                  G_is_marker_variance=False, df=4.0, estimate_variance=True, estimate_scale=False,
                  constraint=False, separator=",", header=True, double_precision=False,
                  quality_control=True, MAF=0.01, missing_value=9.0, center=True, starting_value=False,
                  annotations=False, multi_trait_sampler="I", storage="dense"):
    """readgenotypes.jl:213-448.  `file`: path of a delimited text file (first column = individual
    IDs), a pandas DataFrame (first column IDs) or a 2-D array."""
    if multi_trait_sampler not in ("auto", "I", "II"):
        raise ValueError("multi_trait_sampler must be one of :auto, :I, or :II.")            # :229-231
    if storage not in ("dense", "stream"):
        raise ValueError("storage must be :dense or :stream.")                                # :232-234
    if storage == "stream":                                                                   # :236-295
        if not isinstance(file, str):
            raise ValueError("storage=:stream requires a file path or prefix produced by prepare_streaming_genotypes.")
        if double_precision:
            raise ValueError("storage=:stream MVP supports Float32 only (double_precision=false).")
        if annotations is not False:
            raise NotImplementedError("marker annotations stay on the reference path")
        if method not in SUPPORTED_METHODS:
            raise NotImplementedError(f"method {method} is not on the device path (supported: {SUPPORTED_METHODS})")
        from .streaming import load_streaming_backend
        backend = load_streaming_backend(file)
        if center != backend["centered"]:
            print(f"The argument center={center} is ignored for storage=:stream. Backend metadata "
                  f"centered={backend['centered']} is used.")
        g = Genotypes(backend["obsID"], backend["markerID"], backend["nObs"], backend["nMarkers"],
                      backend["allele_freq"].astype(np.float32), backend["sum2pq"], backend["centered"],
                      np.zeros((backend["nObs"], 0), dtype=np.float32))
        g.storage_mode, g.stream_backend = "stream", backend
        g.G = Variance(G if G_is_marker_variance else False, df, False, estimate_variance, estimate_scale, constraint)
        g.genetic_variance = Variance(False if G_is_marker_variance else G, df, False, estimate_variance, estimate_scale, constraint)
        g.method, g.estimatePi, g.pi = method, estimatePi, Pi
        g.multi_trait_sampler = multi_trait_sampler
        print("Genotype informatin:")
        print(f"#markers: {backend['nMarkers']}; #individuals: {backend['nObs']} (storage=:stream)")
        if not _is_false(starting_value):
            sv = np.asarray(starting_value, dtype=np.float32).reshape(-1)
            if sv.size % backend["nMarkers"] != 0:
                raise ValueError("length of starting values is wrong.")
            g.alpha = sv
        return g
    if method != "GBLUP" and method not in SUPPORTED_METHODS:
        raise NotImplementedError(f"method {method} is not on the device path (supported: {SUPPORTED_METHODS}); "
                                  "GBLUP / RR-BLUP / BayesL stay on the reference")

    data_type = np.float64 if double_precision else np.float32           # readgenotypes.jl:298: Float64 genotypes on request
    obsID, markerID, genotypes = _read_genotype_table(file, separator, header, data_type)
    if method == "GBLUP":                                                                     # :352-366
        from . import gblup as _gb
        if not _gb.is_relationship_matrix(genotypes):
            raise NotImplementedError(f"method GBLUP is not on the device path (supported: {SUPPORTED_METHODS}) for a genotype covariate "
                                      "matrix: form the relationship matrix with genomic_relationship_matrix(...) and pass it")
        return _gb.relationship_genotypes(Genotypes, Variance, obsID, genotypes, G, G_is_marker_variance=G_is_marker_variance, df=df,
                                          estimate_variance=estimate_variance, estimate_scale=estimate_scale, constraint=constraint,
                                          starting_value=starting_value, Pi=Pi, estimatePi=estimatePi)

    nObs, nMarkers = genotypes.shape
    from . import annotations as _ann
    annotation_matrix = _ann.validate_annotations_input(annotations, nMarkers, method)       # :56-70, one row per RAW marker
    if annotation_matrix is not False and estimatePi is False:                                # :152-158
        print(f"estimatePi=false is ignored when annotations are provided; Annotated {method} requires estimatePi=true.")
        estimatePi = True
    genotypes, markerID, p, sum2pq, annotation_matrix = _impute_center_qc(genotypes, markerID, data_type, quality_control, MAF, missing_value, center,
                                                                          annotation_matrix)
    nObs, nMarkers = genotypes.shape

    g = Genotypes(obsID, markerID, nObs, nMarkers, p, sum2pq, center, genotypes)
    g.G = Variance(G if G_is_marker_variance else False, df, False, estimate_variance, estimate_scale, constraint)   # :424
    g.genetic_variance = Variance(False if G_is_marker_variance else G, df, False, estimate_variance, estimate_scale, constraint)
    g.method, g.estimatePi, g.pi = method, estimatePi, Pi
    g.multi_trait_sampler = multi_trait_sampler
    if annotation_matrix is not False:                                                        # :111-150
        if method == "BayesC" and not isinstance(Pi, dict):
            if np.ndim(Pi) == 1:
                if len(Pi) != nMarkers:
                    raise ValueError(f"Annotated BayesC starting Pi vector length {len(Pi)} must match the number of markers ({nMarkers}).")
                g.pi = np.array(Pi, dtype=np.float64)
            else:
                g.pi = np.full(nMarkers, float(Pi))
        g.annotations = _ann.build_marker_annotations(annotation_matrix, method, Pi)
    print("Genotype informatin:")
    print(f"#markers: {nMarkers}; #individuals: {nObs}")
    if not _is_false(starting_value):                                                         # :438-446
        sv = np.asarray(starting_value, dtype=data_type).reshape(-1)
        if sv.size % nMarkers != 0:
            raise ValueError("length of starting values is wrong.")
        g.alpha = sv
    return g


def _read_genotype_table(file, separator, header, data_type):
    """(obsID, markerID, genotypes) of a delimited text file, a DataFrame or a 2-D array (readgenotypes.jl:300-348)."""
    try:
        import pandas as pd
    except ImportError:                                              # pragma: no cover
        pd = None
    if isinstance(file, str):                                                                 # :300-327
        with open(file) as fh:
            row1 = [t.strip().strip('"') for t in fh.readline().rstrip("\r\n").split(separator) if t != ""]
        ncol = len(row1)
        markerID = [str(t) for t in row1[1:]] if header else [str(i + 1) for i in range(ncol - 1)]
        from collections import defaultdict
        # marker columns are parsed straight to Float32 (the reference's default precision): half the transient memory
        tab = pd.read_csv(file, sep=separator, header=None, skiprows=1 if header else 0,
                          dtype=defaultdict(lambda: data_type, {0: str}))
        obsID = [str(v) for v in tab.iloc[:, 0]]
        genotypes = np.asfortranarray(tab.iloc[:, 1:].to_numpy(dtype=data_type))
    elif pd is not None and isinstance(file, pd.DataFrame):                                   # :328-338
        markerID = [str(c) for c in file.columns[1:]] if header else [str(i + 1) for i in range(file.shape[1] - 1)]
        obsID = [str(v) for v in file.iloc[:, 0]]
        genotypes = np.asfortranarray(file.iloc[:, 1:].to_numpy(dtype=data_type))
    elif isinstance(file, np.ndarray) and file.ndim == 2:                                      # :339-345
        markerID = [str(i + 1) for i in range(file.shape[1])]
        obsID = [str(i + 1) for i in range(file.shape[0])]
        genotypes = np.array(file, dtype=data_type, order="F")
    else:
        raise TypeError("The data type is not supported.")                                    # :346-348

    return obsID, markerID, genotypes


def _impute_center_qc(genotypes, markerID, data_type, quality_control, MAF, missing_value, center, annotation_matrix=False):
    """The host steps between reading and the Genotypes object (readgenotypes.jl:372-401): missing values to column means, centring,
    allele frequencies, the MAF / fixed-locus filter.  Returns (genotypes, markerID, p, sum2pq, annotation_matrix)."""
    nObs, nMarkers = genotypes.shape
    if quality_control:                                                                       # :372-382
        mv = data_type(missing_value)
        for j in range(nMarkers):
            col = genotypes[:, j]
            miss = col == mv
            if miss.any():
                col[miss] = col[~miss].mean(dtype=data_type)
    if center:                                                                                # :384
        markerMeans = genotypes.mean(axis=0, dtype=data_type).astype(data_type)
        genotypes -= markerMeans[None, :]
    else:
        markerMeans = genotypes.mean(axis=0, dtype=data_type).astype(data_type)
    p = (markerMeans / data_type(2.0)).astype(data_type)                                      # :385
    if quality_control:                                                                       # :388-399
        select1 = (MAF < p) & (p < 1 - MAF)
        select2 = genotypes.var(axis=0, ddof=1) != 0
        select = select1 & select2
        genotypes = np.asfortranarray(genotypes[:, select])
        p = p[select]
        markerID = [m for m, s in zip(markerID, select) if s]
        if annotation_matrix is not False:
            annotation_matrix = annotation_matrix[select, :]
        print(f"{int((~select).sum())} loci which are fixed or have minor allele frequency < {MAF} are removed.")
    sum2pq = float((2.0 * p.astype(data_type) * (1.0 - p.astype(data_type))).sum(dtype=data_type))   # :401
    return genotypes, markerID, p, sum2pq, annotation_matrix


def _grm_divisor(p, data_type):
    """sqrt(2 p (1 - p)) of the allele frequencies in the matrix's precision (readgenotypes.jl:406)."""
    p = np.asarray(p, dtype=data_type)
    divisor = np.sqrt(data_type(2.0) * p * (data_type(1.0) - p)).astype(data_type)
    if not np.all(np.isfinite(divisor) & (divisor > 0)):
        raise ValueError("genomic_relationship_matrix needs 0 < p < 1 for every marker (a fixed locus has 2p(1-p) = 0); use quality_control=True")
    return divisor


def _grm_frame(K, obsID):
    import pandas as pd
    out = pd.DataFrame(K, columns=[str(i) for i in obsID])
    out.insert(0, "ID", [str(i) for i in obsID])
    return out


_TEXT_ONLY = object()         # default of the keywords that describe a text table: a binary input refuses them when they are given


def _grm_binary(file, input_format, text_only, keep, counted_allele, id_column, center, quality_control, MAF, double_precision, device,
                engine):
    """genomic_relationship_matrix of 2-bit packed genotypes: a PLINK fileset, a prepared .jgb2 backend, or the resident engine of a
    Genotypes object.  No text file and no dense host matrix are made."""
    resident = isinstance(file, Genotypes)
    what = "a Genotypes object" if resident else f'input_format="{input_format}"'
    if double_precision:
        raise ValueError(f"double_precision=True is not available with {what}: 2-bit packed storage has no Float64 path")
    for name, value in text_only.items():
        if value is not _TEXT_ONLY:
            raise ValueError(f'{name}= describes a text table; it is not an argument of {what}')
    if keep is not None and input_format != "plink":
        raise ValueError('keep= belongs to input_format="plink"')
    if resident:
        engine = getattr(file, "device_backend", None)
        if file.storage_mode != "device" or engine is None:
            raise ValueError("genomic_relationship_matrix takes the Genotypes object of plink_genotypes / device_genotypes (genotypes "
                             "resident on an engine); pass a storage=\"stream\" backend as its prefix with input_format=\"stream\"")
        dense = engine.storage_info()["kind"] != "packed2bit"
        if not hasattr(engine, "grm" if dense else "grm_packed"):
            raise NotImplementedError(f"genomic_relationship_matrix needs an engine with {'grm' if dense else 'grm_packed'}; the package has no CPU fallback")
        data_type = np.float64 if dense and getattr(engine, "precision", 32) == 64 else np.float32
        divisor = _grm_divisor(file.alleleFreq, data_type)
        return _grm_frame(engine.grm(divisor) if dense else engine.grm_packed(divisor), file.obsID)
    if not isinstance(file, (str, os.PathLike)):
        raise ValueError(f'{what} requires the prefix of a {".bed/.bim/.fam fileset" if input_format == "plink" else "backend produced by prepare_streaming_genotypes"}.')
    own = engine is None
    if own:
        from .engine import HipEngine
        engine = HipEngine(device)
    try:
        if not hasattr(engine, "grm_packed"):
            raise NotImplementedError("genomic_relationship_matrix needs an engine with grm_packed; the package has no CPU fallback")
        if input_format == "plink":
            from . import plink
            backend = plink.load_plink(engine, file, keep=keep, counted_allele=counted_allele, quality_control=quality_control, MAF=MAF,
                                       center=center, id_column=id_column)
        else:
            from .streaming import load_streaming_backend
            backend = load_streaming_backend(file)
            engine.load_jgb2(backend["prefix"])
        K = engine.grm_packed(_grm_divisor(backend["allele_freq"], np.float32))
    finally:
        if own:
            engine.close()
    return _grm_frame(K, backend["obsID"])


def genomic_relationship_matrix(file, *, separator=_TEXT_ONLY, header=_TEXT_ONLY, center=True, quality_control=True, MAF=0.01,
                                missing_value=_TEXT_ONLY, double_precision=False, device=0, input_format="text", keep=None,
                                counted_allele="A1", id_column="IID", _engine=None):
    """The genomic relationship matrix of a genotype covariate matrix, formed on the device (readgenotypes.jl:403-408):
    K = (Z Z' + 1e-5 I) / nMarkers with Z = genotypes ./ sqrt(2 p (1 - p)) after get_genotypes' host steps (missing values, centring,
    the MAF filter).  Returns a DataFrame with an ID column and one column per individual: what get_genotypes(K, G, method="GBLUP")
    takes.
    input_format="text" (the default): `file` as in get_genotypes -- a delimited text file (separator=",", header=True,
    missing_value=9.0), a DataFrame or a 2-D array -- read into a dense matrix of the asked precision.
    input_format="plink": `file` is a PLINK 1 binary fileset (the prefix, or the path of its .bed / .bim / .fam), loaded straight into
    2-bit packed device storage (plink.load_plink: keep = the IDs wanted in the order wanted, counted_allele "A1" or "A2", id_column
    "IID" or "FID_IID", quality control as prepare_streaming_genotypes has it); the matrix is formed from the packed storage
    (HipEngine.grm_packed) with the Float32 sqrt(2 p (1 - p)) of the scan's allele frequencies.  The rows are in keep's order.
    input_format="stream": `file` is the prefix of a backend prepare_streaming_genotypes wrote; its centring and quality control are the
    backend's.
    `file` may also be the Genotypes object of plink_genotypes / device_genotypes: the matrix comes from its resident engine (grm_packed
    on packed storage, grm on dense), which is neither reloaded nor closed, so the object still goes to runMCMC.
    A binary input is Float32 (double_precision=True is refused: packed storage has no Float64 path) and refuses separator, header and
    missing_value.  `_engine` (private) lets the test-suite inject an engine."""
    if input_format not in ("text", "plink", "stream"):
        raise ValueError('input_format must be "text", "plink" or "stream".')
    if isinstance(file, Genotypes) or input_format != "text":
        return _grm_binary(file, input_format, {"separator": separator, "header": header, "missing_value": missing_value}, keep,
                           counted_allele, id_column, center, quality_control, MAF, double_precision, device, _engine)
    if keep is not None:
        raise ValueError('keep= belongs to input_format="plink"')
    separator = "," if separator is _TEXT_ONLY else separator
    header = True if header is _TEXT_ONLY else header
    missing_value = 9.0 if missing_value is _TEXT_ONLY else missing_value
    data_type = np.float64 if double_precision else np.float32
    obsID, markerID, genotypes = _read_genotype_table(file, separator, header, data_type)
    genotypes, markerID, p, _, _ = _impute_center_qc(genotypes, markerID, data_type, quality_control, MAF, missing_value, center)
    if genotypes.shape[1] == 0:
        raise ValueError("no marker is left after quality control")
    divisor = _grm_divisor(p, data_type)
    own = _engine is None
    engine = _engine
    if own:
        from .engine import HipEngine
        engine = HipEngine(device, precision=64 if double_precision else 32)
    if not hasattr(engine, "grm"):
        raise NotImplementedError("genomic_relationship_matrix needs an engine with grm; the package has no CPU fallback")
    try:
        engine.load_dense(np.asfortranarray(genotypes, dtype=data_type))
        K = engine.grm(divisor)
    finally:
        if own:
            engine.close()
    return _grm_frame(K, obsID)


def device_genotypes(engine, G=False, *, method="BayesC", Pi=0.0, estimatePi=True, G_is_marker_variance=False, df=4.0,
                     estimate_variance=True, estimate_scale=False, constraint=False, multi_trait_sampler="I",
                     obsID=None, markerID=None, centered=True, alleleFreq=None, sum2pq=None):
    """A Genotypes object over a matrix that is ALREADY resident on the GPU (loaded or generated through `engine`, a
    HipEngine) -- the device analogue of storage=:stream, where Genotypes carries a backend handle instead of the matrix
    (types.jl:149-150, readgenotypes.jl:236-295).  Like that mode: phenotype IDs must match the genotype IDs exactly and
    in order, Float32 only.  sum2pq / alleleFreq: pass them when they are known (impute_genotypes does; the reference
    computes sum(2p(1-p)) from the column means before centring, readgenotypes.jl:385-402); otherwise they are derived from
    the device's x'x, which is exact only for CENTRED 0/1/2 genotypes with unit residual weights (x'x / n = 2pq) -- an
    uncentred or weighted resident matrix without explicit values is an error, not a silently wrong variance conversion.
    Block configurations already resident on the engine are used as they are."""
    if method not in SUPPORTED_METHODS:
        raise NotImplementedError(f"method {method} is not on the device path (supported: {SUPPORTED_METHODS})")
    if multi_trait_sampler not in ("auto", "I", "II"):
        raise ValueError("multi_trait_sampler must be one of :auto, :I, or :II.")
    n, p = int(engine.n), int(engine.p)
    if n <= 0 or p <= 0:
        raise ValueError("the engine holds no genotype matrix")
    if engine.block_size == 0:
        engine.setup_blocks(512 if p > 512 else 64, "mfma")
    if sum2pq is None or alleleFreq is None:
        if not centered:
            raise ValueError("device_genotypes(centered=False): x'x / n is 2pq + 4p^2 for an uncentred matrix; pass alleleFreq "
                             "and sum2pq explicitly")
        if getattr(engine, "_weighted", False):
            raise ValueError("device_genotypes: the engine holds residual weights (x'x is x'R^-1 x); pass alleleFreq and "
                             "sum2pq explicitly")
        xpx = engine.xpx().astype(np.float64)
        if sum2pq is None:
            sum2pq = float(xpx.sum() / n)
        if alleleFreq is None:      # allele frequency from 2pq = x'x / n (the smaller root); only marker-level-pi priors read it
            alleleFreq = 0.5 * (1.0 - np.sqrt(np.clip(1.0 - 2.0 * xpx / n, 0.0, 1.0)))
    af = np.asarray(alleleFreq, dtype=np.float32).reshape(-1)
    if af.shape != (p,):
        raise ValueError(f"alleleFreq must have one entry per marker ({p})")
    sum2pq = float(sum2pq)
    g = Genotypes(obsID if obsID is not None else [str(i + 1) for i in range(n)],
                  markerID if markerID is not None else [str(j + 1) for j in range(p)], n, p, af, sum2pq, centered,
                  np.zeros((n, 0), dtype=np.float32))
    g.storage_mode, g.device_backend = "device", engine
    g.G = Variance(G if G_is_marker_variance else False, df, False, estimate_variance, estimate_scale, constraint)
    g.genetic_variance = Variance(False if G_is_marker_variance else G, df, False, estimate_variance, estimate_scale, constraint)
    g.method, g.estimatePi, g.pi = method, estimatePi, Pi
    g.multi_trait_sampler = multi_trait_sampler
    return g


def plink_genotypes(bfile, G=False, *, keep=None, device=0, engine=None, counted_allele="A1", quality_control=True, MAF=0.01,
                    center=True, id_column="IID", method="BayesC", Pi=0.0, estimatePi=True, G_is_marker_variance=False, df=4.0,
                    estimate_variance=True, estimate_scale=False, constraint=False, multi_trait_sampler="I"):
    """A Genotypes object over a PLINK 1 binary fileset (<bfile>.bed/.bim/.fam; `bfile` is the prefix or any of the three
    paths), loaded straight into 2-bit packed device storage (plink.load_plink): what get_genotypes(prefix, storage="stream")
    gives for the backend prepare_streaming_genotypes would write of the same genotypes, without the text file, the dense
    matrix or the backend.  keep: the IDs of the individuals wanted -- the phenotyped ones, in the phenotypes' order (None: all,
    file order); counted_allele: "A1" (the .bim's first allele) or "A2".  engine: a Float32 HipEngine to load into (None: one is
    made on `device`).  The marker-model keywords are device_genotypes'."""
    if method not in SUPPORTED_METHODS:
        raise NotImplementedError(f"method {method} is not on the device path (supported: {SUPPORTED_METHODS})")
    from . import plink
    own = engine is None
    if own:
        from .engine import HipEngine
        engine = HipEngine(device)
    if getattr(engine, "precision", 32) != 32:
        raise ValueError("plink_genotypes needs a Float32 engine (2-bit packed storage has no Float64 path)")
    try:
        b = plink.load_plink(engine, bfile, keep=keep, counted_allele=counted_allele, quality_control=quality_control, MAF=MAF,
                             center=center, id_column=id_column)
        g = device_genotypes(engine, G, method=method, Pi=Pi, estimatePi=estimatePi, G_is_marker_variance=G_is_marker_variance, df=df,
                             estimate_variance=estimate_variance, estimate_scale=estimate_scale, constraint=constraint,
                             multi_trait_sampler=multi_trait_sampler, obsID=b["obsID"], markerID=b["markerID"], centered=b["centered"],
                             alleleFreq=b["allele_freq"], sum2pq=b["sum2pq"])
    except BaseException:
        if own:
            engine.close()
        raise
    g.counted_alleles, g.selected = b["counted_alleles"], b["selected"]
    g.plink_source = b["source"]               # (outputEBV(model, IDs): further individuals of the fileset become packed output rows)
    print("Genotype informatin:")
    print(f"#markers: {b['nMarkers']}; #individuals: {b['nObs']} (PLINK fileset, 2-bit packed on the device)")
    return g


class ModelTerm:
    def __init__(self, trait, name):
        self.trait, self.name = trait, name
        self.kind = "intercept" if name == "intercept" else "factor"      # factor | covariate | intercept


class Model:
    """The slice of MME (types.jl:264-346) the marker path needs."""

    def __init__(self, equations, traits, terms, M, R):
        self.model_equations = equations
        self.lhsVec = traits
        self.nModels = len(traits)
        self.modelTerms = terms                # list (per trait) of ModelTerm
        self.M = M                             # list of Genotypes
        self.R = R
        self.covVec = []
        self.MCMCinfo = None
        self.output = None
        self.output_ID = False                 # outputEBV(model, IDs); False = all genotyped individuals
        self.outputSamplesVec = []             # outputMCMCsamples(model, terms...): (trait, term) pairs
        self.traits_type = ["continuous"] * len(traits)      # "censored" | "categorical" | "categorical(binary)" (types.jl:325)
        self.thresholds = {}                   # trait index -> [-Inf, 0, ..., Inf] (types.jl:326)
        self.rndTrmVec = []                    # set_random(model, ...): RandomEffect (types.jl:217-226)
        self.ped = False                       # set_random(model, "animal", ped, G): the Pedigree (types.jl:279)
        self.pedTrmVec = False                 # ... and its terms, e.g. ["y1:animal", "y2:animal"] (types.jl:280)


class RandomEffect:
    """types.jl:217-226 -- a random effect: one term name over the traits whose equation contains it.  randomType "I": i.i.d.
    levels; "A": the polygenic effect of a pedigree -- Vinv is A-inverse (CSR, doubles) and names the pedigree's IDs, its levels; "V": an
    effect with a given Vinv over its own level names, records of the level "missing" in none -- the single-step ϵ (ssbr.py; built internally,
    set_random does not make one)."""

    def __init__(self, name, term_array, traits, Gi, randomType="I", Vinv=0, names=()):
        self.name, self.term_array, self.traits = name, term_array, traits      # "x2", ["y1:x2", "y2:x2"], [0, 1]
        self.Gi = Gi                           # Variance: val = inv(G) (False until the default prior is set), df, scale
        self.randomType, self.Vinv, self.names = randomType, Vinv, list(names)


def pedigree_structure(ped):
    """A-inverse of the pedigree (Henderson's rules with inbreeding, single_step.a_inverse) the way the reference keeps it --
    rounded through Float32 (random_effects.jl:184) -- as an exactly symmetric scipy CSR matrix of doubles with ascending columns."""
    from .single_step import a_inverse
    A = a_inverse(ped).tocsr().astype(np.float32).astype(np.float64)
    A = ((A + A.T) * 0.5).tocsr()              # (h'h is symmetric up to the order of its sums only; the library asks for exact symmetry)
    A.sum_duplicates()
    A.sort_indices()
    return A


def build_model(model_equations, R=False, *, df=4.0, estimate_variance=True, estimate_scale=False,
                constraint=False, genotypes=None, censored_trait=False, categorical_trait=False, **unsupported):
    """build_MME.jl:42-156.  Genotype terms are found the way the reference does it -- by looking the
    term name up among the caller's variables (build_MME.jl:88-120 reflects on Main) -- or through an
    explicit `genotypes={"geno": obj}` mapping.
    censored_trait / categorical_trait: lists of trait names (build_MME.jl:47-48,146-152); a censored trait reads its bounds from
    the phenotype columns <trait>_l / <trait>_u, a categorical trait is coded 1, 2, 3 ..."""
    for k in unsupported:
        raise NotImplementedError(f"build_model argument '{k}' (neural-network / censored / categorical models) "
                                  "stays on the reference path")
    censored_trait = [] if _is_false(censored_trait) else ([censored_trait] if isinstance(censored_trait, str) else [str(v) for v in censored_trait])
    categorical_trait = [] if _is_false(categorical_trait) else ([categorical_trait] if isinstance(categorical_trait, str) else [str(v) for v in categorical_trait])
    if not _is_false(R):                                                                      # :50-52
        Rm = np.atleast_2d(np.asarray(R, dtype=np.float64))
        ok = Rm.shape[0] == Rm.shape[1] and np.allclose(Rm, Rm.T)
        if ok:
            try:
                np.linalg.cholesky(Rm)
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            raise ValueError("The covariance matrix is not positive definite.")
        if Rm.shape[0] > 1:
            R = (Rm + Rm.T) / 2                  # symmetric to allclose above: exactly symmetric from here on
    if not isinstance(model_equations, str) or model_equations.strip() == "":
        raise ValueError("Model equations are wrong.\n To find an example, type ?build_model and press enter.")   # :53-56
    if estimate_scale is not False:
        raise ValueError("estimate scale for residual variance is not supported now.")        # :57-59
    caller = inspect.currentframe().f_back
    scope = dict(caller.f_globals)
    scope.update(caller.f_locals)
    if genotypes:
        scope.update(genotypes)
    eqs = [e.strip() for e in model_equations.replace("\n", ";").split(";") if e.strip()]
    lhs_names = [e.split("=")[0].strip() for e in eqs]
    for arg, names in (("categorical_trait", categorical_trait), ("censored_trait", censored_trait)):
        unknown = [v for v in names if v not in lhs_names]
        if unknown:
            raise ValueError(f"{arg}: {unknown} not among the traits of the model {lhs_names}.")
    traits, terms, M = [], [], []
    for eq in eqs:
        lhs, rhs = [s.strip() for s in eq.split("=")]
        traits.append(lhs)
        tl = []
        for name in [t.strip() for t in rhs.split("+")]:
            if "*" in name:
                raise NotImplementedError("interaction terms stay on the reference path")
            obj = scope.get(name)
            if isinstance(obj, Genotypes):                                                    # :91-96
                if obj not in M:
                    obj.name = name
                    M.append(obj)
            else:
                tl.append(ModelTerm(lhs, name))
        terms.append(tl)
    if len({Mi.name for Mi in M}) != len(M):
        raise ValueError("every genotype category needs a term name of its own")
    nModels = len(traits)
    if not _is_false(R) and np.atleast_2d(np.asarray(R)).shape[0] != nModels:                 # :67-69
        raise ValueError(f"The residual covariance matrix is not a {nModels} by {nModels} matrix.")
    for Mi in M:                                                                              # :98-116
        Mi.ntraits = nModels
        Mi.trait_names = traits
        if Mi.multi_trait_sampler == "II":
            if Mi.method != "BayesC":
                raise ValueError("multi_trait_sampler overrides are supported for BayesC only.")
            if nModels <= 1:
                raise ValueError("multi_trait_sampler overrides require multi-trait BayesC.")
        for V in (Mi.G, Mi.genetic_variance):
            if not _is_false(V.val) and np.atleast_2d(np.asarray(V.val)).shape[0] != nModels:
                raise ValueError(f"The genomic covariance matrix is not a {nModels} by {nModels} matrix.")
        if nModels != 1:
            Mi.G.df = Mi.G.df + nModels
            Mi.genetic_variance.df = Mi.genetic_variance.df + nModels
    if nModels == 1:                                                                          # :128-134
        Rv = False if _is_false(R) else np.float32(R)
        scale_R = False if _is_false(R) else float(R) * (df - 2) / df
        df_R = df
    else:
        Rv = False if _is_false(R) else np.asarray(R, dtype=np.float32)
        scale_R = False if _is_false(R) else np.asarray(R, dtype=np.float64) * (df - 1)
        df_R = df + nModels
    model = Model(model_equations, traits, terms, M, Variance(Rv, np.float32(df_R), scale_R, estimate_variance, estimate_scale, constraint))
    for k, tr in enumerate(traits):                                                           # :146-152
        if tr in censored_trait:
            model.traits_type[k] = "censored"
        elif tr in categorical_trait:
            model.traits_type[k] = "categorical"
    return model


def outputEBV(model, IDs):
    """output.jl:60-70: individuals of interest for EBV output (default: all genotyped individuals)."""
    model.output_ID = [str(i) for i in IDs]


def outputMCMCsamples(model, *terms):
    """output.jl:76-95: also save the MCMC samples of these location-parameter terms (MCMC_samples_<trait>.<term>.txt)."""
    for trm in terms:
        for tr, tl in zip(model.lhsVec, model.modelTerms):
            if any(mt.name == trm for mt in tl) and (tr, trm) not in model.outputSamplesVec:
                model.outputSamplesVec.append((tr, trm))


def set_random(model, randomStr, *args, G=False, df=4.0, estimate_variance=True, estimate_scale=False, constraint=False,
               Vinv=0, names=()):
    """random_effects.jl:52,93-191.  set_random(model, "herd", G): the class factor is an i.i.d. random effect with covariance G
    among the k traits whose equation contains it.  set_random(model, "animal", ped, G) with a single_step.Pedigree: the polygenic
    effect, covariance A (x) G among the animals of the pedigree; its levels are the pedigree's IDs in pedigree order (one per
    model).  G = False: a default prior from the data (input_data_validation.jl:352-365).  The variance is sampled every iteration
    (sampleVCs, variance_components.jl:115-147) unless estimate_variance=False.  Vinv / names random effects and several
    correlated terms in one call stay on the reference."""
    from .single_step import Pedigree
    ped = None
    if args and isinstance(args[0], Pedigree):                                                # :52
        ped, args = args[0], args[1:]
    if len(args) > 1 or (args and not _is_false(G)):
        raise TypeError("set_random(model, randomStr[, ped][, G]; ...)")
    if args:
        G = args[0]
    if not _is_false(G):                                                                      # :100-104
        Gm = np.atleast_2d(np.asarray(G, dtype=np.float64))
        ok = Gm.ndim == 2 and Gm.shape[0] == Gm.shape[1] and np.array_equal(Gm, Gm.T)
        if ok:
            try:
                np.linalg.cholesky(Gm)
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            raise ValueError("The covariance matrix is not positive definite.")
    if constraint is not False:                                                               # :108-113
        raise ValueError("Constraint for variance of random term is not supported now.")
    if estimate_scale is not False:
        raise ValueError("Estimate scale for variance of random term is not supported now.")
    if not (np.isscalar(Vinv) and Vinv == 0) or len(names) != 0:
        raise NotImplementedError("set_random with Vinv and names (a user-given covariance structure among the levels) stays on the "
                                  "reference; the device path runs i.i.d. random effects and the pedigree form set_random(model, trm, ped, G)")
    trms = str(randomStr).split()
    if len(trms) != 1:
        raise NotImplementedError("set_random with several term names in one call (correlated terms within a trait) stays on "
                                  "the reference; call set_random once per term for independent effects")
    trm = trms[0]
    if trm == "ϵ":
        raise NotImplementedError("the single-step term ϵ stays on the reference")
    traits = [k for k, tl in enumerate(model.modelTerms) if any(mt.name == trm for mt in tl)]
    for k in range(model.nModels):
        if k not in traits:
            print(f"{trm} is not found in model equation {k + 1}.")
    if not traits:
        raise ValueError(f"{trm} is not found in model equation.")                            # :135-137
    if any(re_.name == trm for re_ in model.rndTrmVec):
        raise ValueError(f"{trm} is already a random effect.")
    if ped is not None and any(re_.randomType == "A" for re_ in model.rndTrmVec):
        raise ValueError("a model has one pedigree (polygenic) random effect; animal + maternal effects stay on the reference")
    k = len(traits)
    if not _is_false(G) and Gm.shape[0] != k:                                                 # :156-158
        raise ValueError(f"Dimensions must match. The covariance matrix (G) should be a {k} x {k} matrix.\n")
    dfk = np.float32(df) + k                                                                  # :182-185
    if _is_false(G):
        Gi, scale = False, False
    else:
        Gi = np.linalg.inv(Gm.astype(np.float32))                                             # inv(Float32.(G)) (:162)
        Gi = (Gi + Gi.T) / 2
        scale = Gm * (float(dfk) - k - 1)
    term_array = [f"{model.lhsVec[m]}:{trm}" for m in traits]
    var = Variance(Gi, dfk, scale, estimate_variance, estimate_scale, constraint)              # (df, scale of :168-171 and :182-183 coincide)
    if ped is None:
        model.rndTrmVec.append(RandomEffect(trm, term_array, traits, var))
    else:                                                                                     # :141-143,164-172
        model.ped, model.pedTrmVec = ped, term_array
        model.rndTrmVec.append(RandomEffect(trm, term_array, traits, var, "A", pedigree_structure(ped), ped.ids))


def set_covariate(model, *names):
    """build_MME.jl:158-181: declare terms as continuous covariates (default is a class factor)."""
    flat = []
    for n in names:
        flat.extend(n.split())
    model.covVec.extend(flat)
    for tl in model.modelTerms:
        for t in tl:
            if t.name in flat:
                t.kind = "covariate"


def runMCMC(model, df, *, heterogeneous_residuals=False, chain_length=100, starting_value=False, burnin=0,
            output_samples_frequency=None, update_priors_frequency=0, single_step_analysis=False, pedigree=False,
            causal_structure=False, missing_phenotypes=True, RRM=False, outputEBV=True, output_heritability=True,
            prediction_equation=False, seed=False, printout_model_info=True, printout_frequency=None,
            big_memory=False, double_precision=False, fast_blocks=False, independent_blocks=False,
            memory_guard="error", memory_guard_ratio=0.80, output_folder="results",
            output_samples_for_all_parameters=False,
            # device options (the analogue of storage=:stream's opt-in knobs)
            device=0, block_size=None, gram_mode="mfma", blocks_per_launch=None, location_parameters="auto",
            annotation_priors="host", fitting_J_vector=True, chains=1, first_chain=0, bayesr_gamma=None, gblup_eigen="auto", _engine=None):
    """JWAS.jl:161-511.  Returns the reference's output Dict (output.jl:108-212) as a dict of pandas
    DataFrames and writes the same text files under `output_folder`.

    fast_blocks: False -> the exact non-block chain (computed on the device in blocks with one
    within-block pass, algebraically identical: SURVEY.md section 7 step 4); True / number -> the
    reference's fast_blocks schedule (block-size repetitions, chain_length rescaled, JWAS.jl:293-316).
    independent_blocks=True (needs fast_blocks): every block starts from the same residual snapshot and all blocks are
    sampled concurrently on the device (BayesABC.jl:190-255) -- the reference's approximate parallel mode.
    `_engine` (private, not part of the reference's surface) lets the test-suite inject a sweep engine; the default and
    only shipped engine is HipEngine.
    blocks_per_launch (device option, like block_size): None = by the chain's length (mcmc.grouped_blocks_for_chain: 2 from
    3 000 iterations on, 4 from 8 000), 0 / 2 / 4 = one / two / four 1024-marker blocks per launch of the step kernel in the
    sparse steady state of a single-trait chain (grouped launches) -- the same chain up to float32
    rounding of the block right-hand sides; the group cross-Grams are set-up work (8 / 24 KB per marker).

    location_parameters (device option): where step 1, the non-marker location parameters, runs.  "host": the dense host scan
    (intercepts, covariates and small fixed factors).  "device": term by term on the device from the resident residual
    (csrc/locpar.hpp) -- factors of any number of levels, the i.i.d. random effects of set_random and its pedigree form (the polygenic
    effect, sampled colour by colour over the graph of A-inverse; EBVs and heritability include it), residual weights, threshold
    traits, and multi-trait records that miss some traits (their missing residuals are imputed on the device and every record is
    weighted with the inverse of its observed block of R until the first residual-variance draw, csrc/mtmiss.hpp).  "auto": "device"
    for a model with a set_random term or more than 2 048 location-parameter levels, else "host" -- the host path draws from the
    numpy generator, the device path from the counter generator, so the choice is part of what a seed means; a fixed-only model
    with partially missing multi-trait records stays on "host" under "auto".

    annotation_priors (device option): where the probit update of the annotation coefficients between two sweeps runs (annotated
    BayesC, BayesR and 2-trait BayesC).  "host" (the default): annotations.py from the downloaded indicators, every draw from the
    numpy generator.  "device": csrc/annot.hpp from the resident indicators -- liabilities, the coefficient scan and the rebuilt
    per-marker prior table stay on the device, the sweep reads the table in place, only the coefficients and a few sums come back;
    the liabilities and the coefficients' normals come from the counter generator, the shrinkage variances stay on the numpy
    generator.  The choice is therefore part of what a seed means, as with location_parameters.  Not with storage=:stream,
    constraint=true or marker shards (explicit errors).

    Several genotype categories (build_model("y = intercept + geno1 + geno2"); `for Mi in mme.M`, MCMC_BayesianAlphabet.jl:224-337): a
    driver of its own (multigeno.py).  Every category is a device context with its own method, Pi, variances, block size and outputs
    ("marker effects <name>", "pi_<name>", MCMC_samples_marker_effects_<name>_<trait>.txt, ..._variances_<name>.txt, ...pi_<name>.txt);
    the one residual moves between the contexts on the device (jwas_hip_residual_handover) and category i draws from the counters
    after those of the categories before it.  EBVs, genetic_variance and heritability are those of the sum over the categories;
    the default genetic variance is var(y) / 2 / (number of categories) each.  Single-trait BayesA/B/C/R, RR-BLUP, BayesL chosen
    per category; multi-trait (2-4 traits, complete records) BayesC under samplers I and II and RR-BLUP; dense or storage=:stream
    per category; Float32, or double_precision=True with every category dense Float64; heterogeneous_residuals; outputEBV(model, IDs)
    for dense categories; location parameters on the host.  `_engine`: a list with one engine per category.  All categories must
    hold the same individuals ("genotypic information is not provided for same individuals").  Not with fast_blocks,
    independent_blocks, location_parameters="device", set_random, categorical / censored traits, causal_structure, RRM, annotations,
    marker starting values, constraint=true, multi-trait BayesA/B/L, missing traits, device_genotypes or marker shards (explicit
    errors); the adaptive block-size switching, grouped launches and the section solve are off in this driver.

    More than 4 traits (5 to 64; megaBayesABC! / megaBayesC0!, markers/BayesianAlphabet/BayesABC.jl:1-8): a driver of its own
    (megatrait.py) with the marker sweep of all traits in one pass over the genotypes on the device (csrc/mega.hpp).  The model
    needs constraint=True in BOTH get_genotypes and build_model (zero genetic and residual covariances: t independent single-trait
    chains), one genotype category, BayesC (estimatePi true or false; Pi a scalar or one value per trait) or RR-BLUP, dense
    storage, Float32 or double_precision=True; records may miss some traits (their residuals are redrawn on the device every
    iteration); location parameters on the host; block_size <= 256 (default 256).  Outputs as a multi-trait constraint=true run of
    1 to 4 traits writes them: marker effects <genotypes>, pi_<genotypes> (one per trait), marker effects variance <genotypes>,
    residual variance, EBV_<trait>, genetic_variance, heritability, the MCMC_samples_* files and the sparse .bin marker samples;
    outputEBV(model, IDs) covers genotyped individuals without records.  Everything else with more than 4 traits raises
    NotImplementedError naming the argument before anything is written: no constraint=True on either side (the joint 2^t-state
    samplers), BayesA/B/L/R, annotations, storage=:stream, fast_blocks, independent_blocks, heterogeneous_residuals,
    location_parameters="device", set_random, categorical / censored traits, causal_structure, RRM, several genotype categories,
    starting values, shards, more than 64 traits.
    More than 4 traits WITHOUT constraints (5 to 8, constraint=False -- the default -- in both get_genotypes and build_model): Gibbs
    sampler I (_MTBayesABC_samplerI!, MTBayesABC.jl:57-127) with a full t x t marker-effect covariance, a full residual covariance and
    Pi over the 2^t joint states, a driver of its own (mtjoint.py) on a device session of its own (csrc/mtjoint.hpp; it runs on the
    block form of the mega-trait session).  BayesC (Pi: the scalar default = all mass on the all-ones state, a Dict over all 2^t joint
    states, or a vector of 2^t probabilities; estimatePi true or false) and RR-BLUP; one genotype category, dense storage, Float32 or
    double_precision=True, complete records, location parameters on the host, block_size <= 256 (default 256).  Outputs as an
    unconstrained run of 2 to 4 traits writes them: full t x t covariance tables and sample files, pi_<genotypes> over the joint
    states, marker effects with Model_Frequency, EBVs, genetic_variance and heritability.  Not on this path (NotImplementedError
    naming the argument, before anything is written): records that miss some traits, BayesA/B/L/R, sampler II, annotations,
    fast_blocks, independent_blocks, weights, set_random, location_parameters="device", categorical / censored traits,
    causal_structure, RRM, single-step, starting values, storage=:stream, device_genotypes, several genotype categories, shards,
    chains, more than 8 traits.  constraint=True on one side only is an error as before.  Speed (scripts/mega_bench.py, 20 000 x 100 000, pi = 0.95, one MI355X): 25.3 ms per
    sweep at 8 traits and 39.4 at 64, against 14.8 ms per FOUR traits on the existing MegaBayesC sweep -- 1.17 and 6.0 times as fast
    per trait; below about 7 traits the session is slower per trait than that sweep (0.65 of its speed at 4): NOTES.md, "Mega-trait
    models".

    single_step_analysis=True, pedigree=ped (a single_step.Pedigree), fitting_J_vector=True (JWAS.jl:173; single_step/SSBR.jl): single-step
    Bayesian regression over genotyped and non-genotyped relatives -- a driver of its own (ssbr.py).  The genotypes of the non-genotyped
    pedigree members are imputed on the device (csrc/ssbr.hpp: a sparse solve on the host's LU of A^nn, one thread per marker), the
    model gains the covariate J and the imputation residual ϵ (a random effect with Vinv = A^nn over the non-genotyped individuals,
    prior covariance = the genetic variance, which must be given) per trait, and the chain runs on the resident imputed matrix with
    the location parameters on the device.  EBVs for every pedigree member (or the outputEBV(model, IDs) list within the pedigree):
    Mout alpha + J sol[J] + sol[ϵ]; "location parameters" lists J and ϵ, their samples go to MCMC_samples_<trait>.J.txt / .ϵ.txt, ϵ's
    variance to MCMC_samples_<trait>:ϵ_..._variances.txt; no heritability table.  1 to 4 traits with complete records, every sampler,
    both precisions, residual weights, i.i.d. set_random effects.  Not with storage=:stream (the reference's error), device_genotypes,
    location_parameters="host", a set_random pedigree effect in the same model, categorical / censored traits, marker starting
    values, causal_structure, RRM, several genotype categories, more than 4 traits or shards (explicit errors).  Without
    pedigree=... the flag stays refused.

    RRM (JWAS.jl:177,464-475; RRM/RRM.jl, RRM/MCMC_BayesianAlphabet_RRM.jl): a T x c numeric matrix Phi, one row per distinct time point
    (ascending; generatefullPhi builds normalised Legendre columns) -- the random regression model for longitudinal records: the
    first column of df holds the IDs, the column `time` the time point of every record, every marker carries c coefficients.  A
    driver of its own (rrm.py) with the marker sweep on the device (csrc/rrm.hpp): one trait, BayesC, estimatePi true or false,
    both precisions, 2 <= c <= 4, T <= 64, uniform blocks (block_size <= 256, default 64), location parameters on the host.  The
    coefficients are the "traits" "1" ... "c" of the outputs: marker effects <genotypes>, pi_<genotypes>, residual variance,
    EBV_1 ... EBV_c, genetic_variance (no heritability, as in the reference).  Any other non-false value stays on the reference.

    causal_structure (JWAS.jl:144-147,328-337; structure_equation_model/SEM.jl): a t x t strictly lower 0/1 matrix, entry [i, j] = 1
    when trait j acts on trait i -- the recursive structural equation model of Wang et al. 2020.  The structural coefficients are
    sampled on the device after the residual-variance draw of every iteration (csrc/sem.hpp); the residual the chain runs on is
    the reference's "Lambda ycorr".  missing_phenotypes = false and R.constraint = true are forced as in the reference.  Outputs:
    structure_coefficient_MCMC_samples.txt (vec(Lambda) column-major per saved sample, no header; in the output folder, where the
    reference writes to the working directory), MCMC_samples_indirect_marker_effects_* / MCMC_samples_overall_marker_effects_*,
    direct_ / indirect_ / overall_marker_effects_<genotypes>.txt, and the tables "indirect marker effects <genotypes>", "overall
    marker effects <genotypes>", "structure coefficients".  Every sampler, storage mode and precision; not with categorical or
    censored traits, heterogeneous_residuals, marker shards or marker starting values (explicit errors).

    Categorical / censored traits (build_model(...; categorical_trait, censored_trait)): categories coded 1, 2, 3 ... (two of them
    make a binary trait), bounds of a censored trait in the columns <trait>_l / <trait>_u; the liabilities are sampled on the
    device before the location parameters of every iteration (mcmc.py step 0) and saved, with the thresholds, as
    MCMC_samples_liabilities_<trait>.txt / MCMC_samples_threshold_<trait>.txt.  Every sampler, storage mode and precision.

    chains=K, first_chain=0, bayesr_gamma=None (device options; chains.py): K in 2..64 chains of ONE single-trait model with different
    seeds in one device session (the genotypes uploaded once, one pass over them per sweep for all chains; csrc/mega.hpp) and the
    potential scale reduction factor of Gelman and Rubin over the chains.  chains=1 (the default) is the single-chain path,
    untouched.  BayesC (estimatePi true or false), RR-BLUP and BayesR (the default gamma, or bayesr_gamma = four multipliers starting
    with 0); one genotype category, dense Float32 or double_precision=True, block_size <= 256 (default 256), location parameters
    on the host, outputEBV(model, IDs).  Chain k draws on the device with the counter id first_chain + k and on the host from
    default_rng([seed, first_chain + k]): chain k of a K-chain run equals that chain run alone (chains=2, first_chain=k takes its
    first chain).  All chains start from the reference's starting state (no over-dispersed starts).  Outputs: chain_<id>/ with the
    reference's files of every chain, PSRF.txt (every marker effect on the device, pi and the variances on the host),
    PSRF_summary.txt, the usual tables pooled over the chains; the returned dict also holds "chains", "PSRF", "PSRF_summary".
    Everything else (BayesA/B/L, fast_blocks, independent_blocks, heterogeneous_residuals, set_random, categorical / censored traits,
    annotations, starting values, storage=:stream, device_genotypes, shards, single_step_analysis, RRM, causal_structure,
    location_parameters="device", several traits or categories) raises NotImplementedError naming the argument before anything
    is written.  Against K sequential runs: NOTES.md, "Several chains in one session".

    GBLUP (get_genotypes(K, G, method="GBLUP") with K a relationship matrix, e.g. from genomic_relationship_matrix; GBLUP.jl, gblup.py,
    csrc/gblup.hpp): the sampler on pseudo-markers inside this chain -- K aligned to the records and eigendecomposed (gblup_eigen="auto" |
    "host" | "device": numpy.linalg.eigh in the run's precision, or torch.linalg.eigh on the GPU in a child process, solved in Float64;
    "auto" takes the device from 8 192 records when it is usable), the eigenvectors resident on the device, per iteration three passes
    over them for all traits.  One trait, 2 to 4 traits jointly or with constraint=true (complete records), Float32 or
    double_precision=True (as in get_genotypes), location parameters on host or device, i.i.d. set_random effects, outputEBV(model,
    IDs) within K's IDs.  Outputs as RR-BLUP with the pseudo-markers "1" ... "n"; the variance samples go to
    MCMC_samples_genetic_variance(REML)_<genotypes>.txt.  Raises before anything is written: single_step_analysis ("SSGBLUP is not
    available"), G given as marker variance, fast_blocks, independent_blocks, heterogeneous_residuals, annotations, categorical /
    censored traits, causal_structure, RRM, chains, several genotype categories, records that miss some traits, pedigree random effects,
    shards, device_genotypes, an engine without the gblup_* methods.

    double_precision=True (JWAS.jl:349-366): genotypes, residual, effects and the samplers' arithmetic all Float64 -- a
    Float64 device context (jwas_hip_set_precision; csrc/f64_path.hpp): single-trait BayesA/B/C, RR-BLUP, BayesL, BayesR,
    multi-trait BayesC and BayesA/B under sampler I and II and marker-specific joint priors on dense storage; any fast_blocks
    partition of blocks <= 1024 markers, independent_blocks, residual weights.  Its outputs are formed on the device as well:
    the EBVs of outputEBV(model, IDs) from a second resident Float64 matrix, saved samples read out as sparse lists.  Not in
    Float64: constraint=true, storage=:stream, shards (explicit errors).  The sample files keep their Float32 / 9-digit format."""
    if independent_blocks and fast_blocks is False:
        raise ValueError("independent_blocks=true requires fast_blocks != false.")             # :242-244
    from . import rrm as _rrm
    from . import megatrait as _mt
    from . import mtjoint as _mj
    from . import gblup as _gb
    if _gb.routes(model):                     # GBLUP: mcmc.run_chain with the pseudo-marker step (gblup.py), validated before anything is written
        _gb.validate(model, df, single_step_analysis=single_step_analysis, fast_blocks=fast_blocks, independent_blocks=independent_blocks,
                     heterogeneous_residuals=heterogeneous_residuals, causal_structure=causal_structure, RRM=RRM, chains=chains,
                     engine=_engine, gblup_eigen=gblup_eigen, double_precision=bool(double_precision))
    elif gblup_eigen not in ("auto", "host", "device"):
        raise ValueError('gblup_eigen must be "auto", "host" or "device".')
    if not (isinstance(chains, (int, np.integer)) and not isinstance(chains, bool) and int(chains) == 1):
        from . import chains as _ch             # several chains of one model: a driver of its own (chains.py), validated before anything is written
        nchains = _ch.check_chains(chains)
        for flag, name in ((update_priors_frequency, "update_priors_frequency"), (prediction_equation, "prediction_equation")):
            if not _is_false(flag) and flag != 0:
                raise NotImplementedError(f"runMCMC(...; {name}=...) is outside the device marker path and stays on the reference")
        if location_parameters not in ("auto", "host", "device"):
            raise ValueError('location_parameters must be "auto", "host" or "device".')
        _ch.validate(model, df, chains=nchains, first_chain=first_chain, fast_blocks=fast_blocks, independent_blocks=independent_blocks,
                     causal_structure=causal_structure, RRM=RRM, location_parameters=location_parameters,
                     heterogeneous_residuals=heterogeneous_residuals, starting_value=starting_value, block_size=block_size,
                     single_step_analysis=single_step_analysis, annotation_priors=annotation_priors, bayesr_gamma=bayesr_gamma, engine=_engine)
        if output_samples_frequency is None:
            output_samples_frequency = chain_length // 1000 if chain_length > 1000 else 1      # :168
        if int(output_samples_frequency) <= 0:
            raise ValueError("output_samples_frequency should be an integer > 0.")
        myfolder, folderi = output_folder, 1
        while os.path.exists(output_folder):                            # an existing output folder is never overwritten (JWAS.jl:255-262)
            print(f"The folder {output_folder} already exists.")
            output_folder = myfolder + str(folderi)
            folderi += 1
        os.makedirs(output_folder)
        return _ch.run_chains(model, df, chains=nchains, first_chain=int(first_chain), chain_length=int(chain_length), burnin=int(burnin),
                              output_samples_frequency=int(output_samples_frequency), seed=seed, double_precision=bool(double_precision),
                              outputEBV=outputEBV, output_heritability=bool(output_heritability), output_folder=output_folder,
                              printout_frequency=chain_length + 1 if printout_frequency is None else printout_frequency, device=device,
                              block_size=block_size, bayesr_gamma=bayesr_gamma, engine=_engine, printout_model_info=printout_model_info,
                              output_samples_for_all_parameters=output_samples_for_all_parameters)
    if first_chain != 0 or bayesr_gamma is not None:
        raise ValueError("first_chain and bayesr_gamma apply to runMCMC(...; chains=K) with K >= 2.")
    megatrait = _mt.routes(model)             # more than 4 traits: a driver of its own (megatrait.py), validated before anything is written
    mtjoint = megatrait and _mj.routes(model)    # ... without constraints on either side: Gibbs sampler I with full covariances (mtjoint.py)
    if mtjoint:
        megatrait = False
        _mj.validate(model, df, fast_blocks=fast_blocks, independent_blocks=independent_blocks, causal_structure=causal_structure, RRM=RRM,
                     location_parameters=location_parameters, heterogeneous_residuals=heterogeneous_residuals, starting_value=starting_value,
                     block_size=block_size, single_step_analysis=single_step_analysis, annotation_priors=annotation_priors, engine=_engine)
    if megatrait:
        _mt.validate(model, df, fast_blocks=fast_blocks, independent_blocks=independent_blocks, causal_structure=causal_structure, RRM=RRM,
                     location_parameters=location_parameters, heterogeneous_residuals=heterogeneous_residuals, starting_value=starting_value,
                     block_size=block_size, single_step_analysis=single_step_analysis, annotation_priors=annotation_priors, engine=_engine)
    multigeno = len(model.M) > 1              # several genotype categories: a driver of its own (multigeno.py), validated before anything is written
    if multigeno:
        from . import multigeno as _mg
        for flag, name in ((single_step_analysis, "single_step_analysis"), (update_priors_frequency, "update_priors_frequency"),
                           (prediction_equation, "prediction_equation")):
            if not _is_false(flag) and flag != 0:
                raise NotImplementedError(f"runMCMC(...; {name}=...) is outside the device marker path and stays on the reference")
        if location_parameters not in ("auto", "host", "device"):
            raise ValueError('location_parameters must be "auto", "host" or "device".')
        _engine = _mg.validate(model, df, fast_blocks=fast_blocks, independent_blocks=independent_blocks,
                               location_parameters=location_parameters, causal_structure=causal_structure, RRM=RRM,
                               starting_value=starting_value, double_precision=bool(double_precision), engines=_engine)
    rrm_phi = None
    if _rrm.is_phi(RRM):                                                                       # JWAS.jl:464-475
        for flag, name in ((single_step_analysis, "single_step_analysis"), (update_priors_frequency, "update_priors_frequency"),
                           (prediction_equation, "prediction_equation")):
            if not _is_false(flag) and flag != 0:
                raise NotImplementedError(f"runMCMC(...; {name}=...) is outside the device marker path and stays on the reference")
        if location_parameters not in ("auto", "host", "device"):
            raise ValueError('location_parameters must be "auto", "host" or "device".')
        rrm_phi = _rrm.validate(model, df, RRM, fast_blocks=fast_blocks, independent_blocks=independent_blocks,
                                causal_structure=False if _is_false(causal_structure) else causal_structure,
                                location_parameters=location_parameters, heterogeneous_residuals=heterogeneous_residuals,
                                starting_value=starting_value, block_size=block_size, engine=_engine)
        RRM = False
    single_step = not _is_false(single_step_analysis) and single_step_analysis != 0 and not _is_false(pedigree)
    for flag, name in ((False if single_step else single_step_analysis, "single_step_analysis"), (RRM, "RRM"),
                       (update_priors_frequency, "update_priors_frequency"),
                       (prediction_equation, "prediction_equation")):
        if not _is_false(flag) and flag != 0:
            raise NotImplementedError(f"runMCMC(...; {name}=...) is outside the device marker path and stays on the reference")
    if not model.M:
        raise NotImplementedError("models without a genotype term have no marker sweep: use the reference")
    if location_parameters not in ("auto", "host", "device"):
        raise ValueError('location_parameters must be "auto", "host" or "device".')
    if annotation_priors not in ("host", "device"):
        raise ValueError('annotation_priors must be "host" or "device".')
    if memory_guard not in ("error", "warn", "off"):
        raise ValueError("memory_guard must be :error, :warn or :off.")
    if _is_false(causal_structure):
        causal_structure = False
    else:                                                                                     # JWAS.jl:328-337
        causal_structure = np.asarray(causal_structure, dtype=np.float64)
        tt = model.nModels
        if tt == 1:
            raise ValueError("Causal strutures are only allowed in multi-trait analysis")      # input_data_validation.jl:131-133
        if causal_structure.ndim != 2 or causal_structure.shape != (tt, tt):
            raise ValueError(f"causal_structure must be a {tt} x {tt} matrix (one row and column per trait).")
        if not np.all((causal_structure == 0.0) | (causal_structure == 1.0)):
            raise ValueError("causal_structure must hold 0 and 1 only.")
        if np.any(np.triu(causal_structure, 1) != 0.0):
            raise ValueError("The causal structue needs to be a lower triangular matrix.")     # :334-336
        if np.any(np.diag(causal_structure) != 0.0):
            raise ValueError("causal_structure must have a zero diagonal (a trait does not act on itself).")
        if tt > 4:
            raise NotImplementedError("causal_structure runs with at most 4 traits on the device")
        missing_phenotypes = False          # no missing phenotypes and a diagonal residual covariance, for identifiability (:331-333)
        model.R.constraint = True
    ss_plan = None
    if single_step:                           # a driver of its own (ssbr.py), validated before anything is written
        from . import ssbr as _ss
        if causal_structure is not False:
            raise NotImplementedError("runMCMC(...; single_step_analysis=..., causal_structure=...) stays on the reference")
        ss_plan = _ss.validate(model, df, pedigree, fitting_J_vector=fitting_J_vector, location_parameters=location_parameters,
                               double_precision=bool(double_precision), outputEBV=bool(outputEBV), engine=_engine)
    if output_samples_frequency is None:
        output_samples_frequency = chain_length // 1000 if chain_length > 1000 else 1          # :168
    if int(output_samples_frequency) <= 0:
        raise ValueError("output_samples_frequency should be an integer > 0.")                # input_data_validation.jl:14-16
    for Mi in model.M:                                                                        # :19-23
        if Mi.method not in ("BayesL", "BayesC", "BayesB", "BayesA", "BayesR", "RR-BLUP", "GBLUP"):
            raise ValueError(f"{Mi.method} is not available in JWAS. Please read the documentation.")
    if printout_frequency is None:
        printout_frequency = chain_length + 1
    # an existing output folder is never overwritten (JWAS.jl:255-262)
    myfolder, folderi = output_folder, 1
    while os.path.exists(output_folder):
        print(f"The folder {output_folder} already exists.")
        output_folder = myfolder + str(folderi)
        folderi += 1
    os.makedirs(output_folder)
    if multigeno:
        return _mg.run_multigeno(model, df, chain_length=int(chain_length), burnin=int(burnin),
                                 output_samples_frequency=int(output_samples_frequency), seed=seed,
                                 heterogeneous_residuals=bool(heterogeneous_residuals), double_precision=bool(double_precision),
                                 outputEBV=outputEBV, output_heritability=bool(output_heritability), output_folder=output_folder,
                                 printout_frequency=printout_frequency, memory_guard=memory_guard, memory_guard_ratio=memory_guard_ratio,
                                 device=device, block_size=block_size, gram_mode=gram_mode, engines=_engine,
                                 printout_model_info=printout_model_info, output_samples_for_all_parameters=output_samples_for_all_parameters)
    if mtjoint:
        return _mj.run_mtjoint(model, df, chain_length=int(chain_length), burnin=int(burnin), output_samples_frequency=int(output_samples_frequency),
                               seed=seed, double_precision=bool(double_precision), outputEBV=outputEBV,
                               output_heritability=bool(output_heritability), output_folder=output_folder, printout_frequency=printout_frequency,
                               device=device, block_size=block_size, engine=_engine, printout_model_info=printout_model_info,
                               output_samples_for_all_parameters=output_samples_for_all_parameters)
    if megatrait:
        return _mt.run_megatrait(model, df, chain_length=int(chain_length), burnin=int(burnin),
                                 output_samples_frequency=int(output_samples_frequency), seed=seed, double_precision=bool(double_precision),
                                 outputEBV=outputEBV, output_heritability=bool(output_heritability), output_folder=output_folder,
                                 printout_frequency=printout_frequency, missing_phenotypes=missing_phenotypes, device=device,
                                 block_size=block_size, engine=_engine, printout_model_info=printout_model_info,
                                 output_samples_for_all_parameters=output_samples_for_all_parameters)
    if rrm_phi is not None:
        return _rrm.run_rrm(model, df, rrm_phi, chain_length=int(chain_length), burnin=int(burnin),
                            output_samples_frequency=int(output_samples_frequency), seed=seed, double_precision=bool(double_precision),
                            outputEBV=outputEBV, output_heritability=bool(output_heritability), output_folder=output_folder,
                            printout_frequency=printout_frequency, device=device, block_size=block_size, engine=_engine,
                            printout_model_info=printout_model_info)
    if ss_plan is not None:
        return _ss.run_single_step(model, df, pedigree, ss_plan, double_precision=bool(double_precision), device=device, engine=_engine,
                                   memory_guard=memory_guard, memory_guard_ratio=memory_guard_ratio,
                                   chain_kwargs=dict(chain_length=int(chain_length), burnin=int(burnin),
                                                     output_samples_frequency=int(output_samples_frequency), seed=seed, starting_value=starting_value,
                                                     fast_blocks=fast_blocks, independent_blocks=bool(independent_blocks),
                                                     heterogeneous_residuals=bool(heterogeneous_residuals), outputEBV=outputEBV,
                                                     output_heritability=bool(output_heritability), output_folder=output_folder,
                                                     printout_frequency=printout_frequency, missing_phenotypes=missing_phenotypes, block_size=block_size,
                                                     gram_mode=gram_mode, blocks_per_launch=blocks_per_launch, annotation_priors=annotation_priors,
                                                     printout_model_info=printout_model_info,
                                                     output_samples_for_all_parameters=output_samples_for_all_parameters))
    return run_chain(model, df, chain_length=int(chain_length), burnin=int(burnin),
                     output_samples_frequency=int(output_samples_frequency), seed=seed,
                     starting_value=starting_value, fast_blocks=fast_blocks,
                     independent_blocks=bool(independent_blocks), heterogeneous_residuals=bool(heterogeneous_residuals),
                     double_precision=bool(double_precision),
                     outputEBV=outputEBV, output_heritability=bool(output_heritability),
                     output_folder=output_folder, printout_frequency=printout_frequency,
                     memory_guard=memory_guard, memory_guard_ratio=memory_guard_ratio,
                     missing_phenotypes=missing_phenotypes, device=device, block_size=block_size,
                     gram_mode=gram_mode, blocks_per_launch=blocks_per_launch, location_parameters=location_parameters, annotation_priors=annotation_priors, causal_structure=causal_structure, engine=_engine, printout_model_info=printout_model_info,
                     output_samples_for_all_parameters=output_samples_for_all_parameters, gblup_eigen=gblup_eigen)
