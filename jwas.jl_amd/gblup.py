"""GBLUP on the device path (markers/BayesianAlphabet/GBLUP.jl; readgenotypes.jl:352-366,403-420; tools4genotypes.jl:409-418;
variance_components.jl:151-189): the marker sampler on pseudo-markers.

    get_genotypes(K, G, method="GBLUP")       K a relationship matrix (api.genomic_relationship_matrix forms it on the device)
    runMCMC                                   mcmc.run_chain with three GBLUP hooks: prepare() instead of the block set-up,
                                              step() instead of engine.sweep, draw_genetic_variance() as step 4

prepare() aligns K to the records, eigendecomposes it (K = L D L'), uploads L as the context's dense matrix and forms the output
matrix K[out, rows] L diag(1 / D): EBVs, PEV, genetic variance and heritability then come from the existing output layer
(mul_alpha / mul_alpha_output on the pseudo-marker effects).  The device step is csrc/gblup.hpp."""
import os
import subprocess
import sys
import tempfile

import numpy as np

GBLUP_METHODS = ("gblup_begin", "gblup_step", "gblup_rhs", "gblup_end")
EIGEN_AUTO_MIN_N = 8192      # gblup_eigen="auto": below this the host solves (n = 5 000, Float32: host 2.0 s, device 3.1 s with its process and transfers; NOTES.md)


def is_relationship_matrix(A):
    """issymmetric(genotypes) (readgenotypes.jl:354): square and exactly symmetric."""
    A = np.asarray(A)
    return A.ndim == 2 and A.shape[0] == A.shape[1] and A.shape[0] > 0 and np.array_equal(A, A.T)


def _isposdef(K):
    try:
        np.linalg.cholesky(K)           # (in the matrix's precision, as isposdef(::Matrix{Float32}))
        return True
    except np.linalg.LinAlgError:
        return False


def relationship_genotypes(Genotypes, Variance, obsID, K, G, *, G_is_marker_variance, df, estimate_variance, estimate_scale, constraint,
                           starting_value, Pi, estimatePi):
    """The Genotypes object of get_genotypes(K, G, method="GBLUP") (readgenotypes.jl:352-366,403-420)."""
    data_type = K.dtype.type
    print("A genomic relationship matrix is provided (instead of a genotype covariate matrix).")      # center = quality_control = false
    if G_is_marker_variance:
        raise ValueError("Genetic variance is required.")
    if not (starting_value is False or starting_value is None):
        raise ValueError("starting values are not supported for GBLUP now.")
    if not np.all(np.isfinite(K)):
        raise ValueError("the relationship matrix holds non-finite values")
    n = K.shape[0]
    count = 0
    while not _isposdef(K):                                                                   # :409-417
        print("The relationship matrix is not positive definite. A very small number is added to the diagonal.")
        K = np.asfortranarray(K + np.eye(n, dtype=data_type) * data_type(0.00001))
        count += 1
        if count > 10:
            raise ValueError("Please provide a positive-definite relationship matrix.")
    p = (K.mean(axis=0, dtype=data_type) / data_type(2.0)).astype(data_type)                  # :384-385 with center = false
    sum2pq = float((2.0 * p * (1.0 - p)).sum(dtype=data_type))
    g = Genotypes(obsID, [str(i + 1) for i in range(n)], n, n, p, sum2pq, False, K)
    g.isGRM = True
    g.G = Variance(False, df, False, estimate_variance, estimate_scale, constraint)
    g.genetic_variance = Variance(G, df, False, estimate_variance, estimate_scale, constraint)
    g.method, g.estimatePi, g.pi = "GBLUP", estimatePi, Pi
    print("Genotype informatin:")
    print(f"#markers: 0; #individuals: {n}")
    return g


def routes(model):
    return any(getattr(Mi, "method", None) == "GBLUP" for Mi in model.M)


def _set(x):
    return not (x is False or x is None or (np.isscalar(x) and x == 0))


def validate(model, df, *, single_step_analysis, fast_blocks, independent_blocks, heterogeneous_residuals, causal_structure, RRM, chains,
             engine, gblup_eigen, double_precision):
    """Everything a GBLUP run refuses, each naming its argument, before anything is written."""
    if gblup_eigen not in ("auto", "host", "device"):
        raise ValueError('gblup_eigen must be "auto", "host" or "device".')
    if _set(single_step_analysis):
        raise ValueError("SSGBLUP is not available (runMCMC(...; single_step_analysis=...) with method GBLUP)")      # input_data_validation.jl:41-43
    if len(model.M) > 1:
        raise NotImplementedError("GBLUP with several genotype categories stays on the reference")
    Mi = model.M[0]
    if Mi.genetic_variance.val is False and Mi.G.val is not False:                            # :38-40
        raise ValueError("Please provide values for the genetic variance for GBLUP analysis (G was given as a marker variance)")
    if getattr(Mi, "storage_mode", "dense") != "dense":
        raise NotImplementedError("GBLUP needs a relationship matrix on the host (device_genotypes and storage=:stream are not supported)")
    if not getattr(Mi, "isGRM", False):
        raise NotImplementedError("GBLUP needs get_genotypes(K, G, method=\"GBLUP\") with K from genomic_relationship_matrix(...)")
    if (np.asarray(Mi.genotypes).dtype == np.float64) != bool(double_precision):
        raise NotImplementedError("get_genotypes(K, ...; double_precision=...) and runMCMC(...; double_precision=...) must agree for GBLUP")
    for flag, name in ((independent_blocks, "independent_blocks"), (fast_blocks, "fast_blocks")):
        if _set(flag):
            raise NotImplementedError(f"runMCMC(...; {name}=...) with GBLUP: the pseudo-marker sampler has no blocks; stays on the reference")
    if _set(heterogeneous_residuals):
        raise NotImplementedError("runMCMC(...; heterogeneous_residuals=true) with GBLUP: the reference indexes the record weights by "
                                  "pseudo-marker (lhs = Rinv .+ ...), which is not a Gibbs step once L'WL is not diagonal; not built")
    if getattr(Mi, "annotations", False) is not False:
        raise NotImplementedError("annotations with GBLUP stay on the reference")
    tt = list(getattr(model, "traits_type", None) or [])
    if any(v != "continuous" for v in tt):
        raise NotImplementedError("categorical_trait / censored_trait with GBLUP stay on the reference")
    for flag, name in ((causal_structure, "causal_structure"), (RRM, "RRM")):
        if _set(flag):
            raise NotImplementedError(f"runMCMC(...; {name}=...) with GBLUP stays on the reference")
    if not (isinstance(chains, (int, np.integer)) and not isinstance(chains, bool) and int(chains) == 1):
        raise NotImplementedError("runMCMC(...; chains=K) with GBLUP stays on the reference")
    t = model.nModels
    if t > 4:
        raise NotImplementedError("GBLUP runs 1 to 4 traits on the device")
    for re_ in getattr(model, "rndTrmVec", []):
        if re_.randomType != "I":
            raise NotImplementedError(f"set_random({re_.name}) with a pedigree or a covariance structure and GBLUP stays on the reference")
    if t > 1:                                                                                 # complete records only
        ids = df[df.columns[0]].astype(str)
        have = ids.isin(set(Mi.obsID)).to_numpy()
        obs = np.stack([np.isfinite(df[tr].to_numpy(dtype=np.float64)) if tr in df.columns else np.zeros(len(df), dtype=bool)
                        for tr in model.lhsVec], axis=1)
        if (have & obs.any(axis=1) & ~obs.all(axis=1)).any():
            raise NotImplementedError("GBLUP with records that miss some traits (missing_phenotypes) stays on the reference")
    if engine is not None:
        if isinstance(engine, (list, tuple)):
            raise NotImplementedError("GBLUP takes one engine")
        missing = [m for m in GBLUP_METHODS if not hasattr(engine, m)]
        if missing:
            raise NotImplementedError("GBLUP needs an engine with the pseudo-marker step (" + ", ".join(missing)
                                      + " missing); the package has no CPU fallback")
        if hasattr(engine, "comm_info") and engine.comm_info()[1] > 1:
            raise NotImplementedError("GBLUP is not driven from marker or row shards")


# ---- the eigendecomposition ------------------------------------------------------------------------------------------------------------
# torch brings a HIP runtime of its own; the solver therefore runs in a child process (the engine's runtime holds the device here).
# It always solves in Float64 and rounds D and L once to the matrix's precision: the device's Float32 solver left L'L - I and
# L D L' - K about 30 times larger than LAPACK's ssyevd on the 301 x 301 test matrix (2.1e-5 against 6.2e-7), the Float64 solve
# rounded to Float32 does not (NOTES.md, "GBLUP").
_EIGH_CHILD = r"""
import sys
import numpy as np
import torch
src, dst, dev = sys.argv[1], sys.argv[2], int(sys.argv[3])
if not torch.cuda.is_available():
    sys.exit(3)
K = np.load(src)
free, _ = torch.cuda.mem_get_info(dev)
if 4 * 8 * K.size > 0.9 * free:
    sys.exit(4)
A = torch.from_numpy(K).to(torch.device("cuda", dev)).double()
D, L = torch.linalg.eigh(A)
np.save(dst + ".D.npy", D.cpu().numpy().astype(K.dtype))
np.save(dst + ".L.npy", L.cpu().numpy().astype(K.dtype))
"""


def eigh_host(K):
    D, L = np.linalg.eigh(K)
    return D, L


def eigh_device(K, device=0):
    """torch.linalg.eigh on the GPU in a child process.  Raises RuntimeError when it cannot run."""
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "K.npy"), os.path.join(tmp, "out")
        np.save(src, np.ascontiguousarray(K))
        r = subprocess.run([sys.executable, "-c", _EIGH_CHILD, src, dst, str(int(device))], capture_output=True, text=True)
        if r.returncode != 0:
            why = {3: "torch sees no GPU", 4: "the workspace does not fit the free device memory"}.get(r.returncode, (r.stderr or "").strip()[-400:])
            raise RuntimeError(f"gblup_eigen=\"device\": torch.linalg.eigh is not usable here ({why})")
        return np.load(dst + ".D.npy"), np.load(dst + ".L.npy")


def eigen(K, mode="auto", device=0):
    """(D, L, where) with K = L diag(D) L' in K's precision."""
    if mode == "host" or (mode == "auto" and K.shape[0] < EIGEN_AUTO_MIN_N):
        return eigh_host(K) + ("host",)
    try:
        return eigh_device(K, device) + ("device",)
    except RuntimeError:
        if mode == "device":
            raise
        return eigh_host(K) + ("host",)


class Prepared:
    """What run_chain needs of GBLUP_setup (GBLUP.jl:9-31): L (n x n, the element type of the run), D (float64, abs), the output
    matrix (None: EBVs for exactly the training records, X = L itself) and where the eigendecomposition ran."""

    def __init__(self, L, D, Xout, where):
        self.L, self.D, self.Xout, self.where = L, D, Xout, where


def prepare(Mi, rows, out_rows, ftype, *, gblup_eigen="auto", device=0):
    """rows: the rows of K behind the records, in record order (tools4genotypes.jl:288-323); out_rows: the rows EBVs are reported
    for (None: the records themselves)."""
    rows = np.asarray(rows, dtype=np.int64)
    if len(np.unique(rows)) != len(rows):
        raise ValueError("GBLUP: an individual has more than one record; its rows of the relationship matrix are equal and the matrix "
                         "of the records is singular (repeated records stay on the reference)")
    Kall = np.asarray(Mi.genotypes)
    if Kall.dtype != ftype:
        raise NotImplementedError("the relationship matrix and runMCMC must agree on double_precision")
    K = np.ascontiguousarray(Kall[np.ix_(rows, rows)])
    D, L, where = eigen(K, gblup_eigen, device)
    D = np.abs(np.asarray(D, dtype=np.float64))                                               # GBLUP.jl:30: avoid very small negative values
    if not np.all(np.isfinite(D) & (D > 0)):
        raise ValueError("GBLUP: the relationship matrix of the records has a zero or non-finite eigenvalue")
    L = np.asfortranarray(L, dtype=ftype)
    n = len(rows)
    Mi.nMarkers, Mi.markerID = n, [str(i + 1) for i in range(n)]                              # pseudo markers of length nObs (:25-26)
    Xout = None
    if out_rows is not None:                                                                  # Mi.output_genotypes = M2Mt L diag(1 / D) (:23)
        K2 = np.asarray(Kall[np.ix_(np.asarray(out_rows, dtype=np.int64), rows)], dtype=np.float64)
        Xout = np.asfortranarray((K2 @ L.astype(np.float64)) / D[None, :], dtype=ftype)
    return Prepared(L, D, Xout, where)


# ---- the chain's hooks -----------------------------------------------------------------------------------------------------------------
def step(engine, *, iteration, seed, vare, G, t, diagonal):
    """Step 2 of the chain: engine.gblup_step in the shape run_chain reads a sweep's result."""
    st = engine.gblup_step(iteration=iteration, seed=seed, vare=np.asarray(vare, dtype=np.float64).reshape(t, t),
                           G=np.asarray(G, dtype=np.float64).reshape(t, t), diagonal=diagonal)
    st["sweep_ms"] = st["step_ms"]
    return st


def draw_genetic_variance(rng, alpha_ss, n, df, scale, t, constraint, ftype):
    """sample_marker_effect_variance with invweights = 1 ./ D (variance_components.jl:151-189): alpha_ss = sum_i alpha_i alpha_i' / D_i."""
    if t == 1:
        return ftype((float(np.asarray(alpha_ss).reshape(-1)[0]) + df * float(scale)) / rng.chisquare(n + df))
    S = np.asarray(alpha_ss, dtype=np.float64).reshape(t, t)
    scale = np.asarray(scale, dtype=np.float64)
    if constraint:
        return np.diag([(S[k, k] + df * scale[k, k]) / rng.chisquare(n + df) for k in range(t)]).astype(ftype)
    from scipy.stats import invwishart
    W = scale + S
    return np.asarray(invwishart.rvs(df=df + n, scale=(W + W.T) / 2, random_state=rng), dtype=ftype).reshape(t, t)


def rename_variance_file(output_folder, name):
    """MCMC_BayesianAlphabet.jl:434-439."""
    src = os.path.join(output_folder, f"MCMC_samples_marker_effects_variances_{name}.txt")
    if os.path.exists(src):
        os.replace(src, os.path.join(output_folder, f"MCMC_samples_genetic_variance(REML)_{name}.txt"))
