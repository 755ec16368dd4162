"""Host side of one MCMC chain: everything of MCMC_BayesianAlphabet (MCMC/MCMC_BayesianAlphabet.jl:4-447)
that is NOT the marker sweep, driving a sweep engine (jwas.jl_amd.engine.HipEngine) for step 2.

Per iteration (the reference's order, MCMC_BayesianAlphabet.jl:184-421):
  0. categorical / censored traits: engine.liability_sample(...), then the threshold draw                (:186-191, DEVICE)
  1. location parameters: ycorr += X sol ; rhs = X'ycorr ; single-site Gibbs ; ycorr -= X sol   (:196-220, host, or DEVICE:
     engine.locpar_step(...), term by term from the resident residual -- location_parameters="device" / "auto")
     multi-trait records that miss some traits: the host imputes their residuals first (residual.jl:51-73), or on the DEVICE
     path engine.mtmiss_impute(...) does and locpar_step weights record by record until the first residual-variance draw
  4c. variances of the set_random effects from the device's U'U (sampleVCs, :347-351)            (host)
  2. marker effects: engine.sweep(...)                                                      (:224-290, DEVICE)
  3. pi  ~ Beta / Dirichlet from the sweep's counts                                          (:294-317, host)
  4. marker effect variance from alpha'alpha / ssq / beta'beta                               (:321-326, host)
  5. residual variance from r'r                                                              (:363-370, host)
  5b. causal_structure: the structural coefficients among the traits, engine.sem_step(...)   (:372-377, DEVICE)
  6. every output_samples_frequency after burn-in: running means (device for markers)       (:399-413)
The host consumes only O(n) + O(p)-reducible quantities from the device.
"""
import contextlib
import os
import time

import numpy as np

from .chain_output import (GeneticVarianceSamples, Running, SampleFiles, covariance_table, ebv_tables, host_blas_limit, location_table,
                           marker_effects_table, pi_labels, pi_table, print_posterior_means, resolve_output_ids, sparse_effects,
                           term_sample_columns, write_id_files, write_tables)

BAYESR_GAMMA = np.array([0.0, 0.01, 0.1, 1.0])
DEVICE_BLOCK_SIZES = (64, 128, 256, 512, 1024)


def _supported_block(b):
    return min(DEVICE_BLOCK_SIZES, key=lambda s: abs(s - b))


def _design(model, df, ids_col):
    """Fixed-effect incidence matrices per trait (build_MME.jl:183-290, dense): intercept = ones,
    covariate = the column, factor = one 0/1 column per level."""
    cols, labels = [], []
    for tl in model.modelTerms:
        Xk, lab = [], []
        for term in tl:
            if term.kind == "intercept":
                Xk.append(np.ones((len(df), 1)))
                lab.append((term.trait, "intercept", "intercept"))
            elif term.kind == "covariate":
                Xk.append(df[term.name].to_numpy(dtype=np.float64)[:, None])
                lab.append((term.trait, term.name, term.name))
            else:
                if term.name not in df.columns:
                    raise ValueError(f"{term.name} is not found in the phenotype data (genotype terms must be "
                                     "Genotypes objects visible to build_model).")
                lev = df[term.name].astype(str)
                for lv in sorted(lev.unique()):
                    Xk.append((lev == lv).to_numpy(dtype=np.float64)[:, None])
                    lab.append((term.trait, term.name, lv))
        cols.append(np.hstack(Xk) if Xk else np.zeros((len(df), 0)))
        labels.append(lab)
    return cols, labels


LOCPAR_METHODS = ("locpar_begin", "locpar_add_covariate", "locpar_add_factor", "locpar_step", "locpar_get_sol", "locpar_accumulate",
                  "locpar_get_means", "locpar_end")
LOCPAR_PED_METHODS = ("locpar_set_group_structure",)      # ... and what a pedigree random effect needs on top
MTMISS_METHODS = ("mtmiss_begin", "mtmiss_impute", "mtmiss_set_record_weights", "mtmiss_end")      # ... and partially missing multi-trait records
SEM_METHODS = ("sem_begin", "sem_step", "sem_accumulate", "sem_get_effects", "sem_end")      # ... and a causal structure among the traits
ANNOT_METHODS = ("annot_begin", "annot_step", "annot_accumulate", "annot_prior", "annot_means", "annot_end")
LOCPAR_AUTO_LEVELS = 2048               # location_parameters="auto": more levels than this run on the device


def _location_terms(model, df):
    """The terms of _design without the dense matrices: per trait a list of (name, kind, values) -- kind "covariate": the column
    (None: the intercept), kind "factor": (codes, nlevels) with the levels numbered in _design's order -- and _design's labels."""
    terms, labels = [], []
    for tl in model.modelTerms:
        tk, lab = [], []
        for term in tl:
            if term.kind == "intercept":
                tk.append((term.name, "covariate", None))
                lab.append((term.trait, "intercept", "intercept"))
            elif term.kind == "covariate":
                tk.append((term.name, "covariate", df[term.name].to_numpy(dtype=np.float64)))
                lab.append((term.trait, term.name, term.name))
            else:
                if term.name not in df.columns:
                    raise ValueError(f"{term.name} is not found in the phenotype data (genotype terms must be "
                                     "Genotypes objects visible to build_model).")
                lev = df[term.name].astype(str)
                ped_ = next((re_ for re_ in getattr(model, "rndTrmVec", []) if re_.randomType in ("A", "V") and re_.name == term.name), None)
                if ped_ is not None:                          # the levels of a polygenic effect: the pedigree's IDs, in its order
                    names = list(ped_.names)
                    lev = lev.str.strip()
                    unknown = sorted(set(lev) - set(names) - ({"missing"} if ped_.randomType == "V" else set()))      # (a Vinv effect: "missing" = in no level, SSBR.jl:28-31)
                    if unknown:
                        raise ValueError(f"{term.name}: {unknown[:5]} {'...' if len(unknown) > 5 else ''} not found in the pedigree.")
                else:
                    names = sorted(lev.unique())
                index = {lv: i for i, lv in enumerate(names)}
                tk.append((term.name, "factor", (lev.map(index).fillna(-1).to_numpy(dtype=np.int32), len(names))))
                lab.extend((term.trait, term.name, lv) for lv in names)
        terms.append(tk)
        labels.append(lab)
    return terms, labels


def genetic2marker(Mi, pi, method, t=1):
    """Marker-effect (co)variance implied by the genetic variance and pi (tools4genotypes.jl:426-478)."""
    p = Mi.nMarkers
    Vg = np.asarray(Mi.genetic_variance.val, dtype=np.float64)
    if t > 1:                                                          # :426-438 (Dict Pi)
        pi_arr = np.asarray(pi, dtype=np.float64)
        denom = np.zeros((t, t))
        for i in range(t):
            for j in range(t):
                sel = [s for s in range(1 << t) if (s >> i) & 1 and (s >> j) & 1]
                denom[i, j] = Mi.sum2pq * pi_arr[sel].sum()
        return Vg / denom
    if method == "BayesR":                                             # :461-467
        pv = np.asarray(pi, dtype=np.float64)
        if pv.shape != (4,):
            raise ValueError("BayesR Pi must have length 4.")
        denom = Mi.sum2pq * float((BAYESR_GAMMA * pv).sum())
        if not denom > 0:
            raise ValueError("BayesR implied variance denominator must be positive.")
        return float(Vg) / denom
    if np.ndim(pi) == 1:                                               # :468-475
        if len(pi) != p:
            raise ValueError(f"BayesC marker-level Pi must have length {p}.")
        af = np.asarray(Mi.alleleFreq, dtype=np.float64)
        denom = float((2 * af * (1 - af) * (1 - np.clip(np.asarray(pi, dtype=np.float64), 0, 1))).sum())
        if not denom > 0:
            raise ValueError("BayesC implied variance denominator must be positive.")
        return float(Vg) / denom
    return float(Vg) / ((1 - float(pi)) * Mi.sum2pq)                   # :457-459


ADAPTIVE_CHANGE_FRACTION = float(os.environ.get("JWAS_ADAPTIVE_FRACTION", "0.0125"))      # measured crossover of block 512 vs 1024


ADAPTIVE_CHANGE_FRACTION_PAIRS = float(os.environ.get("JWAS_ADAPTIVE_FRACTION_PAIRS", "0.009"))    # ... when the 512-marker sweeps run as ping-pong pairs


def pick_block_size(n_events, p, small=512, large=1024, pairs=False):
    """Block size of the next sweep from the number of markers whose effect changed in the last one.  pairs: the small size runs as
    ping-pong pairs (pingpong_pairs_for_chain), which moves the crossover down (config 3's chain: 24 ms per sweep on 512-marker pairs at
    8 700 changes per sweep, 26.5 ms on 4 x 1024-marker launches at 7 500, 22.6 ms at 4 700)."""
    return large if n_events < (ADAPTIVE_CHANGE_FRACTION_PAIRS if pairs else ADAPTIVE_CHANGE_FRACTION) * p else small


# Grouped launches (jwas_hip_setup_groups / jwas_sweep_params.group_launch): blocks per launch of the step kernel on the LARGE block
# size of a single-trait chain -- the size the adaptive policy selects once few markers change per sweep, where a launch's fixed
# cost (~3.5 us of a 32 us launch at 50 000 x 1024) is what separates the sweep from the copy rate.  0 = off.
GROUPED_BLOCKS_PER_LAUNCH = 4


def grouped_blocks_for_chain(chain_length):
    """Blocks per grouped launch a chain of this length pays for: the group cross-Grams are set-up work (at 50 000 x 600 000:
    +1.7 s for 2 blocks per launch, +5 s for 4) against 0.6 / 0.9 ms saved per sweep of the sparse steady state."""
    # (measured break-even, round 6: 4 blocks per launch + 4.1 s of set-up / 1.07 ms per sweep = 3 800 sweeps; 2 blocks: + 1.4 s / 0.6 ms
    # = 2 300 -- the thresholds leave a margin of 1.3x, they were 8 000 / 3 000)
    return GROUPED_BLOCKS_PER_LAUNCH if chain_length >= 5000 else (2 if chain_length >= 3000 else 0)


def pingpong_pairs_for_chain(method, estimate_pi, chain_length):
    """Pairs of 512-marker blocks per launch (ping-pong samplers: csrc/sweep.hpp k_group_step, SamplerArgs::pp_role) for the
    HIGH-TURNOVER sweeps of a single-trait chain -- the ones the adaptive policy runs on 512-marker blocks because the sampler is the
    critical path: BayesR sheds its markers over hundreds of sweeps, a fixed pi keeps ~(1 - pi) p markers in the model for ever
    (config 3: 29.5 -> 26.8 ms per sweep, fixed pi = 0.95: 29.4 -> 27.0).  BayesC with pi estimated leaves that regime after ~25
    sweeps: not worth the pair cross-Grams (4 p 1024 bytes, 0.7 s at 50 000 x 600 000)."""
    # (4 blocks per launch, one sampler workgroup per block: config 3 25.2 ms, fixed pi 26.1 ms per sweep against 26.6 / 27.0 with pairs,
    # for + 2.5 GB and + 1.1 s of cross-Grams: pays from ~800 high-turnover sweeps on -- a fixed pi stays in the regime for ever, config 3's
    # BayesR chain runs its first ~1 300 sweeps on 512-marker blocks)
    if chain_length >= 2000 and (method == "BayesR" or not estimate_pi):
        return 4
    return 2 if (chain_length >= 300 and (method == "BayesR" or not estimate_pi)) else 0


def grouped_launch_size(method, ntraits, row_shards, block_size, groups=GROUPED_BLOCKS_PER_LAUNCH, dense_prior=False):
    """Block size on which grouped launches are set up (0: none): single-trait BayesA/B/C/R chains with a sparse prior on uniform
    blocks of one GPU's markers (marker shards included, row shards not), groups * block_size <= 4096."""
    if groups not in (2, 4) or ntraits != 1 or row_shards or dense_prior or method not in ("BayesC", "BayesB", "BayesA", "BayesR"):
        return 0
    if block_size < 512 or groups * block_size > 4096:
        return 0
    return int(block_size)


MT_SPARSE_CHANGE_FRACTION = float(os.environ.get("JWAS_MT_SPARSE_FRACTION", "0.1"))          # the share of markers changing per sweep below which a dense-start multi-trait chain is sparse


MT_1024_CHANGE_FRACTION = float(os.environ.get("JWAS_MT_1024_FRACTION", "0.005"))          # ... below which it runs 1024-marker blocks (skip and verify)


def mt_1024_allowed(t, p, per_marker_cov=False):
    """1024-marker multi-trait blocks: the block's draws and constants must fit LDS (block x traits <= 3072: up to three traits,
    no covariance per marker) and there must be a few of them."""
    return bool(1024 * t <= 3072 and not per_marker_cov and p > 4 * 1024)


def pick_block_size_mt(n_events, p, allow_1024=False):
    """Multi-trait sampler I that STARTS dense (the reference's default prior, every marker in the model): 256-marker blocks
    (dense_big_mt / Rule T) while most markers change every sweep; with Pi estimated such a chain moves on to a sparse steady
    state, where the speculative rounds want 512-marker blocks (3.98 vs 5.12 ms per sweep at 20k x 100k x 3)
    and, once a block holds only a handful of candidates (< 0.5 % of the markers change per sweep: most 64-marker sub-blocks are left
    to the helper waves, sampler_role_mt's skip and verify), 1024-marker blocks: half the launches and fronts (3.35 vs 3.83 ms)."""
    if allow_1024 and n_events < MT_1024_CHANGE_FRACTION * p:
        return 1024
    return 512 if n_events < MT_SPARSE_CHANGE_FRACTION * p else 256


def _missing_pattern_matrices(R0, code):
    """The matrices of one missing pattern (bit k of `code` set = trait k observed) under the residual covariance R0:
    o / m: the observed / missing traits (boolean masks); Ro_inv = inv(R0[o, o]); Rc = R0[m, o];
    C: Ro_inv embedded in a t x t matrix of zeros (the RZ of getRi, residual.jl:2-44);
    B = Rc Ro_inv (|m| x |o|) and U = the upper Cholesky factor of R0[m, m] - Rc Ro_inv Rc' (residual.jl:63-69); both None for the
    full pattern.  The one place these are formed: the host path, the device tables and the tests read the same doubles."""
    t = R0.shape[0]
    o = np.array([(code >> k) & 1 for k in range(t)], dtype=bool)
    Ro_inv = np.linalg.inv(R0[np.ix_(o, o)])
    RZ = np.zeros((t, t))
    RZ[np.ix_(o, o)] = Ro_inv
    out = {"o": o, "m": ~o, "Ro_inv": Ro_inv, "C": RZ, "Rc": None, "B": None, "U": None}
    if not o.all():
        m = ~o
        Rc = R0[np.ix_(m, o)]
        out["Rc"] = Rc
        out["U"] = np.linalg.cholesky(R0[np.ix_(m, m)] - Rc @ Ro_inv @ Rc.T).T          # upper factor, as cholesky(...).U
        out["B"] = (Ro_inv @ Rc.T).T
    return out


def missing_pattern_tables(R0):
    """(B, U, C): the per-code tables of csrc/mtmiss.hpp for the residual covariance R0, each [2^t][t][t] (code 0 and the unused
    entries zero; B and U in the top-left corner of their slot)."""
    R0 = np.asarray(R0, dtype=np.float64)
    t = R0.shape[0]
    B, U, Ct = (np.zeros((1 << t, t, t)) for _ in range(3))
    for code in range(1, 1 << t):
        pm = _missing_pattern_matrices(R0, code)
        Ct[code] = pm["C"]
        if pm["B"] is not None:
            nm, no = pm["B"].shape
            B[code, :nm, :no] = pm["B"]
            U[code, :nm, :nm] = pm["U"]
    return B, U, Ct


def _impute_missing_residuals(res, observed, R0, rng):
    """sampleMissingResiduals (residual.jl:52-73), in place on the per-trait residual vectors `res`: for every missing
    pattern the missing residuals are drawn from their conditional distribution given the observed ones,
    e_m | e_o ~ N(Rc Ro^-1 e_o, Rmm - Rc Ro^-1 Rc').  Returns the per-record inverse residual covariance of mkRi/getRi
    (residual.jl:2-44): inv(R0[o, o]) embedded in a t x t matrix of zeros."""
    n, t = observed.shape
    Ri_rows = np.empty((n, t, t))
    codes = observed @ (1 << np.arange(t))
    full = (1 << t) - 1
    for code in np.unique(codes):
        rows = np.nonzero(codes == code)[0]
        pm = _missing_pattern_matrices(R0, int(code))
        o, m, Ro_inv, Rc, U = pm["o"], pm["m"], pm["Ro_inv"], pm["Rc"], pm["U"]
        Ri_rows[rows] = pm["C"]
        if code == full:
            continue
        eo = np.stack([res[k][rows] for k in np.nonzero(o)[0]], axis=1)          # rows x n_obs
        em = eo @ Ro_inv @ Rc.T + rng.standard_normal((len(rows), int(m.sum()))) @ U
        for c, k in enumerate(np.nonzero(m)[0]):
            res[k][rows] = em[:, c]
    return Ri_rows


def _inverse_wishart_batch(rng, df, scale):
    """One InverseWishart(df, scale_j) draw per matrix of the batch (m x t x t), Bartlett's decomposition: with
    scale_j = C C' (Cholesky) and A lower-triangular (A_ii = sqrt(chi2(df - i)), A_ik ~ N(0,1) below the diagonal),
    W = C'^-1 A A' C^-1 ~ Wishart(df, scale_j^-1) and G = W^-1 = K K' with K' = A^-1 C' (one batched Cholesky and a forward
    substitution vectorised over the batch; the reference draws each marker's matrix with rand(InverseWishart(df, scale)),
    variance_components.jl:181-186)."""
    m, t, _ = scale.shape
    C = np.linalg.cholesky(scale)
    A = np.zeros((m, t, t))
    for i in range(t):
        A[:, i, i] = np.sqrt(rng.chisquare(df - i, size=m))
        for k in range(i):
            A[:, i, k] = rng.standard_normal(m)
    Kt = np.empty((m, t, t))
    Ct = C.transpose(0, 2, 1)
    for i in range(t):
        acc = Ct[:, i, :].copy()
        for k in range(i):
            acc -= A[:, i, k, None] * Kt[:, k, :]
        Kt[:, i, :] = acc / A[:, i, i, None]
    G = Kt.transpose(0, 2, 1) @ Kt
    return (G + G.transpose(0, 2, 1)) / 2


def indirect_matrix(lam):
    """K = sum_{m=1}^{t-1} Lambda^m (compute_indirect_effect, SEM.jl:245-252): row k holds what every trait's direct marker effects
    contribute to trait k through the causal paths."""
    lam = np.asarray(lam, dtype=np.float64)
    K, P = np.zeros_like(lam), np.eye(lam.shape[0])
    for _ in range(lam.shape[0] - 1):
        P = P @ lam
        K = K + P
    return K


def indirect_overall_rows(K, direct):
    """One saved sample's indirect and overall marker effects from the sparse direct ones: direct = [(idx, val)] per trait.
    Returns (the union of the indices ascending, indirect [t][nnz], overall [t][nnz]) in double, with the device's order of
    operations: indirect_k = sum_j K[k, j] alpha_j (j ascending from 0), overall_k = alpha_k + indirect_k."""
    t = len(direct)
    u = np.unique(np.concatenate([np.asarray(si, dtype=np.int64) for si, _ in direct])) if t else np.zeros(0, dtype=np.int64)
    A = np.zeros((t, u.size))
    for k, (si, sv) in enumerate(direct):
        A[k, np.searchsorted(u, si)] = np.asarray(sv, dtype=np.float64)
    ind = np.zeros((t, u.size))
    for k in range(t):
        for j in range(t):
            ind[k] = ind[k] + K[k, j] * A[j]
    return u.astype(np.int32), ind, A + ind


LIABILITY_TYPES = ("categorical", "categorical(binary)", "censored")
LIABILITY_METHODS = ("liability_begin", "set_categorical", "set_censored", "set_thresholds", "liability_init", "liability_sample",
                     "liability_minmax", "liabilities", "liability_end")


def add_censored_trait_column(model, ph, rng):
    """add_censored_trait_column! (categorical_and_censored_trait.jl:263-296; JWAS.jl:229-235): the column <trait> from the bounds
    <trait>_l / <trait>_u -- missing when the record is not truncated at all, the finite bound of a one-sided record, a value
    l, l + 1, ... <= u of a two-sided one (rand(l:u)); missing bounds become -Inf / +Inf."""
    for k, tr in enumerate(model.lhsVec):
        if model.traits_type[k] != "censored":
            continue
        for c in (f"{tr}_l", f"{tr}_u"):
            if c not in ph.columns:
                raise ValueError(f"censored trait {tr}: the phenotype data need the columns {tr}_l and {tr}_u.")
        lo = ph[f"{tr}_l"].to_numpy(dtype=np.float64).copy()
        up = ph[f"{tr}_u"].to_numpy(dtype=np.float64).copy()
        both = np.isnan(lo) & np.isnan(up)
        lo[both], up[both] = -np.inf, np.inf
        if np.isnan(lo).any() or np.isnan(up).any() or (lo > up).any():
            raise ValueError(f"censored trait {tr}: every record needs lower bound <= upper bound (both missing = not observed).")
        y = np.full(len(ph), np.nan)
        one_l, one_u = np.isinf(lo) & ~np.isinf(up), ~np.isinf(lo) & np.isinf(up)
        y[one_l], y[one_u] = up[one_l], lo[one_u]
        two = ~np.isinf(lo) & ~np.isinf(up)
        y[two] = lo[two] + np.floor(rng.random(int(two.sum())) * (np.floor(up[two] - lo[two]) + 1.0))
        ph[tr], ph[f"{tr}_l"], ph[f"{tr}_u"] = y, lo, up


def sample_from_conditional_inverse_wishart(rng, df, scale, binary_index):
    """sample_from_conditional_inverse_Wishart (categorical_and_censored_trait.jl:228-260; Korsgaard et al. 1999): a draw of R in
    which the binary traits are independent with unit variance.  `scale` is the Wishart scale inv(scale_R + SSE)."""
    from scipy.stats import wishart
    t = scale.shape[0]
    i2 = list(binary_index)
    i1 = [k for k in range(t) if k not in i2]
    n1, n2 = len(i1), len(i2)
    if n1 == 0:
        return np.eye(t)
    V11, V12, V22 = scale[np.ix_(i1, i1)], scale[np.ix_(i1, i2)], scale[np.ix_(i2, i2)]
    V11i = np.linalg.inv(V11)
    V22_1 = V22 - V12.T @ V11i @ V12
    X1 = np.atleast_2d(wishart.rvs(df=df, scale=(V11 + V11.T) / 2, random_state=rng))
    X1i = np.linalg.inv(X1)
    mu = (V11i @ V12).ravel(order="F")
    Sig = np.kron(V22_1, X1i)
    X2 = rng.multivariate_normal(mu, (Sig + Sig.T) / 2).reshape((n1, n2), order="F")
    X1i = (X1i + X1i.T) / 2                    # (inv() is symmetric up to rounding only; the device asks for an exactly symmetric R)
    R = np.block([[X1i + X2 @ X2.T, -X2], [-X2.T, np.eye(n2)]])
    order = np.argsort(i1 + i2)
    R = R[np.ix_(order, order)]
    return (R + R.T) / 2


@contextlib.contextmanager
def _on_error(*calls):
    """An exception inside the block: `calls` run, then it propagates."""
    try:
        yield
    except BaseException:
        for call in calls:
            call()
        raise


def _gibbs(A, x, b, rng, vare=None):
    """One sweep of the single-site Gibbs sampler on the MME (iterative_solver/solver.jl:143-162)."""
    for i in range(len(x)):
        if A[i, i] != 0.0:
            invlhs = 1.0 / A[i, i]
            mu = invlhs * (b[i] - A[:, i] @ x) + x[i]
            x[i] = rng.standard_normal() * np.sqrt(invlhs * (vare if vare is not None else 1.0)) + mu


def host_location_step(engine, Xf0, lhs, sol, w64, rng, vare, ftype):
    """Step 1 of a single-trait iteration on the host (MCMC_BayesianAlphabet.jl:196-220): the residual comes to the host, the dense
    design matrix Xf0 adds X sol, one scan of _gibbs on (lhs, X'R^-1 ycorr), and the residual goes back."""
    r = engine.get_residual(0).astype(np.float64)
    r += Xf0 @ sol
    rhs = Xf0.T @ (w64 * r)                                             # MCMC_BayesianAlphabet.jl:211
    _gibbs(lhs, sol, rhs, rng, float(vare))
    r -= Xf0 @ sol
    engine.set_residual(r.astype(ftype), 0)


def run_chain(model, df, *, chain_length, burnin, output_samples_frequency, seed, starting_value,
              fast_blocks, independent_blocks=False, heterogeneous_residuals=False, outputEBV, output_heritability=True, output_folder, printout_frequency, memory_guard, memory_guard_ratio,
              missing_phenotypes, device, block_size, gram_mode, engine, printout_model_info,
              output_samples_for_all_parameters, double_precision=False, blocks_per_launch=None, location_parameters="auto",
              annotation_priors="host", causal_structure=False, single_step=None, gblup_eigen="auto"):
    """single_step: ssbr.SingleStep (None: not a single-step analysis) -- the imputed matrices are resident on the engine, the output IDs
    and the J / ϵ parts of the EBVs come from it (ssbr.py)."""
    Mi = model.M[0]
    t = model.nModels
    sem = causal_structure is not False                                 # the recursive structural equation model (SEM.jl)
    method = Mi.method
    # runMCMC(double_precision=true) (JWAS.jl:349-366): genotypes, G, alpha -> Float64; everything the chain holds follows.
    # ftype is the element type of the run (the reference's Float32 default, or Float64).
    ftype = np.float64 if double_precision else np.float32
    if not double_precision and getattr(Mi, "genotypes", None) is not None and getattr(Mi.genotypes, "dtype", None) == np.float64:
        raise NotImplementedError("Float64 genotypes (get_genotypes(double_precision=true)) run with runMCMC(double_precision=true); "
                                  "the mixed Float64 / Float32 chain stays on the reference")
    gblup = method == "GBLUP"                                           # the sampler on pseudo-markers (GBLUP.jl; gblup.py, csrc/gblup.hpp)
    if gblup:
        from . import gblup as _gb
    if t > 1 and method not in ("BayesC", "RR-BLUP", "BayesB", "BayesA", "GBLUP"):
        raise NotImplementedError("multi-trait device path implements BayesC (Gibbs samplers I, II and the constraint=true "
                                  "megaBayesABC! path) and BayesA/B (the same three); other methods stay on the reference")
    mega = t > 1 and bool(Mi.G.constraint)                              # megaBayesABC! (MCMC_BayesianAlphabet.jl:233-234)
    # Methods the reference never runs block-wise: megaBayesABC! / megaBayesC0! (constraint = true), BayesC0! / MTBayesC0!
    # (RR-BLUP) and BayesL! are ONE plain pass over the markers per outer iteration whatever fast_blocks says -- although
    # chain_length has already been divided by the block size (MCMC_BayesianAlphabet.jl:233-262, JWAS.jl:308-316).
    plain_pass = mega or method in ("RR-BLUP", "BayesL")
    if t == 1 and (Mi.G.constraint or model.R.constraint):
        raise ValueError("constraint==true is for multi-trait only")     # input_data_validation.jl:534-535,550-551
    if not isinstance(starting_value, bool) or starting_value:
        raise NotImplementedError("starting values for location parameters stay on the reference; marker starting "
                                  "values go through get_genotypes(starting_value=...)")
    seed_int = 0 if seed is False else int(seed)
    rng = np.random.default_rng(seed_int)                                # host-side draws (JWAS.jl:239-241)

    # ---- align phenotypes and genotypes (input_data_validation.jl:198-294, tools4genotypes.jl:288-323)
    idcol = df.columns[0]
    ph = df.copy()
    ph[idcol] = ph[idcol].astype(str)
    ped = getattr(model, "ped", False)
    if ped is not False:                                                 # input_data_validation.jl:213-218,235-243
        if not set(Mi.obsID) <= set(ped.ids):
            raise ValueError("Not all genotyped individuals are found in pedigree!")
        ph[idcol] = ph[idcol].str.strip()
        inped = ph[idcol].isin(set(ped.ids)).to_numpy()
        if not inped.all():
            ph = ph.loc[inped].reset_index(drop=True)
            print(f"In this incomplete genomic data (single-step) or PBLUP analysis, {int((~inped).sum())} phenotyped individuals are not "
                  "included in the pedigree. These are removed from the analysis.")
    traits_type = model.traits_type = list(getattr(model, "traits_type", None) or ["continuous"] * t)
    has_liab = any(tt in LIABILITY_TYPES for tt in traits_type)
    if sem:
        if has_liab:
            raise NotImplementedError("causal_structure with categorical / censored traits stays on the reference")
        if heterogeneous_residuals:
            raise NotImplementedError("causal_structure with heterogeneous_residuals stays on the reference")
        if Mi.alpha is not False:
            raise NotImplementedError("causal_structure with marker starting values stays on the reference")
        eng_ = engine if engine is not None else (Mi.device_backend if getattr(Mi, "storage_mode", "dense") == "device" else None)
        missing_ = [m_ for m_ in SEM_METHODS if eng_ is not None and not hasattr(eng_, m_)]
        if missing_:
            raise NotImplementedError("causal_structure needs an engine with the structural-coefficient step (" + ", ".join(missing_)
                                      + " missing); the package has no CPU fallback")
        if eng_ is not None and hasattr(eng_, "comm_info") and eng_.comm_info()[1] > 1:
            raise NotImplementedError("causal_structure is not driven from marker shards")
    if has_liab:
        if heterogeneous_residuals:
            raise NotImplementedError("heterogeneous_residuals with categorical / censored traits stays on the reference")
        if engine is not None or getattr(Mi, "storage_mode", "dense") == "device":
            eng_ = engine if engine is not None else Mi.device_backend
            missing_ = [m_ for m_ in LIABILITY_METHODS if not hasattr(eng_, m_)]
            if missing_:
                raise TypeError("categorical / censored traits need an engine with the liability step (" + ", ".join(missing_)
                                + " missing); the package has no CPU fallback")
        add_censored_trait_column(model, ph, rng)                        # JWAS.jl:229-235
    for tr in model.lhsVec:
        if tr not in ph.columns:
            raise ValueError(f"Phenotypes for {tr} are not found in the data.")
    complete = np.ones(len(ph), dtype=bool)
    for tr in model.lhsVec:
        complete &= np.isfinite(ph[tr].to_numpy(dtype=np.float64))
    if t > 1:
        # individuals whose phenotypes are missing for ALL traits are removed (input_data_validation.jl:396-404);
        # partially missing records need the reference's residual imputation (residual.jl:15-73)
        anyobs = np.zeros(len(ph), dtype=bool)
        for tr in model.lhsVec:
            anyobs |= np.isfinite(ph[tr].to_numpy(dtype=np.float64))
        if (anyobs & ~complete).any() and not missing_phenotypes:
            raise ValueError("phenotypes are missing for some traits of some individuals; missing_phenotypes=false does not allow that")
        usable = anyobs                          # partially observed records stay; their residuals are imputed every iteration
    else:
        usable = complete
    stream = getattr(Mi, "storage_mode", "dense") == "stream"
    devres = getattr(Mi, "storage_mode", "dense") == "device"          # matrix already resident on the GPU (api.device_genotypes)
    if devres:
        if not complete.all() or list(ph[idcol]) != list(Mi.obsID):
            raise ValueError("device-resident genotypes require exact genotype/phenotype ID match and order "
                             "(as storage=:stream does, JWAS.jl:388-398).")
        if engine is not None and engine is not Mi.device_backend:
            raise ValueError("the genotypes are resident on a different engine")
        engine = Mi.device_backend
        X = None
        n, p = Mi.nObs, Mi.nMarkers
    elif stream:
        # the packed payload goes from the file straight to HBM and is never re-ordered: like the reference's stream
        # mode, phenotype IDs must match the genotype IDs exactly and in order (JWAS.jl:388-398)
        # (a multi-trait record that misses SOME traits stays, with its missing residuals imputed every iteration: no row is dropped)
        if not usable.all() or list(ph[idcol]) != list(Mi.obsID):
            raise ValueError("storage=:stream MVP requires exact genotype/phenotype ID match and order. "
                             "Please reorder phenotypes to match genotype IDs.")
        print("storage=:stream is enabled; genotype alignment is skipped and original ID order is used.")
        X = None
        n, p = Mi.nObs, Mi.nMarkers
    else:
        geno_index = {g: i for i, g in enumerate(Mi.obsID)}
        keep = usable & ph[idcol].isin(geno_index).to_numpy()
        ph = ph.loc[keep].reset_index(drop=True)
        if len(ph) == 0:
            raise ValueError("no individual has both phenotypes and genotypes")
        rows = np.array([geno_index[i] for i in ph[idcol]], dtype=np.int64)
        X = None if gblup else Mi.genotypes if (len(rows) == Mi.nObs and np.array_equal(rows, np.arange(Mi.nObs))) else np.asfortranarray(Mi.genotypes[rows, :])
        n, p = (len(rows), len(rows)) if gblup else X.shape            # (GBLUP: nMarkers = nObs; the eigenvectors come below)
    # ---- individuals EBVs are reported for (check_outputID, input_data_validation.jl:143-196): all genotyped
    # individuals unless outputEBV(model, IDs) named a list; IDs without genotypes are dropped with the reference's note
    out_ids, out_rows, out_same = None, None, True
    plink_out = False                          # the output individuals are packed rows of a PLINK fileset (below)
    if outputEBV and single_step is not None:      # the pedigree's IDs or the caller's list within it (:173,187-195); its matrix is resident (ssbr.py)
        out_ids, out_same = list(single_step.out_ids), False
    elif outputEBV and devres and getattr(Mi, "plink_source", None) is not None and getattr(model, "output_ID", False) is not False:
        # plink_genotypes: the genotyped individuals are ALL of the fileset, not only the kept ones; those of the caller's list that
        # are not the training records become 2-bit packed output rows beside the packed training storage (plink.load_plink_output)
        from . import plink as _plink
        out_ids = _plink.resolve_plink_output_ids(Mi.plink_source, model.output_ID)
        if not out_ids:
            raise ValueError("outputEBV(model, IDs): none of the listed individuals is in the fileset's .fam file")
        out_same = out_ids == list(ph[idcol])
        plink_out = not out_same
        missing_ = [m_ for m_ in ("plink_scan", "plink_commit_output", "mul_alpha_output") if plink_out and not hasattr(engine, m_)]
        if missing_:
            raise NotImplementedError("outputEBV(model, IDs) on a PLINK fileset needs an engine with " + ", ".join(missing_)
                                      + "; the package has no CPU fallback")
    elif outputEBV:
        out_ids, out_same = resolve_output_ids(model, Mi.obsID, ph[idcol])      # (out_same: exactly the training rows, same order: X itself)
        if not out_same:
            if stream or devres:
                raise NotImplementedError("storage=:stream reports EBVs for the genotyped individuals in file order "
                                          "(outputEBV(model, IDs) lists stay on the reference)")
            gi = {g: i for i, g in enumerate(Mi.obsID)}
            out_rows = np.array([gi[i] for i in out_ids], dtype=np.int64)
    if not stream and not devres:
        # rows of Mi.genotypes behind Mi.output_genotypes (tools4genotypes.jl:290-296); GWAS() reads them (GWAS.jl:148)
        Mi.output_rows = out_rows if (outputEBV and not out_same) else rows
    write_id_files(output_folder, ph[idcol], Mi.obsID)
    if gblup:
        # GBLUP_setup (GBLUP.jl:9-31) in place of the block set-up: K aligned to the records, K = L D L', the pseudo-markers' names,
        # the output matrix K[out, records] L diag(1 / D); X = L is what goes to the device
        gb = _gb.prepare(Mi, rows, out_rows if (outputEBV and not out_same) else None, ftype, gblup_eigen=gblup_eigen, device=device)
        X = gb.L
    liab_codes, liab_bounds = {}, {}
    if has_liab:                                                          # input_data_validation.jl:255-290
        for k, tr in enumerate(model.lhsVec):
            if traits_type[k] == "categorical":
                col = ph[tr].to_numpy(dtype=np.float64)
                obs = col[np.isfinite(col)]
                if not np.all(obs == np.floor(obs)):
                    raise ValueError(f"For categorical trait {tr}, the categories should be integers 1, 2, 3, ...")
                user = sorted(set(int(v) for v in obs))
                correct = list(range(1, len(user) + 1))
                if user != correct:
                    raise ValueError(f"For categorical trait {tr}, the categories should be {correct} ; instead of {user}")
                if len(user) > 15:
                    raise NotImplementedError(f"categorical trait {tr}: at most 15 categories on the device (got {len(user)})")
                if len(user) < 2:
                    raise ValueError(f"For categorical trait {tr}, at least two categories must be observed")
                if len(user) == 2:
                    traits_type[k] = "categorical(binary)"
                liab_codes[k] = np.where(np.isfinite(col), col, 0.0).astype(np.int32)       # 0 = missing (:54,115-117)
            elif traits_type[k] == "censored":
                liab_bounds[k] = (ph[f"{tr}_l"].to_numpy(dtype=np.float64), ph[f"{tr}_u"].to_numpy(dtype=np.float64))
        for lab, typ in (("Censored traits are: ", "censored"), ("Categorical traits (>2 categories) are: ", "categorical"),
                         ("Binary traits are: ", "categorical(binary)")):
            names_ = [tr for tr, tt in zip(model.lhsVec, traits_type) if tt == typ]
            if names_:
                print(lab + str(names_))
        if t > 1 and "categorical(binary)" in traits_type:
            print(" - note that binary traits are assumed to be independent with unit variance.")
    binary_index = [k for k in range(t) if traits_type[k] == "categorical(binary)"]
    liab_traits = [k for k in range(t) if traits_type[k] in LIABILITY_TYPES]
    ngibbs = 5 if len(liab_traits) > 1 else 1                             # categorical_and_censored_trait.jl:184-188
    Y = np.stack([ph[tr].to_numpy(dtype=ftype) for tr in model.lhsVec])       # t x n
    observed = np.isfinite(Y).T                                                     # n x t: mme.missingPattern (residual.jl:17-21)
    has_missing = not observed.all()
    if sem and has_missing:                                               # SEM.jl:51: no missing phenotypes in SEM
        raise ValueError("causal_structure needs complete records: some training records miss the phenotype of a trait.")
    phenovar = np.array([np.var(Y[k][observed[:, k]].astype(np.float64), ddof=1) for k in range(t)])
    Y = np.where(np.isfinite(Y), Y, ftype(0)).astype(ftype)               # imputed before first use (residual.jl:52-73)
    invw = None
    if heterogeneous_residuals:                                           # build_MME.jl:305-310
        if "weights" not in ph.columns:
            raise ValueError("heterogeneous_residuals=true requires a column named weights in the phenotype data.")
        invw = (1.0 / ph["weights"].to_numpy(dtype=np.float64)).astype(ftype)
        if not np.all(np.isfinite(invw) & (invw > 0)):
            raise ValueError("weights must be positive and finite.")
    w64 = np.ones(len(ph)) if invw is None else invw.astype(np.float64)

    # ---- default priors (input_data_validation.jl:296-350, tools4genotypes.jl:353-478, build_MME.jl:128-141)
    rnd = list(getattr(model, "rndTrmVec", []))
    ped_count = sum(re_.randomType == "A" for re_ in rnd)    # genetic_random_count = the genotypes + the pedigree effect (:301-312)
    varg = np.diag(phenovar) * 0.5 / (1 + ped_count)
    vare0 = np.diag(phenovar) * 0.5 / (1 + sum(re_.randomType != "A" and re_.name != "ϵ" for re_ in rnd))       # nongenetic_random_count (input_data_validation.jl:301-313): only an i.i.d. set_random term changes it
    vare_rnd = vare0.copy()                                # ... what the random effects' default prior reads (:352-365)
    R = model.R
    if R.val is False:
        single_cat = t == 1 and traits_type[0] in ("categorical", "categorical(binary)")
        if single_cat:                         # known to be 1.0 in a single-trait threshold model (input_data_validation.jl:333-338)
            vare0[0, 0] = 1.0
            R.estimate_variance = False
        for k in (binary_index if t > 1 else []):                      # :341-349: binary traits independent with unit variance
            vare0[k, :] = 0.0
            vare0[:, k] = 0.0
            vare0[k, k] = 1.0
            vare_rnd[k, k] = 1.0
        R.val = ftype(vare0[0, 0]) if t == 1 else vare0.astype(ftype)
        R.scale = float(R.val) * (float(R.df) - 2) / float(R.df) if t == 1 else np.asarray(R.val, dtype=np.float64) * (float(R.df) - t - 1)
        if t > 1 and len(binary_index) == t:
            R.constraint = True
            R.estimate_variance = False
    if Mi.G.val is False and Mi.genetic_variance.val is False:
        Mi.genetic_variance.val = varg[0, 0] if t == 1 else varg
    for re_ in rnd:                                                       # :352-365
        if re_.Gi.val is False:
            kk = len(re_.traits)
            G0_ = np.diag([(varg if re_.randomType == "A" else vare_rnd)[m, m] for m in re_.traits])      # :359-363
            re_.Gi.val = np.linalg.inv(G0_)
            re_.Gi.scale = G0_ * (float(re_.Gi.df) - kk - 1)
    pi = Mi.pi
    if isinstance(pi, dict):
        # the reference's multi-trait Pi: Dict(state vector => probability), e.g. Dict([1.0,0.0] => 0.1, ...)
        # (tools4genotypes.jl:357-373, test/runtests.jl); device order: state index = sum_k delta_k << k
        if t == 1:
            raise ValueError("a Dict Pi is for multi-trait analyses only")
        tab = np.zeros(1 << t)
        for key, val in pi.items():
            key = tuple(float(v) for v in key)
            if len(key) != t or any(v not in (0.0, 1.0) for v in key):
                raise ValueError(f"Pi keys must be 0/1 vectors of length {t} (got {key})")
            tab[sum(1 << k for k in range(t) if key[k] == 1.0)] = float(val)
        if abs(tab.sum() - 1.0) > 1e-6:
            raise ValueError("Summation of probabilities of Pi is not equal to one.")       # input_data_validation.jl
        pi = tab
    if (t > 1 and getattr(Mi, "annotations", False) is not False and np.ndim(pi) == 1 and len(pi) == Mi.nMarkers
            and len(pi) != (1 << t) and np.all(np.asarray(pi) == np.asarray(pi)[0])):
        # get_genotypes expanded a scalar Pi to one value per marker for annotated BayesC before the number of traits was
        # known (readgenotypes.jl:111-150); the multi-trait set-up reads the scalar (annotation_setup.jl:106-118)
        pi = float(np.asarray(pi)[0])
    if t > 1 and (np.isscalar(pi) and pi == 0.0):                      # tools4genotypes.jl:357-373
        pi = np.zeros(1 << t)
        pi[(1 << t) - 1] = 1.0
        Mi._pi_was_default = True
    if method == "BayesR" and np.isscalar(pi) and pi == 0.0:           # :375-377
        pi = np.array([0.95, 0.03, 0.015, 0.005])
    if method == "BayesA":                                             # input_data_validation.jl:33-36
        method, Mi.estimatePi = "BayesB", False
        pi = 0.0 if t == 1 else np.eye(1, 1 << t, (1 << t) - 1).ravel()  # every marker in the model for every trait
    lasso = method == "BayesL"
    if lasso:
        # Bayesian LASSO (BayesL!, BayesC0L.jl:25-47): every marker in the model, effect variance G*gamma_j with the
        # gamma_j updated by Metropolis-Hastings on the host (sampleGammaArray!, variance_components.jl:191-203).  Its full
        # conditional lhs = x'x + (vare/G)/gamma_j is the device's BayesB update with pi = 0 and var_j = G*gamma_j.
        if t > 1:
            raise NotImplementedError("multi-trait BayesL stays on the reference")
        if not (np.isscalar(pi) and (pi is False or pi == 0.0)):
            print("BayesL runs with π = false.")                        # input_data_validation.jl:24-31
        elif Mi.estimatePi:
            print("BayesL runs with estimatePi = false.")
        method, pi, Mi.estimatePi = "BayesB", 0.0, False
    if method == "RR-BLUP":                                            # input_data_validation.jl:24-31
        if not (np.isscalar(pi) and (pi is False or pi == 0.0)):
            print("RR-BLUP runs with π = false.")
        elif Mi.estimatePi:
            print("RR-BLUP runs with estimatePi = false.")
        # the device's BayesC update with pi = 0 (every marker included) is RR-BLUP's full conditional (api.SUPPORTED_METHODS)
        method, Mi.estimatePi = "BayesC", False
        pi = 0.0 if t == 1 else np.eye(1, 1 << t, (1 << t) - 1).ravel()
    if gblup:                                                          # input_data_validation.jl:24-31; tools4genotypes.jl:409-410
        if not (np.isscalar(Mi.pi) and (Mi.pi is False or Mi.pi == 0.0)):
            print("GBLUP runs with π = false.")
        elif Mi.estimatePi:
            print("GBLUP runs with estimatePi = false.")
        # every pseudo-marker is in the model: the state, the running means and the outputs are RR-BLUP's (the device's BayesC state)
        method, Mi.estimatePi = "BayesC", False
        pi = 0.0 if t == 1 else np.eye(1, 1 << t, (1 << t) - 1).ravel()
        Mi.G.val = np.float64(Mi.genetic_variance.val) if t == 1 else np.asarray(Mi.genetic_variance.val, dtype=np.float64)
    if t == 2 and getattr(Mi, "annotations", False) is not False and not mega:
        # start-row validation of the annotated 2-trait model comes first (finalize_marker_annotation_setup!,
        # annotation_setup.jl:101-121, runs at build_model time in the reference)
        from . import annotations as A_
        A_.bayesc_mt_start_row(0.0 if getattr(Mi, "_pi_was_default", False) else pi)
    if Mi.G.val is False:
        Mi.G.val = genetic2marker(Mi, pi, method, t)
        if (t == 1 and not Mi.G.val > 0) or (t > 1 and (not np.all(np.isfinite(Mi.G.val)) or np.any(np.linalg.eigvalsh(Mi.G.val) <= 0))):
            raise ValueError("Marker effects variance is negative!" if t == 1 else
                             "Marker effects covariance matrix is not postive definite! Please modify the argument: Pi.")
    ann = getattr(Mi, "annotations", False)
    if ann is not False:
        from . import annotations as A_
        if t > 1:                                                      # annotation_setup.jl:101-133
            if t != 2:
                raise ValueError("Annotated multi-trait BayesC currently supports exactly 2 traits.")
            if mega:
                raise NotImplementedError("annotated multi-trait BayesC with constraint=true stays on the reference")
            start_row = A_.bayesc_mt_start_row(0.0 if getattr(Mi, "_pi_was_default", False) else pi)
            ann = Mi.annotations = A_.initialize_bayesc_mt(ann.design_matrix, start_row)
            pi = start_row.copy()
        if stream:
            raise NotImplementedError("marker annotations with storage=:stream stay on the reference")
        if method == "BayesC":                                         # annotation_setup.jl:78-99
            pi = np.array(pi, dtype=np.float64) if np.ndim(pi) == 1 else np.full(p, float(pi))
            A_.initialize_bayesc_single_trait(ann, pi)
        Mi.estimatePi = True
    Gdf = float(Mi.G.df)
    Mi.G.scale = (np.float64(Mi.G.val) * (Gdf - 2) / Gdf) if t == 1 else np.asarray(Mi.G.val, dtype=np.float64) * (Gdf - t - 1)   # :414-418
    Rdf = float(R.df)
    if t > 1 and R.constraint:                                         # R_constraint! (input_data_validation.jl:530-540)
        Rdf -= t
        R.scale = np.diag(np.diag(np.asarray(R.scale, dtype=np.float64)) / (Rdf - 1)) * (Rdf - 2) / Rdf
        R.val = np.diag(np.diag(np.asarray(R.val, dtype=ftype)))
    pi_t = None
    if mega:                                                           # G_constraint! (input_data_validation.jl:543-559)
        Gdf -= t
        Mi.G.scale = np.diag(np.diag(np.asarray(Mi.G.scale, dtype=np.float64)) / (Gdf - 1)) * (Gdf - 2) / Gdf
        Mi.G.val = np.diag(np.diag(np.asarray(Mi.G.val, dtype=ftype)))
        # megaBayesABC! reads one pi per trait (genotypes.pi[i], BayesABC.jl:5).  The reference only holds the joint
        # 2^t table before the first samplePi; the per-trait value used here is its marginal Pr(delta_k = 0).
        pa = np.asarray(pi, dtype=np.float64)
        pi_t = np.array([pa[[s_ for s_ in range(1 << t) if not (s_ >> k) & 1]].sum() for k in range(t)]) if pa.size == (1 << t) else pa
        if pi_t.shape != (t,):
            raise ValueError(f"Pi must hold one value per trait or one per joint state (got {pa.size} entries for {t} traits)")
    sampler = getattr(Mi, "multi_trait_sampler", "I")                   # mt_bayesc_sampler_mode (MTBayesABC.jl:20-25)
    if t > 1 and sampler == "auto":
        # support-based dispatch: a Pi Dict that does not list every joint state (a restricted support, where sampler I
        # cannot move between the listed states) selects the joint-state sampler II
        n_states = len(Mi.pi) if isinstance(Mi.pi, dict) else (1 << t)
        sampler = "I" if n_states == (1 << t) else "II"
    mt_method = "MegaBayesC" if mega else ("MTBayesC_II" if sampler == "II" else "MTBayesC")
    mt_pervar = t > 1 and method == "BayesB"        # multi-trait BayesA/B: one t x t effect covariance per marker
    if mt_pervar:
        if getattr(Mi, "annotations", False) is not False:
            raise NotImplementedError("annotated multi-trait BayesB stays on the reference")
        # constraint = true: megaBayesABC! reads every marker's own diagonal (BayesABC.jl:5)
        mt_method = "MegaBayesB" if mega else ("MTBayesB_II" if sampler == "II" else "MTBayesB")
        if independent_blocks:
            raise NotImplementedError("independent_blocks with multi-trait BayesA/B (one effect covariance per marker) stays on the reference")

    # ---- fast_blocks parsing (JWAS.jl:293-316); device blocks are powers of two >= 64
    nreps = 1
    explicit_partition = None                                          # 0-based starts of a non-uniform explicit partition
    if fast_blocks is not False:
        explicit_starts = False
        if fast_blocks is True:
            want = int(np.floor(np.sqrt(n)))
        elif np.isscalar(fast_blocks):
            want = int(np.floor(fast_blocks))
        else:
            try:
                starts = [int(v) for v in fast_blocks]
            except (TypeError, ValueError):
                raise ValueError("fast_blocks must be false, true, a positive number, or a vector of block start positions.")
            if any(int(v) != v for v in fast_blocks):
                raise ValueError("fast_blocks must be false, true, a positive number, or a vector of block start positions.")
            if len(starts) == 0:                                         # validate_fast_block_starts (JWAS.jl:73-79)
                raise ValueError("fast_blocks block start vector cannot be empty.")
            if starts[0] != 1:
                raise ValueError("fast_blocks block starts must begin with 1.")
            if not all(1 <= v <= p for v in starts):
                raise ValueError("fast_blocks block starts must be within 1:nMarkers.")
            if not all(b_ > a_ for a_, b_ in zip(starts, starts[1:])):
                raise ValueError("fast_blocks block starts must be sorted and unique.")
            sizes = [b_ - a_ for a_, b_ in zip(starts, starts[1:])] + [p - starts[-1] + 1]
            if len(starts) < 2:
                raise ValueError("fast_blocks block size must create at least two block starts.")
            # the reference does not rescale chain_length for explicit starts (JWAS.jl:298-304: block_size = false)
            explicit_starts = True
            if max(sizes) > max(DEVICE_BLOCK_SIZES):
                # a block of more than 1024 markers does not fit the sampler's LDS plan: the nearest legal partition is the
                # given one with every oversized block cut into k = ceil(size / 1024) BALANCED pieces (sizes differ by at
                # most one marker: no sliver of a tail piece), each piece repeated its own size (BayesABC.jl:153) -- a valid
                # chain with MORE within-block sweeps per outer iteration than the request (a block of 1150 markers becomes
                # 575 + 575 repetitions of half-blocks instead of 1150 of the whole); chain_length, the number of saved
                # samples and of hyper-parameter updates are unchanged.  Said out loud, as the reference prints its block
                # size (JWAS.jl:308-316).
                lim = max(DEVICE_BLOCK_SIZES)
                cut = []
                for a_, sz in zip(starts, sizes):
                    k_ = -(-sz // lim)
                    base, extra = divmod(sz, k_)
                    pos = a_
                    for i_ in range(k_):
                        cut.append(pos)
                        pos += base + (1 if i_ < extra else 0)
                print(f"NOTICE: fast_blocks blocks of up to {max(sizes)} markers exceed the device limit of {lim}; "
                      f"running {len(cut)} blocks (oversized blocks cut into balanced pieces of at most {lim} markers, each "
                      f"repeated its own size: the schedule differs from the request's, the number of saved samples does not)")
                starts = cut
                sizes = [b_ - a_ for a_, b_ in zip(starts, starts[1:])] + [p - starts[-1] + 1]
            if len(set(sizes[:-1])) != 1 or sizes[-1] > sizes[0]:
                # NON-UNIFORM partition: the device runs exactly these blocks, each with its own size as repetition count
                # (BayesABC.jl:153); jwas_hip_setup_blocks_explicit
                explicit_partition = np.asarray(starts, dtype=np.int64) - 1
            want = max(sizes) if explicit_partition is not None else sizes[0]
        if want < 1:
            raise ValueError("fast_blocks block size must be at least 1.")
        if want >= p:                                                   # range(1, step=want, stop=p) has one start
            raise ValueError("fast_blocks block size must create at least two block starts.")
        # The schedule AND the partition are the reference's (JWAS.jl:308-312): block starts collect(range(1, step=want,
        # stop=p)), every block repeated its own size (BayesABC.jl:153: the last, shorter block fewer times), and
        # chain_length / want outer iterations -- the same number of hyper-parameter updates and saved samples.
        #   * `want` is one of the device's uniform block sizes (64 ... 1024): the uniform layout IS that partition
        #     (nreps <= 0 = every block its own size);
        #   * any other size <= 1024: the ragged-partition form (jwas_hip_setup_blocks_explicit) with those starts;
        #   * more than 1024 markers per block do not fit the sampler's LDS plan: the nearest legal schedule with a printed
        #     NOTICE (below: blocks of 1024 markers, chain_length / 1024 outer iterations -- fewer saved samples and
        #     hyper-parameter updates per requested iteration than chain_length / want would give)
        #     (independent_blocks alone may ask for more: uniform device blocks of 1024 markers with `want` repetitions
        #     each -- independent blocks are the reference's own approximation).
        if want > max(DEVICE_BLOCK_SIZES) and not explicit_starts and not independent_blocks:
            # fast_blocks = true on more than 1024^2 records, or a number above 1024: the sampler's LDS plan holds the draws,
            # constants and staged Gram rows of at most 1024 markers.  The nearest legal schedule is the reference's own at
            # the largest device size -- blocks of 1024 markers, each repeated 1024 times, chain_length / 1024 outer
            # iterations -- and the run says so where the reference prints its block size (JWAS.jl:308-316).
            print(f"NOTICE: fast_blocks block size {want} exceeds the device limit of {max(DEVICE_BLOCK_SIZES)} markers per block; "
                  f"running BLOCK SIZE {max(DEVICE_BLOCK_SIZES)} (chain_length / {max(DEVICE_BLOCK_SIZES)} outer iterations)")
            want = max(DEVICE_BLOCK_SIZES)
        if not explicit_starts:
            chain_length = int(np.floor(chain_length / want))
        if explicit_partition is None and want not in DEVICE_BLOCK_SIZES and want <= max(DEVICE_BLOCK_SIZES):
            explicit_partition = np.arange(0, p, want, dtype=np.int64)          # = collect(range(1, step=want, stop=p)) - 1
            sizes = [want] * (len(explicit_partition) - 1) + [p - int(explicit_partition[-1])]
        block_size = _supported_block(want)
        nreps = want if (explicit_partition is None and want not in DEVICE_BLOCK_SIZES) else 0   # 0: every block its own size
        if plain_pass:
            nreps = 1            # the reference's schedule for these methods: chain_length / block size plain passes
        if explicit_partition is not None:
            while block_size < want:
                block_size *= 2
            print(f"BLOCK STARTS: {len(explicit_partition)} blocks of {min(sizes)}..{max(sizes)} markers")
        else:
            print(f"BLOCK SIZE: {want}" + (f" (device blocks of {min(block_size, p)} markers)" if min(block_size, p) != want else ""))
    if mt_pervar and block_size is not None and block_size * t > 2048:
        # the markers' own covariances are parked in LDS beside their draws (sampler_mt.hpp): known before anything is loaded
        raise NotImplementedError(f"multi-trait BayesA/B needs fast_blocks * traits <= 2048 on the device (got {block_size} x {t})")
    adaptive = False
    adaptive_mt = False
    adaptive_mts = False
    mt_1024 = False
    section_solve = False
    if block_size is None:
        # Device block size.  Sparse priors (few markers change per sweep): big blocks amortise the per-launch cost.
        # Dense priors (every marker is in the model: Pi = 0 / BayesA / the multi-trait default of all-ones) change
        # every marker every sweep, so the whole block Gram must sit in LDS: 128 x 128 floats.
        if mega:
            dense = float(np.mean(pi_t)) < 0.5
        elif t > 1:
            dense = float(np.asarray(pi, dtype=np.float64)[(1 << t) - 1]) > 0.5
        elif method == "BayesR":
            dense = float(np.asarray(pi, dtype=np.float64)[0]) < 0.5
        else:
            dense = float(np.mean(pi)) < 0.5
        # ... except when the prior includes every marker whatever its rhs (single-trait BayesA / B / C with Pi = 0, RR-BLUP,
        # BayesL): the sampler's dense_big_st path walks 512-marker blocks section by section (diagonal Gram tiles in LDS,
        # the rest applied in parallel) -- four times fewer launches of the streaming role.
        all_in = (t == 1 and method in ("BayesC", "BayesB") and np.ndim(pi) == 0 and float(pi) == 0.0 and not Mi.estimatePi
                  and getattr(Mi, "annotations", False) is False)
        # ... and multi-trait BayesC sampler I with one shared covariance and the shared prior table (the reference's default
        # all-ones prior): 256-marker blocks through dense_big_mt (round 4)
        mt_big = (t > 1 and not mega and mt_method in ("MTBayesC", "MTBayesB") and getattr(Mi, "annotations", False) is False)
        block_size = (512 if all_in else (256 if mt_big else 128)) if dense else 512
        while block_size > 64 and p <= block_size:
            block_size //= 2
        while mt_pervar and block_size * t > 2048:                      # the markers' own constants are parked in LDS
            block_size //= 2
        # Rule T (jwas_sweep_params.section_solve, round 5): the dense 256-marker blocks of sampler I as triangular solves with
        # per-sweep section inverses (at most three traits, Float32 context, the plain single-pass schedule)
        section_solve = bool(dense and mt_big and t <= 3 and block_size == 256 and not double_precision and fast_blocks is False
                             and not independent_blocks)
        # Sparse priors: keep a second, larger block size resident and pick per sweep from the previous sweep's number
        # of effect changes (a chain quantity, so runs stay reproducible): 1024-marker blocks amortise the per-launch cost
        # once fewer than ~1.3 % of the markers change per sweep (measured crossover at 50k x 600k: 8 900 changes).
        # (single-trait only: the multi-trait samplers are bound by the serial phase, not by launches, and at 1024
        # markers x 3 traits the per-marker draws no longer fit LDS next to the staged Gram rows -- measured 10.0 vs 8.9 ms
        # per sweep at 20k x 100k x 3 traits)
        adaptive = (not dense) and t == 1 and block_size == 512 and p > 4 * 1024
        # (multi-trait chains that start dense: 256-marker blocks now, 512 once the chain has become sparse -- pick_block_size_mt)
        adaptive_mt = bool(dense and mt_big and block_size == 256 and p > 4 * 512 and 512 * t <= 2048)
        mt_1024 = adaptive_mt and mt_1024_allowed(t, p, mt_pervar)
        # (multi-trait chains that START sparse: 512-marker blocks, 1024 for the sweeps below 0.5 % turnover -- the same last level)
        adaptive_mts = bool((not dense) and t > 1 and block_size == 512 and mt_1024_allowed(t, p, mt_pervar)
                            and getattr(Mi, "annotations", False) is False)      # (marker-specific prior tables: their LDS copy does not fit at 1024 x 3)
        mt_1024 = mt_1024 or adaptive_mts

    if double_precision:
        # the Float64 device context (csrc/f64_path.hpp): dense storage; single-trait BayesA/B/C (+ RR-BLUP, BayesL through
        # them), BayesR, multi-trait BayesC and BayesA/B under sampler I and II, marker-specific joint priors; any fast_blocks
        # partition with blocks of <= 1024 markers (uniform or explicit starts), independent_blocks, residual weights; block
        # size x traits <= 2048
        if stream or (devres and single_step is None):      # (a single-step run imputes into a Float64 context's own matrix: ssbr.py)
            raise NotImplementedError("double_precision=true needs dense host genotypes (the streaming backend is Float32 only, readgenotypes.jl:246-248)")
        if mega and not gblup:
            raise NotImplementedError("double_precision=true runs every sampler on the device except constraint=true (megaBayesABC), "
                                      "which stays on the reference in Float64 mode")
        if fast_blocks is not False:
            if explicit_partition is None:
                block_size = want                      # (the Float64 context runs uniform blocks of ANY size <= 1024 as they are)
        else:
            # two stream-ordered launches per block, no lookahead: big blocks amortise them (20k x 20k BayesC: 6.8 ms per sweep
            # at 128 markers per block, 2.1 ms at 512 -- scripts/f64_bench.py); the chain is the same whatever the size
            block_size = 512
            while block_size > 64 and p <= block_size:
                block_size //= 2
        if block_size * t > 2048:
            raise NotImplementedError(f"double_precision=true needs fast_blocks * traits <= 2048 on the device (got {block_size} x {t})")
        adaptive = False
        adaptive_mt = False
        adaptive_mts = False
        mt_1024 = False

    if gblup:                                  # no blocks: nothing of the block policies applies
        adaptive = adaptive_mt = adaptive_mts = mt_1024 = section_solve = False

    # grouped launches (engine.setup_groups): the adaptive policy's 1024-marker sweeps of a single-trait chain (dense or 2-bit packed
    # storage), when the chain is long enough to pay for the group cross-Grams; an explicitly partitioned / row-sharded run keeps
    # one block per launch
    group_m = 0
    if adaptive and not double_precision and explicit_partition is None and not independent_blocks and fast_blocks is False:
        # (blocks_per_launch: None = by the chain's length; 0 / 2 / 4 = the caller's choice -- a device option like block_size)
        group_m = grouped_blocks_for_chain(chain_length) if blocks_per_launch is None else int(blocks_per_launch)
        if not grouped_launch_size(method, t, False, 1024, group_m):
            group_m = 0
    pair_m = 0                                 # ... and ping-pong pairs on the 512-marker sweeps of a high-turnover chain (dense storage)
    if adaptive and not double_precision and explicit_partition is None and not independent_blocks and fast_blocks is False and not stream:
        pair_m = pingpong_pairs_for_chain(method, bool(Mi.estimatePi), chain_length) if blocks_per_launch is None else (2 if int(blocks_per_launch) else 0)
        if pair_m == 4 and 4 * p * 512 * 5 > 0.05 * 288e9:      # (pair + four cross-Grams of the 512-marker set: keep them a small part of the HBM)
            pair_m = 2
        if not grouped_launch_size(method, t, False, 512, pair_m):
            pair_m = 0

    from .engine import SectionSolvePolicy
    solve_policy = SectionSolvePolicy(section_solve, 4 * (p // 256))

    # ---- location parameters: on the host (dense design matrices, today's path) or on the device (csrc/locpar.hpp)
    lp_terms, labels = _location_terms(model, ph)
    q = [len(lab) for lab in labels]
    lp_device = location_parameters == "device" or (location_parameters == "auto" and (bool(rnd) or sum(q) > LOCPAR_AUTO_LEVELS))
    mt_device = False
    if lp_device and t > 1 and has_missing:
        # the reference's per-record Ri (mkRi, residual.jl:2-44) does not factor as kron(inv(R), diag(w)): the device imputes the
        # missing residuals and weights record by record (csrc/mtmiss.hpp); a fixed-only model under "auto" keeps the host scan
        if not rnd and location_parameters == "auto":
            lp_device = False
        else:
            eng_ = engine if engine is not None else (Mi.device_backend if devres else None)
            missing_ = [m_ for m_ in MTMISS_METHODS if eng_ is not None and not hasattr(eng_, m_)]
            if missing_:
                raise NotImplementedError("location parameters on the device need complete multi-trait records (the per-record Ri of "
                                          "partially missing records stays on the host path, which has no random effects); the engine "
                                          "lacks " + ", ".join(missing_))
            mt_device = True
    if rnd and not lp_device:
        raise NotImplementedError('set_random effects run on the device: location_parameters="host" has no random effects')
    if lp_device:
        eng_ = engine if engine is not None else (Mi.device_backend if devres else None)
        missing_ = [m_ for m_ in LOCPAR_METHODS if eng_ is not None and not hasattr(eng_, m_)]
        if missing_:
            raise NotImplementedError("location parameters on the device need an engine with the locpar step (" + ", ".join(missing_)
                                      + " missing); the package has no CPU fallback")
        for g_, re_ in enumerate(rnd):
            for m in re_.traits:
                kind_ = [kd for nm, kd, _ in lp_terms[m] if nm == re_.name]
                if kind_ != ["factor"]:
                    raise NotImplementedError(f"set_random: {re_.name} must be one class factor of trait {model.lhsVec[m]} "
                                              "(random covariates stay on the reference)")
        if len(rnd) > 8:
            raise NotImplementedError("at most 8 set_random effects on the device")
        if any(re_.randomType in ("A", "V") for re_ in rnd):
            missing_ = [m_ for m_ in LOCPAR_PED_METHODS if eng_ is not None and not hasattr(eng_, m_)]
            if missing_:
                raise NotImplementedError("a pedigree random effect needs an engine with " + ", ".join(missing_) + "; the package has no CPU fallback")

    # ---- annotation priors: the probit update on the host (annotations.py, numpy's generator) or on the device from the
    # resident delta (csrc/annot.hpp, the counter RNG)
    ann_device = annotation_priors == "device" and ann is not False
    if ann_device:
        eng_ = engine if engine is not None else (Mi.device_backend if devres else None)
        missing_ = [m_ for m_ in ANNOT_METHODS if eng_ is not None and not hasattr(eng_, m_)]
        if missing_:
            raise NotImplementedError("annotation priors on the device need an engine with the annotation step (" + ", ".join(missing_)
                                      + " missing); the package has no CPU fallback")
        if eng_ is not None and hasattr(eng_, "comm_info") and eng_.comm_info()[1] > 1:
            raise NotImplementedError("annotation priors on the device are not driven from marker shards")
        ann_kind = "tree" if t > 1 else method

    # ---- engine (the only engine shipped is the HIP one; there is no CPU fallback)
    own_engine = engine is None
    if own_engine:
        from .engine import HipEngine
        need = HipEngine.estimate_bytes(n, p, t, block_size, "stream" if stream else "dense") * (2 if double_precision else 1)
        if adaptive or adaptive_mt:
            need += 2 * 4 * (1024 if adaptive else 512) * p        # the second resident block size (Grams + cross-Grams)
        if mt_1024:
            need += 2 * 4 * 1024 * p                               # ... and the third one of a multi-trait chain
        if group_m:
            need += 4 * p * 1024 * (5 if group_m == 4 else 2)      # grouped launches: pair (4 blocks: the odd pairs + the fours) cross-Grams of the 1024-marker set
        if pair_m:
            need += 4 * p * 512 * (5 if pair_m == 4 else 2)       # ... and the pair (4 blocks: odd pairs + fours) cross-Grams of the 512-marker set
        if double_precision and independent_blocks:
            # Float64 independent blocks: one change list of 1024 entries per block (4 + 4 x 8 bytes per entry, whatever the
            # block size) and one partial-sum buffer per block (4 traits x row slices x block doubles)
            nb_ = -(-p // max(1, block_size))
            need += nb_ * (4 + 1024 * (4 + 4 * 8)) + 4 * 8 * (-(-n // 256)) * nb_ * block_size
        if double_precision and mt_pervar:
            need += p * t * t * 8 * 2                              # Float64 multi-trait BayesA/B: the covariances and their inverses in double
        if lp_device:                                              # the term layouts, sol and its means (jwas_hip_locpar_estimate_bytes)
            need += HipEngine.locpar_estimate_bytes(n, sum(len(tk) for tk in lp_terms), sum(q))
            for re_ in rnd:                                        # A-inverse and its colours (jwas_hip_lp_structure_estimate_bytes)
                if re_.randomType in ("A", "V"):
                    need += HipEngine.locpar_structure_estimate_bytes(re_.Vinv.shape[0], re_.Vinv.nnz)
        if mt_device:                                              # the records' codes, the tables, the second piece sums
            need += HipEngine.mtmiss_estimate_bytes(n)
        if ann_device:                                             # the design matrix, liabilities, the table's means (jwas_hip_annot_estimate_bytes)
            need += HipEngine.annot_estimate_bytes(p, ann.design_matrix.shape[1], ann_kind)
        if sem:                                                    # the phenotypes, the indirect / overall accumulators (jwas_hip_sem_estimate_bytes)
            need += HipEngine.sem_estimate_bytes(n, p, t)
        if gblup:                                                  # r + L alpha, the right-hand sides, the column-part sums (jwas_hip_gblup_estimate_bytes)
            need += HipEngine.gblup_estimate_bytes(n, t, 64 if double_precision else 32)
        if outputEBV and not out_same:                             # Mi.output_genotypes: a second dense matrix (n_out x p)
            need += (8 if double_precision else 4) * ((len(out_rows) + 255) // 256 * 256) * p
        engine = HipEngine(device, precision=64 if double_precision else 32)
        free = engine.device_info()["hbm_free"]
        if memory_guard != "off" and need > memory_guard_ratio * free:   # JWAS.jl:422-459 analogue for HBM
            msg = (f"marker path needs {need / 1e9:.2f} GB of HBM, more than {memory_guard_ratio:.2f} x free "
                   f"({free / 1e9:.2f} GB)")
            if memory_guard == "error":
                engine.close()
                raise MemoryError(msg)
            print("WARNING: " + msg)
    if devres:
        pass                                   # already resident
    elif stream:
        engine.load_jgb2(Mi.stream_backend["prefix"])          # payload stays 2-bit packed in HBM
    else:
        engine.load_dense(np.asfortranarray(X, dtype=ftype))      # after alignment (tools4genotypes.jl:310-321); Float64 on request (JWAS.jl:353)
    X_out_host = None
    if plink_out:                              # once, before the chain: the rows stay resident for all of it
        _plink.load_plink_output(engine, Mi.plink_source, out_ids, memory_guard=memory_guard, memory_guard_ratio=memory_guard_ratio)
    elif outputEBV and not out_same and single_step is None:      # Mi.output_genotypes = Z_out * genotypes (tools4genotypes.jl:290-296)
        if double_precision and not (hasattr(engine, "load_output_dense") and hasattr(engine, "mul_alpha_output")):
            X_out_host = np.asarray(gb.Xout if gblup else Mi.genotypes[out_rows, :], dtype=np.float64)      # (an injected engine without output rows: the host forms the product)
        else:                                  # a second resident matrix, Float64 in a Float64 run (JWAS.jl:353)
            Xo = gb.Xout if gblup else Mi.genotypes[out_rows, :]
            engine.load_output_dense(np.asfortranarray(Xo, dtype=np.float64) if double_precision else np.asfortranarray(Xo))
    # A device-resident engine may come from an earlier run: its weights, Grams and block partition must be THIS run's.
    # set_weights(None) restores unit weights (and drops the resident Grams, which were X_b'R^-1 X_b); an explicit
    # partition left by the previous run is rebuilt as uniform blocks below.
    if invw is not None or getattr(engine, "_weighted", False):
        engine.set_weights(invw)               # x'R^-1 x, X_b'R^-1 X_b, X_b'R^-1 r on the device (GibbsMats with Rinv)
    if gblup:
        pass                                   # (no Grams: the session opens below, once the state exists)
    elif explicit_partition is not None:
        engine.setup_blocks_explicit(explicit_partition, gram_mode)
    elif devres and invw is None and engine.block_size and getattr(engine, "_explicit_starts", None) is None:
        resident = set(engine.resident_block_sizes())
        if block_size not in resident:
            engine.add_block_size(block_size, gram_mode)
        if (adaptive or adaptive_mt) and (1024 if adaptive else 512) not in resident:
            engine.add_block_size(1024 if adaptive else 512, gram_mode)
        if mt_1024 and 1024 not in resident:
            engine.add_block_size(1024, gram_mode)
        engine.select_block_size(block_size)
    else:
        engine.setup_blocks(block_size, gram_mode)
        if adaptive or adaptive_mt:
            engine.add_block_size(1024 if adaptive else 512, gram_mode)
        if mt_1024:
            engine.add_block_size(1024, gram_mode)
    if group_m:            # grouped launches on the large block size of the adaptive policy (setup work, once)
        if engine.blocks_per_launch(1024) != group_m:
            cur_bs = engine.block_size
            engine.select_block_size(1024)
            try:
                engine.setup_groups(group_m, gram_mode)
            except Exception as ex:      # noqa: BLE001  (no HBM left for the group cross-Grams on an injected engine, an unsupported storage, ...)
                print(f"NOTICE: grouped launches not set up ({ex}); the chain runs one block per launch.")
                group_m = 0
            engine.select_block_size(cur_bs)
    if pair_m and engine.blocks_per_launch(512) != pair_m:
        cur_bs = engine.block_size
        engine.select_block_size(512)
        try:
            engine.setup_groups(pair_m, gram_mode)
        except Exception as ex:      # noqa: BLE001
            print(f"NOTICE: ping-pong pairs not set up ({ex}); the 512-marker sweeps run one block per launch.")
            pair_m = 0
        engine.select_block_size(cur_bs)
    engine.init_state(("MTBayesC" if gblup else mt_method) if t > 1 else method, t)
    if gblup:
        engine.gblup_begin(gb.D)

    # ---- location parameters: the terms go to the device (csrc/locpar.hpp) or the host builds its dense design matrices
    if lp_device:
        engine.locpar_begin(t)
        for g_, re_ in enumerate(rnd):                                   # the structure goes up before the effect's members are added
            if re_.randomType in ("A", "V"):
                engine.locpar_set_group_structure(g_, re_.Vinv.indptr, re_.Vinv.indices, re_.Vinv.data)
        for k in range(t):                                               # trait by trait, term by term: the reference's equation order
            for nm, kind_, val in lp_terms[k]:
                if kind_ == "covariate":
                    engine.locpar_add_covariate(k, val)
                else:
                    grp = [g_ for g_, re_ in enumerate(rnd) if re_.name == nm and k in re_.traits]
                    engine.locpar_add_factor(k, val[0], val[1], grp[0] if grp else -1)
        if mt_device:
            engine.mtmiss_begin((observed.astype(np.int64) @ (1 << np.arange(t))).astype(np.int32))      # mme.missingPattern (residual.jl:17-21)
        Xf = None
    else:
        Xf, labels = _design(model, ph, idcol)
    sol = np.zeros(sum(q))
    off = np.cumsum([0] + q)

    # ---- starting state (MCMC_BayesianAlphabet.jl:85-147)
    alpha0 = np.zeros((t, p), dtype=ftype)
    if Mi.alpha is not False:
        alpha0[:] = np.asarray(Mi.alpha, dtype=ftype).reshape(t, p)
    thresholds = {}
    if has_liab:
        # categorical_censored_traits_setup! (categorical_and_censored_trait.jl:29-95): thresholds, bounds and the set-up draw of
        # the liabilities; the liabilities live on the device beside the residual
        R0_ = np.atleast_2d(np.asarray(R.val, dtype=np.float64))
        engine.liability_begin(t)
        for k in liab_traits:
            if k in liab_codes:
                ncat = int(liab_codes[k].max())
                if traits_type[k] == "categorical(binary)":
                    th = [-np.inf, 0.0, np.inf]                           # :65
                elif t == 1:                                             # :58  (t1 = 0 < t2 < ... < 1)
                    th = [-np.inf] + list(np.linspace(0.0, 1.0, ncat)[:-1]) + [np.inf]
                else:                                                    # :60-62  (t1 = 0, t2 = 1 < t3 < ... < mu + 10 sigma, mu = 0)
                    th = [-np.inf, 0.0] + list(np.linspace(1.0, 10.0 * R0_[k, k], ncat - 1)[:-1]) + [np.inf]
                thresholds[k] = np.asarray(th, dtype=np.float64)
                engine.set_categorical(k, liab_codes[k], thresholds[k])
            else:
                engine.set_censored(k, liab_bounds[k][0], liab_bounds[k][1])
        model.thresholds = thresholds
    for k in range(t):
        engine.set_state(k, alpha=alpha0[k], beta=alpha0[k],
                         delta=np.ones(p, dtype=np.int32 if method == "BayesR" else ftype))
        # sol = 0; a liability trait starts from the placeholder phenotype the engine holds (its residual is y - cmean for THAT y)
        engine.set_residual(engine.liabilities(k).astype(ftype) if k in liab_traits else Y[k], k)
        if alpha0[k].any():
            engine.sub_xalpha(k)
    if has_liab:
        engine.liability_init(seed=seed_int, R=R0_)                       # :82-88
    ann_open = False
    if ann_device:                                                      # the session starts from annotations.py's start values
        with np.errstate(divide="ignore"):
            start_ = np.log(ann.snp_pi) if t > 1 else (ann.snp_pi if method == "BayesR" else np.asarray(pi, dtype=np.float64))
        engine.annot_begin(ann_kind, ann.design_matrix, ann.coefficients, ann.variance, start_)
        ann_open = True
    sem_open = False
    if sem:
        # SEM_setup (SEM.jl:53-62): the coefficients start at 0, so the residual just set IS the reference's "Lambda ycorr"
        sem_cs = np.asarray(causal_structure, dtype=np.int32)
        sem_edges = [(i, j) for i in range(t) for j in range(i) if sem_cs[i, j]]
        engine.sem_begin(Y.astype(np.float64), sem_cs)
        sem_open = True
        sem_lam = np.zeros((t, t))
        run_lam = Running(sem_lam)

    vare = ftype(R.val) if t == 1 else np.asarray(R.val, dtype=ftype)
    Gval = ftype(Mi.G.val) if t == 1 else np.asarray(Mi.G.val, dtype=ftype)
    if lasso:                                                           # MCMC_BayesianAlphabet.jl:70-81
        Gval = ftype(Gval / 8)
        Mi.G.scale = Mi.G.scale / 8
        gamma_l = rng.gamma(1.0, 8.0, size=p)
        Gvec = (np.float64(Gval) * gamma_l).astype(ftype)
    elif mt_pervar:
        Gmat = np.tile(np.asarray(Gval, dtype=ftype), (p, 1, 1))   # MCMC_BayesianAlphabet.jl:67-69 (fill(G, nMarkers))
    elif method == "BayesB":
        Gvec = np.full(p, Gval, dtype=ftype)                       # MCMC_BayesianAlphabet.jl:67-69
    pervar = method == "BayesB" and not lasso                           # per-marker variances, no common variance to report
    if t == 1 and method in ("BayesC", "BayesB") and np.ndim(pi) == 0:
        pi = float(pi)
    if lp_device:
        pass
    elif t > 1:
        lhs_blocks = [[Xf[k].T @ (w64[:, None] * Xf[l]) for l in range(t)] for k in range(t)]    # X'RiX, Ri = kron(R^-1, diag(w))
    else:
        lhs = Xf[0].T @ (w64[:, None] * Xf[0])                          # X'R^-1 X (build_MME.jl:339)

    def _gi64(re_):
        return np.asarray(re_.Gi.val, dtype=np.float64)

    # ---- accumulators and sample files (output.jl:320-437)
    run_sol, run_vare = Running(sol), Running(vare)
    run_varg = Running(Gval) if not pervar else None
    run_pi = Running(np.atleast_1d(np.asarray(pi_t if mega else pi, dtype=np.float64))) if Mi.estimatePi else None
    ebv_run = [Running(np.zeros(len(out_ids))) for _ in range(t)] if outputEBV else None
    run_scale = Running(np.atleast_1d(np.float64(Mi.G.scale))) if (Mi.G.estimate_scale and t == 1) else None
    name = Mi.name
    cov = [f"{a}_{b}" for a in model.lhsVec for b in model.lhsVec] if t > 1 else [model.lhsVec[0]]
    term_cols = term_sample_columns(model, labels, off)
    write_marker_samples = output_samples_for_all_parameters or p <= 20000
    rnd_keys = ["polygenic_effects_variance" if re_.randomType == "A" else "_".join(re_.term_array) + "_variances" for re_ in rnd]
    rnd_cov = [[f"{a}_{b}" for a in re_.term_array for b in re_.term_array] for re_ in rnd]
    run_rnd = [Running(np.zeros(len(names_))) for names_ in rnd_cov]
    genvar, bin_writers = None, {}
    files = SampleFiles(output_folder)
    lp_utu = None
    # EBV = genomic + polygenic part (prediction_setup, output.jl:29-36): entry of sol of every output ID in the pedigree term of trait k
    ped_cols = {}
    if outputEBV:
        for re_ in rnd:
            if re_.randomType == "A":
                lev_ = np.array([ped.index[i] for i in out_ids], dtype=np.int64)
                for k in re_.traits:
                    ped_cols[k] = off[k] + next(i for i, (_, eff, _) in enumerate(labels[k]) if eff == re_.name) + lev_
    # single-step EBV = Mout alpha + J_out sol[J] + Zo sol[ϵ] (getEBV over mme.output_X, output.jl:281-306; SSBR.jl:39-47): per trait the
    # (columns of sol, coefficients) of every output ID
    ss_cols = {}
    if outputEBV and single_step is not None:
        for k in range(t):
            for trm, cols_, coef_ in single_step.ebv_terms(labels[k]):
                ss_cols.setdefault(k, []).append((off[k] + cols_, coef_))
    t_sweep = 0.0
    iter_end = []                                # perf_counter at the end of every iteration (each ends synchronised with the device)
    # an exception inside the chain: the open sessions go with the files
    ends = ([engine.sem_end] if sem_open else []) + ([engine.annot_end] if ann_open else []) + ([engine.gblup_end] if gblup else [])
    t0 = time.time()
    # ================================ the chain =================================================
    with host_blas_limit(), files, _on_error(*ends):
        files.open("residual_variance", cov)                            # output.jl:320-437
        if not pervar:
            files.open(f"marker_effects_variances_{name}", cov if t > 1 else ["1"])
        if Mi.estimatePi and (np.size(pi) <= 20000 or output_samples_for_all_parameters):   # (marker-level pi: p values per sample)
            npi = t if mega else np.size(pi)
            files.open(f"pi_{name}", [f"pi{i + 1}" for i in range(npi)] if npi > 1 else ["pi"])
        for key_, (_, header) in term_cols.items():
            files.open(key_, header)
        # every saved sample goes to a binary file of sparse records -- the nonzero effects compacted on the device (samples.py);
        # the text row of p values (output.jl:467) only for small p or on request
        for kind_ in ("", "indirect_", "overall_") if sem else ("",):   # SEM.jl:187-316 (the reference's files name the term "genotypes")
            bin_writers[kind_] = [files.marker_writer(f"{kind_}marker_effects_{name}_{tr}", Mi.markerID) for tr in model.lhsVec]
            if write_marker_samples:
                for tr in model.lhsVec:
                    files.open(f"{kind_}marker_effects_{name}_{tr}", Mi.markerID)
        if sem:      # (the reference writes this file to the working directory, SEM.jl:59-60; here it lives with the other samples)
            files.open_bare("structure_coefficient", "structure_coefficient_MCMC_samples.txt")
        for key_, names_ in zip(rnd_keys, rnd_cov):                     # output.jl:348-351,401-405; the polygenic effect: :326-327,416-420
            files.open(key_, names_)
        for k in liab_traits:                                           # output.jl:367-372 (no header lines, as there)
            files.open_bare(f"liabilities_{model.lhsVec[k]}")
            if k in thresholds:
                files.open_bare(f"threshold_{model.lhsVec[k]}")
        if outputEBV and output_heritability and single_step is None:   # output.jl:358-362,426-432 (not in a single-step analysis: :196,358,426,498)
            genvar = GeneticVarianceSamples(files, cov, list(model.lhsVec))
        for it in range(1, chain_length + 1):
            # 0. categorical and censored traits (MCMC_BayesianAlphabet.jl:186-191): liabilities and residuals on the device,
            #    then the thresholds of the traits with more than two categories from the chain's rng
            if has_liab:
                engine.liability_sample(iteration=it, seed=seed_int, ngibbs=ngibbs, R=np.atleast_2d(np.asarray(vare, dtype=np.float64)))
                for k in liab_traits:
                    if traits_type[k] != "categorical":
                        continue
                    mx, mn = engine.liability_minmax(k)                  # categorical_and_censored_trait.jl:152-155
                    for i in range(2 if t == 1 else 3, len(thresholds[k]) - 1):
                        thresholds[k][i] = rng.uniform(mx[i], mn[i])
                    engine.set_thresholds(k, thresholds[k])              # :160

            # 1. location parameters: on the device (solver.jl:143-162 term by term, csrc/locpar.hpp) ...
            if mt_device:
                # sampleMissingResiduals (residual.jl:51-73) on the device, then the per-record Ri of mkRi / getRi until the first
                # residual-variance draw and kron(inv(R), diag(w)) afterwards (MCMC_BayesianAlphabet.jl:357-361): the host path's switch
                mt_B, mt_U, mt_C = missing_pattern_tables(np.asarray(vare, dtype=np.float64))
                engine.mtmiss_impute(iteration=it, seed=seed_int, B=mt_B, U=mt_U)
                engine.mtmiss_set_record_weights(mt_C if (it == 1 or not R.estimate_variance) else None)
            if lp_device:
                if sum(q):
                    if t == 1:
                        lp_st = engine.locpar_step(iteration=it, seed=seed_int, vare=float(vare), Gi=[_gi64(re_) for re_ in rnd])
                    else:
                        Rinv_ = np.linalg.inv(np.asarray(vare, dtype=np.float64))
                        lp_st = engine.locpar_step(iteration=it, seed=seed_int, Rinv=(Rinv_ + Rinv_.T) / 2, Gi=[_gi64(re_) for re_ in rnd])
                    lp_utu = lp_st["utu"]
            # ... or on the host
            elif sum(q):
                if t == 1:
                    host_location_step(engine, Xf[0], lhs, sol, w64, rng, vare, ftype)
                else:
                    R0 = np.asarray(vare, dtype=np.float64)
                    Rinv = np.linalg.inv(R0)
                    res = [engine.get_residual(k).astype(np.float64) for k in range(t)]
                    Ri_rows = _impute_missing_residuals(res, observed, R0, rng) if has_missing else None
                    if has_missing and (it == 1 or not R.estimate_variance):
                        # Residuals of the missing records are imputed from the observed ones every iteration
                        # (sampleMissingResiduals, residual.jl:52-73).  The location-parameter equations weight every record
                        # with the inverse of the OBSERVED block of R only (mkRi / getRi, residual.jl:2-44) -- but only until
                        # the first residual-variance draw: the reference then replaces Ri by kron(inv(R), diag(invweights))
                        # (MCMC_BayesianAlphabet.jl:357-361) and runs plain data augmentation on the imputed residuals.
                        if invw is not None:
                            Ri_rows = Ri_rows * w64[:, None, None]
                        rr = [res[k] + Xf[k] @ sol[off[k]:off[k + 1]] for k in range(t)]
                        A = np.block([[Xf[k].T @ (Ri_rows[:, k, l][:, None] * Xf[l]) for l in range(t)] for k in range(t)])
                        b = np.concatenate([Xf[k].T @ sum(Ri_rows[:, k, l] * rr[l] for l in range(t)) for k in range(t)])
                    else:
                        rr = [res[k] + Xf[k] @ sol[off[k]:off[k + 1]] for k in range(t)]
                        A = np.block([[Rinv[k, l] * lhs_blocks[k][l] for l in range(t)] for k in range(t)])
                        b = np.concatenate([Xf[k].T @ (w64 * sum(Rinv[k, l] * rr[l] for l in range(t))) for k in range(t)])
                    _gibbs(A, sol, b, rng, None)
                    for k in range(t):
                        engine.set_residual((rr[k] - Xf[k] @ sol[off[k]:off[k + 1]]).astype(ftype), k)

            elif t > 1 and has_missing:                                       # no location parameters: imputation only
                res = [engine.get_residual(k).astype(np.float64) for k in range(t)]
                _impute_missing_residuals(res, observed, np.asarray(vare, dtype=np.float64), rng)
                for k in range(t):
                    engine.set_residual(res[k].astype(ftype), k)

            # 2. marker effects (DEVICE)
            kw = dict(iteration=it, seed=seed_int, vare=vare, nreps=nreps)
            if independent_blocks:
                kw["independent_blocks"] = True
            if solve_policy.use(it) and engine.block_size == 256:
                kw["section_solve"] = True
            if mega:
                kw.update(var_effect=Gval, pi=pi_t)
                if mt_pervar:
                    kw["var_effect_matrix"] = Gmat
            elif ann_device:                                                # the prior table of the annotation session, resident on the device
                kw.update(var_effect=Gval, resident_priors=True)
                if method == "BayesR" and fast_blocks is not False:         # bayesr_block_nreps (BayesR.jl:22-25)
                    kw["nreps"] = 1 if it <= burnin else nreps
            elif t > 1:
                with np.errstate(divide="ignore"):
                    kw.update(var_effect=Gval, log_prior_states=np.log(ann.snp_pi if ann is not False else np.asarray(pi, dtype=np.float64)))
                if mt_pervar:
                    kw["var_effect_matrix"] = Gmat
            elif method == "BayesR":
                kw.update(var_effect=Gval, pi_classes=np.asarray(pi, dtype=np.float64))
                if ann is not False:
                    kw["pi_matrix"] = ann.snp_pi                            # per-marker class priors (BayesR.jl:62-66)
                if fast_blocks is not False:                                # bayesr_block_nreps (BayesR.jl:22-25)
                    kw["nreps"] = 1 if it <= burnin else nreps
            elif method == "BayesB":
                kw.update(var_effect=Gval, var_effect_vec=Gvec, pi=pi)
            elif np.ndim(pi) == 1:                                          # marker-level pi (bayesabc_pi_vector, BayesABC.jl:16-22)
                kw.update(var_effect=Gval, pi_vec=pi)
            else:
                kw.update(var_effect=Gval, pi=pi)
            if (group_m or pair_m) and engine.blocks_per_launch() >= 2:
                kw["group_launch"] = True
            if gblup:                                                       # GBLUP! / megaGBLUP! / MTGBLUP! (MCMC_BayesianAlphabet.jl:280-289)
                st = _gb.step(engine, iteration=it, seed=seed_int, vare=vare, G=Gval, t=t, diagonal=mega)
            else:
                st = engine.sweep(**kw)
            solve_policy.observe(it, engine, ran=bool(kw.get("section_solve")))
            t_sweep += st["sweep_ms"]
            if adaptive:
                engine.select_block_size(pick_block_size(st["n_events"], p, pairs=bool(pair_m)))
            elif adaptive_mt:
                engine.select_block_size(pick_block_size_mt(st["n_events"], p, allow_1024=mt_1024))
            elif adaptive_mts:
                engine.select_block_size(1024 if st["n_events"] < MT_1024_CHANGE_FRACTION * p else 512)

            # 3. pi (Pi.jl:7-42)
            if Mi.estimatePi:
                if mega:                                                    # MCMC_BayesianAlphabet.jl:300-301
                    pi_t = np.array([rng.beta(p - st["sum_delta"][k] + 1.0, st["sum_delta"][k] + 1.0) for k in range(t)])
                elif ann_device:                                            # the same update on the device (csrc/annot.hpp)
                    res_ = engine.annot_step(iteration=it, seed=seed_int, variance=ann.variance)
                    ann.coefficients[...] = res_["coefficients"]
                    if ann.design_matrix.shape[1] > 1:                      # the shrinkage variances stay on the chain's rng (annotation_updates.jl:125-137)
                        if ann.nsteps == 1:
                            ann.variance = A_.sample_effect_variance(ann.coefficients, rng)
                        else:
                            for s_ in range(ann.nsteps):
                                if res_["n_active"][s_] > 0:
                                    ann.variance[s_] = A_.sample_effect_variance(ann.coefficients[:, s_], rng)
                    if ann.nsteps > 1:
                        pi = res_["means"]
                elif t > 1 and ann is not False:                            # annotation_updates.jl:353-361
                    pi = A_.update_bayesc_mt_tree_priors(ann, engine.get_state(0)[2], engine.get_state(1)[2], rng)
                elif t > 1:
                    pi = rng.dirichlet(st["state_counts"] + 1.0)
                elif ann is not False:                                      # update_marker_annotation_priors! (annotation_updates.jl:328-351)
                    dlt = engine.get_state(0)[2]
                    pi = A_.update_bayesr_nested_priors(ann, dlt, rng) if method == "BayesR" else A_.update_bayesc_binary_priors(ann, dlt, rng)
                elif method == "BayesR":
                    pi = rng.dirichlet(st["class_counts"] + 1.0)
                else:
                    pi = float(rng.beta(p - st["sum_delta"][0] + 1.0, st["sum_delta"][0] + 1.0))

            # 4. marker effect variance (variance_components.jl:151-189), re-cast to Float32 (:323-325)
            if Mi.G.estimate_variance and gblup:                           # invweights = 1 ./ D, nloci = nObs (variance_components.jl:153-176)
                Gval = _gb.draw_genetic_variance(rng, st["alpha_ss"], n, Gdf, Mi.G.scale, t, mega, ftype)
            elif Mi.G.estimate_variance:
                if mega and mt_pervar:                                     # one scaled inverse chi-square per marker and trait
                    sc = np.diag(Gdf * np.diag(np.asarray(Mi.G.scale, dtype=np.float64)))      # (variance_components.jl:112-117,181-186)
                    if hasattr(engine, "sample_marker_covariances"):        # on the device, from the resident beta
                        engine.sample_marker_covariances(Gdf + 1.0, sc, seed=seed_int, iteration=it)
                        Gmat = None
                    else:
                        B = np.stack([engine.get_state(k)[1] for k in range(t)], axis=1).astype(np.float64)
                        Gmat = np.zeros((p, t, t), dtype=ftype)
                        for k in range(t):
                            Gmat[:, k, k] = (B[:, k] ** 2 + sc[k, k]) / rng.chisquare(Gdf + 1.0, size=p)
                elif mega:                                                  # diagonal only (variance_components.jl:104-109)
                    Gval = np.diag([(st["beta_ss"][k, k] + Gdf * Mi.G.scale[k, k]) / rng.chisquare(p + Gdf) for k in range(t)]).astype(ftype)
                elif mt_pervar:                                             # variance_components.jl:181-186: one draw per marker,
                    if hasattr(engine, "sample_marker_covariances"):        # IW(df + 1, scale + b_j b_j') -- on the device, from the
                        # resident beta (jwas_hip_sample_marker_covariances: Bartlett on the counter RNG); the next sweep uses them in place
                        engine.sample_marker_covariances(Gdf + 1.0, np.asarray(Mi.G.scale, dtype=np.float64), seed=seed_int, iteration=it)
                        Gmat = None
                    else:
                        B = np.stack([engine.get_state(k)[1] for k in range(t)], axis=1).astype(np.float64)
                        Gmat = _inverse_wishart_batch(rng, Gdf + 1.0, np.asarray(Mi.G.scale, dtype=np.float64)[None] + B[:, :, None] * B[:, None, :]).astype(ftype)
                elif t > 1:
                    from scipy.stats import invwishart
                    S = np.asarray(Mi.G.scale, dtype=np.float64) + st["beta_ss"]
                    Gval = np.asarray(invwishart.rvs(df=Gdf + p, scale=(S + S.T) / 2, random_state=rng), dtype=ftype).reshape(t, t)
                elif method == "BayesR":
                    Gval = ftype((st["bayesr_ssq"] + Gdf * Mi.G.scale) / rng.chisquare(st["bayesr_nnz"] + Gdf))
                elif lasso:                                                 # variance_components.jl:152-166,191-203
                    a64 = engine.get_state(0)[0].astype(np.float64)
                    Gval = ftype((np.dot(a64 / gamma_l, a64) + Gdf * Mi.G.scale) / rng.chisquare(p + Gdf))
                    Q = a64 * a64 / np.float64(Gval)
                    cand = 1.0 / rng.gamma(0.5, 4.0, size=p)
                    with np.errstate(over="ignore"):
                        accept = rng.random(p) < np.exp(Q / 4.0 * (2.0 / gamma_l - cand))
                    gamma_l[accept] = 2.0 / cand[accept]
                    Gvec = (np.float64(Gval) * gamma_l).astype(ftype)
                elif method == "BayesB":
                    beta = engine.get_state(0)[1].astype(np.float64)
                    Gvec = ((beta * beta + Gdf * Mi.G.scale) / rng.chisquare(1.0 + Gdf, size=p)).astype(ftype)
                else:
                    Gval = ftype((ftype(st["alpha_ss"][0, 0]) + Gdf * Mi.G.scale) / rng.chisquare(st["sum_delta"][0] + Gdf))

            # 4b. scale of the marker-effect variance prior (MCMC_BayesianAlphabet.jl:328-336; single trait only there too)
            if Mi.G.estimate_scale and t == 1:
                gv = Gvec.astype(np.float64) if pervar else np.atleast_1d(np.float64(Gval))
                Mi.G.scale = float(rng.gamma(gv.size * Gdf / 2 + 1, 1.0 / (np.sum(Gdf / (2 * gv)) + 1)))

            # 4c. variances of the random effects (sampleVCs, variance_components.jl:115-147; MCMC_BayesianAlphabet.jl:347-351):
            #     G0 ~ InvWishart(df + q, scale + U'U) from the cross-products the device returned with step 1
            for g_, re_ in enumerate(rnd):
                if re_.Gi.estimate_variance:
                    nlev_ = next(val[1] for nm, kd, val in lp_terms[re_.traits[0]] if nm == re_.name)
                    S_ = np.asarray(re_.Gi.scale, dtype=np.float64) + lp_utu[g_]
                    G0_ = _inverse_wishart_batch(rng, float(re_.Gi.df) + nlev_, ((S_ + S_.T) / 2)[None])[0]
                    Gi_ = np.linalg.inv(G0_.astype(ftype))               # Float32.(G0) unless double_precision (:138-140)
                    re_.Gi.val = (Gi_ + Gi_.T) / 2

            # 5. residual variance (variance_components.jl:60-66,82-112), re-cast to Float32 (:368-370)
            if R.estimate_variance:
                if t > 1 and R.constraint:                                  # variance_components.jl:104-109
                    vare = np.diag([(st["resid_ss"][k, k] + Rdf * R.scale[k, k]) / rng.chisquare(n + Rdf) for k in range(t)]).astype(ftype)
                elif t > 1 and binary_index:                                # variance_components.jl:100-104
                    S = np.asarray(R.scale, dtype=np.float64) + st["resid_ss"]
                    vare = sample_from_conditional_inverse_wishart(rng, Rdf + n, np.linalg.inv((S + S.T) / 2), binary_index).astype(ftype)
                elif t > 1:
                    from scipy.stats import invwishart
                    S = np.asarray(R.scale, dtype=np.float64) + st["resid_ss"]
                    vare = np.asarray(invwishart.rvs(df=Rdf + n, scale=(S + S.T) / 2, random_state=rng), dtype=ftype).reshape(t, t)
                elif traits_type[0] in ("categorical", "categorical(binary)"):
                    pass                                                    # fixed (MCMC_BayesianAlphabet.jl:363)
                else:
                    vare = ftype((ftype(st["resid_ss"][0, 0]) + Rdf * R.scale) / rng.chisquare(n + Rdf))

            # 5b. causal relationships among the phenotypes (MCMC_BayesianAlphabet.jl:372-377; get_Λ, SEM.jl:124-165): on the device
            #     from the resident residual, which moves to the new coefficients in place; only diag(R) is read (SEM.jl:129)
            if sem:
                sem_lam = engine.sem_step(iteration=it, seed=seed_int, R_diag=np.diag(np.asarray(vare, dtype=np.float64)))["lambda"]

            # 6. save (MCMC_BayesianAlphabet.jl:399-413, output.jl:443-604)
            if it > burnin and (it - burnin) % output_samples_frequency == 0:
                k = (it - burnin) / output_samples_frequency
                if lp_device:
                    engine.locpar_accumulate(k)                             # (running means on the device, read once at the end)
                    if term_cols or ped_cols or ss_cols:
                        sol = engine.locpar_get_sol()
                else:
                    run_sol.add(sol, k)
                for g_, re_ in enumerate(rnd):                              # output.jl:449-452
                    Gv_ = np.linalg.inv(_gi64(re_)).ravel()
                    run_rnd[g_].add(Gv_, k)
                    files.row(rnd_keys[g_], Gv_)
                run_vare.add(vare, k)
                if run_varg is not None:
                    run_varg.add(Gval, k)
                pi_marker_dev = ann_device and ann.nsteps == 1                # annotated BayesC on the device: the p values stay there
                if pi_marker_dev:
                    engine.annot_accumulate(k)
                elif run_pi is not None:
                    run_pi.add(np.atleast_1d(pi_t if mega else pi), k)
                engine.accumulate(k)
                if run_scale is not None:
                    run_scale.add(np.atleast_1d(np.float64(Mi.G.scale)), k)
                if ann is not False:
                    A_.accumulate(ann, k)
                for key_, (cols, _) in term_cols.items():
                    files.row(key_, sol[cols])
                files.row("residual_variance", np.atleast_1d(vare).ravel())
                for kk in liab_traits:                                      # output.jl:514-523 (read from the device only here)
                    files.row(f"liabilities_{model.lhsVec[kk]}", engine.liabilities(kk))
                    if kk in thresholds:
                        files.row(f"threshold_{model.lhsVec[kk]}", thresholds[kk])
                if not pervar:
                    files.row(f"marker_effects_variances_{name}", np.atleast_1d(Gval).ravel())
                if Mi.estimatePi and f"pi_{name}" in files:
                    files.row(f"pi_{name}", engine.annot_prior() if pi_marker_dev else np.atleast_1d(pi_t if mega else pi))
                sem_direct = []
                for kk, tr in enumerate(model.lhsVec):
                    si, sv = sparse_effects(engine, kk)
                    bin_writers[""][kk].append(si, sv)
                    sem_direct.append((si, sv))
                    if write_marker_samples:                                # run_chain: nine digits also under double_precision
                        files.sparse_effects_row(f"marker_effects_{name}_{tr}", si, sv, p, ftype, "%.9g")
                if sem:
                    # compute_indirect_effect (SEM.jl:245-252): K = sum_m Lambda^m; the device keeps the running means of K alpha and
                    # alpha + K alpha, the host forms this sample's rows from the sparse direct effects it has just read
                    sem_K = indirect_matrix(sem_lam)
                    engine.sem_accumulate(sem_K, k)
                    run_lam.add(sem_lam, k)
                    files.row("structure_coefficient", sem_lam.ravel(order="F"))      # vec(Λ), MCMC_BayesianAlphabet.jl:410-412
                    u_idx, ind_, ov_ = indirect_overall_rows(sem_K, sem_direct)
                    for kind_, rows_ in (("indirect_", ind_), ("overall_", ov_)):
                        for kk, tr in enumerate(model.lhsVec):
                            nz_ = rows_[kk] != 0.0
                            bin_writers[kind_][kk].append(u_idx[nz_], rows_[kk][nz_])
                            if write_marker_samples:
                                files.sparse_effects_row(f"{kind_}marker_effects_{name}_{tr}", u_idx, rows_[kk], p, ftype, "%.9g")
                if outputEBV:
                    if X_out_host is not None:
                        ebvs = [(X_out_host @ engine.get_state(kk)[0].astype(np.float64)).astype(ftype) for kk in range(t)]
                    elif plink_out and hasattr(engine, "ebv_output"):      # all traits in one launch on the packed output rows
                        ebvs = list(engine.ebv_output())
                    else:
                        ebvs = [engine.mul_alpha(kk) if out_same else engine.mul_alpha_output(kk) for kk in range(t)]   # getEBV, output.jl:281-306
                    for kk, cols_ in ped_cols.items():                      # the polygenic part of this sample, added on the host
                        ebvs[kk] = (np.asarray(ebvs[kk], dtype=np.float64) + sol[cols_]).astype(ftype)
                    for kk, parts_ in ss_cols.items():                      # the J and ϵ parts of this sample, added on the host
                        e_ = np.asarray(ebvs[kk], dtype=np.float64)
                        for cols_, coef_ in parts_:
                            e_ = e_ + coef_ * sol[cols_]
                        ebvs[kk] = e_.astype(ftype)
                    for kk in range(t):
                        ebv_run[kk].add(ebvs[kk], k)
                    if genvar is not None:                                  # output.jl:498-512 (the EBVs in the element type of the run)
                        genvar.add(ebvs, np.diag(np.atleast_2d(np.asarray(vare, dtype=np.float64))), diagonal_only=t > 1 and Mi.G.constraint)
            iter_end.append(time.perf_counter())
            if it % printout_frequency == 0 and it > burnin:
                print_posterior_means(it, run_vare.mean)
    wall = time.time() - t0
    if gblup:
        engine.gblup_end()
        _gb.rename_variance_file(output_folder, name)                    # MCMC_BayesianAlphabet.jl:434-439

    # ---- results (output.jl:108-212)
    if lp_device:
        lp_mean, lp_mean2 = engine.locpar_get_means() if sum(q) else (np.zeros(0), np.zeros(0))
        lp_sd = np.sqrt(np.abs(lp_mean2 - lp_mean ** 2))
        engine.locpar_end()
        if mt_device:
            engine.mtmiss_end()
    else:
        lp_mean, lp_sd = run_sol.mean, run_sol.sd()
    out = {"location parameters": location_table(labels, off, lp_mean, lp_sd), "residual variance": covariance_table(cov, run_vare)}
    for g_, re_ in enumerate(rnd):
        out["polygenic effects covariance matrix" if re_.randomType == "A" else rnd_keys[g_]] = covariance_table(rnd_cov[g_], run_rnd[g_])
    # run_chain: the SD from the moments cast to Float64 (the engine returns them in the element type of the run)
    out[f"marker effects {name}"] = marker_effects_table([(tr, Mi.markerID) + tuple(engine.posterior(k)) for k, tr in enumerate(model.lhsVec)],
                                                         sd_in_double=True)
    if sem_open:                                                         # generate_marker_effect (SEM.jl:318-368; JWAS.jl:496-507)
        write_tables({f"direct marker effects {name}": out[f"marker effects {name}"]}, output_folder)
        for kind_ in ("indirect", "overall"):                            # (the session's moments are doubles)
            out[f"{kind_} marker effects {name}"] = marker_effects_table(
                [(tr, Mi.markerID) + tuple(engine.sem_get_effects(kind_, k)) for k, tr in enumerate(model.lhsVec)], sd_in_double=False)
        import pandas as pd
        lam_sd = run_lam.sd()
        out["structure coefficients"] = pd.DataFrame({"Trait": [model.lhsVec[i] for i, _ in sem_edges], "Parent": [model.lhsVec[j] for _, j in sem_edges],
                                                      "Estimate": [run_lam.mean[i, j] for i, j in sem_edges], "SD": [lam_sd[i, j] for i, j in sem_edges]})
        engine.sem_end()
    if run_varg is not None:
        out[f"marker effects variance {name}"] = covariance_table(cov, run_varg)
    if ann_open:
        if ann.nsteps == 1:
            run_pi.mean, run_pi.mean2 = engine.annot_means()
        engine.annot_end()
    if run_pi is not None:
        if mega:
            lab = list(model.lhsVec)
        elif t == 1 and method != "BayesR" and np.size(run_pi.mean) > 1:
            lab = list(Mi.markerID)                                      # annotated BayesC: marker-level pi
        else:
            lab = pi_labels(t, method)
        out[f"pi_{name}"] = pi_table(run_pi, lab)
    if ann is not False:
        out[f"annotation coefficients {name}"] = A_.coefficients_table(ann, method)
    if run_scale is not None:                                            # output.jl:148-150
        out[f"ScaleEffectVar{name}"] = covariance_table([model.lhsVec[0]], run_scale)
    if outputEBV:
        out.update(ebv_tables(model.lhsVec, out_ids, ebv_run))
    if genvar is not None:                                               # output.jl:196-209 (mean and std of the samples)
        out.update(genvar.tables())
    write_tables(out, output_folder)
    out["_timing"] = {"wall_s": wall, "device_sweep_ms_total": t_sweep, "iterations": chain_length,
                      "block_size": block_size, "n": n, "p": p, "iteration_end_s": iter_end,
                      "block_starts": (np.asarray(engine.block_starts(), dtype=np.int64) + 1).tolist() if fast_blocks is not False else None,
                      "block_repetitions": int(nreps)}
    if has_liab:
        engine.liability_end()
    if own_engine and not devres:
        engine.close()
    return out
