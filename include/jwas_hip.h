/*
 * jwas_hip.h -- C ABI of libjwas_hip.so: the MI355X (gfx950) marker-effect Gibbs sweep.
 *
 * Drop-in boundary for ONE path of reworkhow/JWAS.jl (v2.3.6): the single-site marker-effect
 * update loop inside runMCMC and the genotype storage/access layer under it.  A host (the bundled
 * Python host in jwas.jl_amd/, or a Julia `ccall` shim -- see INTEGRATION.md) keeps
 * get_genotypes()/build_model()/runMCMC(); everything else (fixed effects, pedigree terms, variance
 * components, pi draws, output files) stays on the host and consumes only the O(n)+O(p)-reducible
 * statistics returned by jwas_hip_sweep().
 *
 * Reference interfaces replaced (paths relative to /root/reference/src/1.JWAS/src/):
 *   jwas_hip_load_dense_f32*   Genotypes.genotypes + GibbsMats column views
 *                              (types.jl:98-165, markers/tools4genotypes.jl:8-10,237-258)
 *   jwas_hip_setup_blocks      GibbsMats x'x and block Grams, get_column_blocks_ref
 *                              (markers/tools4genotypes.jl:28-36,80-88,259-267)
 *   jwas_hip_set/get_state     Genotypes.alpha/beta/delta (MCMC/MCMC_BayesianAlphabet.jl:85-117)
 *   jwas_hip_set/get_residual  the shared ycorr vector (MCMC/MCMC_BayesianAlphabet.jl:131-157)
 *   jwas_hip_residual_sub_xalpha   ycorr -= X*alpha0 (MCMC/MCMC_BayesianAlphabet.jl:137-146)
 *   jwas_hip_sweep             BayesABC!  (markers/BayesianAlphabet/BayesABC.jl:60-80,118-188)
 *                              BayesR!    (markers/BayesianAlphabet/BayesR.jl:45-97,111-193)
 *                              MTBayesABC! sampler I (markers/BayesianAlphabet/MTBayesABC.jl:57-127,243-333)
 *                              + the post-sweep reductions consumed by Pi.jl:7-17,20-42 and
 *                              variance_components.jl:60-112,151-189
 *   jwas_hip_accumulate        output_posterior_mean_variance, marker part (output.jl:568-577)
 *   jwas_hip_mul_alpha         getEBV's X*alpha (output.jl:281-306)
 *   jwas_hip_load_output_dense_f32 / jwas_hip_mul_alpha_output
 *                              Mi.output_genotypes (markers/tools4genotypes.jl:290-296) and getEBV over mme.output_ID
 *                              (output.jl:281-306; default output_ID = all genotyped individuals,
 *                              input_data_validation.jl:150-154)
 *   jwas_hip_window_sums       window genomic variances of a marker-effect sample (src/3.GWAS/src/GWAS.jl:152-165)
 *   jwas_hip_gwas_begin / _sample / _local_ebv / _end
 *                              the same over a resident session, plus the local EBVs (src/3.GWAS/src/GWAS.jl:149-173)
 *   jwas_hip_liability_*       sample_liabilities! and the threshold bounds of categorical / censored traits
 *                              (categorical_and_censored_trait/categorical_and_censored_trait.jl:29-210)
 *   jwas_hip_locpar_*          the non-marker location parameters: the single-site scan Gibbs(A, x, b[, vare])
 *                              (iterative_solver/solver.jl:143-162) of MCMC/MCMC_BayesianAlphabet.jl:193-220 in residual-update
 *                              form, and the cross-products sampleVCs reads (variance_components.jl:115-147)
 *   jwas_hip_mtmiss_*          multi-trait records that miss some traits: sampleMissingResiduals (residual.jl:51-73) and the
 *                              per-record Ri of mkRi / getRi (residual.jl:2-44) in the location-parameter step
 *   jwas_hip_annot_*           update_marker_annotation_priors!: the probit update of the annotation coefficients and the
 *                              per-marker prior table of annotated BayesC / BayesR / 2-trait BayesC
 *                              (MCMC/annotation_updates.jl:21-137,181-361)
 *   jwas_hip_sem_*             the structural coefficients of runMCMC(...; causal_structure): SEM_setup / get_Λ and the indirect and
 *                              overall marker effects (structure_equation_model/SEM.jl:53-165,245-252)
 *   jwas_hip_rrm_*             the marker sweep of runMCMC(...; RRM = Phi): BayesABCRRM!, get_mΦΦarray and the running means of
 *                              MCMC_BayesianAlphabet_RRM (RRM/RRM.jl:43-57,101-158; RRM/MCMC_BayesianAlphabet_RRM.jl:123-144,212-218)
 *   jwas_hip_mega_*            constraint = true with up to 64 traits: megaBayesABC! / megaBayesC0!, t independent single-trait
 *                              chains over one genotype matrix (markers/BayesianAlphabet/BayesABC.jl:1-58), and
 *                              sampleMissingResiduals under a diagonal R (residual.jl:51-73)
 *
 * Conventions: every entry point returns 0 on success and a negative JWAS_HIP_E* code on failure
 * (no exceptions cross the boundary; jwas_hip_last_error() returns the message -- the analogue of
 * the reference's error(...) strings).  All pointers are plain host pointers unless a parameter
 * name ends in _dev.  The context owns all device memory it allocates; host arrays are copied
 * during the call and never retained.  One host thread per context; calls are synchronous unless
 * stated.  The library never falls back to a CPU path.
 */
#ifndef JWAS_HIP_H
#define JWAS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jwas_hip_ctx jwas_hip_ctx;

enum {
    JWAS_HIP_OK        =  0,
    JWAS_HIP_EINVAL    = -1,   /* invalid argument (message says which; mirrors error(...) text) */
    JWAS_HIP_EHIP      = -2,   /* a HIP runtime call failed                                     */
    JWAS_HIP_ESTATE    = -3,   /* call order violated (e.g. sweep before setup_blocks)          */
    JWAS_HIP_EUNSUP    = -4,   /* combination not supported by the device path                  */
    JWAS_HIP_ENOMEM    = -5    /* memory guard / allocation failure                             */
};

/* Marker-effect samplers (Mi.method / multi_trait_sampler in the reference). */
enum {
    JWAS_HIP_BAYESC    = 0,    /* single-trait BayesC: one shared effect variance               */
    JWAS_HIP_BAYESB    = 1,    /* single-trait BayesB (BayesA = BayesB with pi = 0): per-marker  */
    JWAS_HIP_BAYESR    = 2,    /* single-trait BayesR, 4-class mixture                          */
    JWAS_HIP_MTBAYESC1 = 3,    /* multi-trait BayesC, Gibbs sampler I  (MTBayesABC.jl:57-127)    */
    JWAS_HIP_MTBAYESC2 = 4,    /* multi-trait BayesC, Gibbs sampler II (MTBayesABC.jl:129-210):  */
                               /* joint indicator state; candidate states in bitmask order       */
    JWAS_HIP_MEGABAYESC = 5,   /* megaBayesABC! (BayesABC.jl:1-8, G.constraint = true): t         */
                               /* independent single-trait BayesC chains sharing one pass over X */
    JWAS_HIP_MTBAYESB1 = 6,    /* multi-trait BayesA/B, Gibbs sampler I with ONE t x t effect      */
                               /* covariance PER MARKER (locus_effect_variances[marker],           */
                               /* MTBayesABC.jl:66,86-90; variance_components.jl:181-186):          */
                               /* jwas_sweep_params.var_effect_matrix, or drawn on the device by    */
                               /* jwas_hip_sample_marker_covariances                                 */
    JWAS_HIP_MTBAYESB2 = 7,    /* multi-trait BayesA/B under Gibbs sampler II (a Pi that lists fewer */
                               /* than 2^t states with multi_trait_sampler = :auto, MTBayesABC.jl:   */
                               /* 20-25,129-210 with Ginv[marker]); covariances as for MTBAYESB1     */
    JWAS_HIP_MEGABAYESB = 8    /* megaBayesABC! with BayesA/B (BayesABC.jl:1-8, G.constraint = true): */
                               /* t independent single-trait chains, trait k of marker j with        */
                               /* variance var_effect_matrix[j][k][k] (off-diagonals ignored);       */
                               /* jwas_hip_sample_marker_covariances then draws the diagonal only    */
};

/* Genotype storage kinds (Genotypes.storage_mode in the reference, types.jl:149-150). */
enum {
    JWAS_HIP_STORAGE_DENSE_F32  = 0,   /* storage=:dense, Float32 matrix                                 */
    JWAS_HIP_STORAGE_PACKED2BIT = 1    /* storage=:stream's 2-bit packed marker-major payload (.jgb2)   */
};

/* Gram precompute modes for jwas_hip_setup_blocks. */
enum {
    JWAS_HIP_GRAM_F64  = 0,    /* fp64-accumulated (bit-reproducible vs the CPU oracle); slow    */
    JWAS_HIP_GRAM_MFMA = 1     /* fp32 MFMA (v_mfma_f32_32x32x2_f32), fp64 chunk combine         */
};

#define JWAS_HIP_MAX_TRAITS 4
#define JWAS_HIP_MAX_STATES 16          /* 2^JWAS_HIP_MAX_TRAITS */

/* Parameters of one sweep = one call of BayesABC!/BayesR!/MTBayesABC! in the reference. */
typedef struct jwas_sweep_params {
    int32_t  method;                    /* JWAS_HIP_BAYESC ...                                       */
    int32_t  ntraits;                   /* 1, or t (2..4) for the multi-trait methods                */
    int32_t  nreps;                     /* within-block repetitions: 1 = exact non-block chain;      */
                                        /* <= 0 = block size (reference fast_blocks, BayesABC.jl:153) */
    uint32_t iteration;                 /* MCMC iteration index (enters the RNG counter)             */
    uint64_t seed;                      /* runMCMC(seed=...) (JWAS.jl:239-251)                       */
    uint32_t marker_offset;             /* global index of this context's column 0 (marker shards)   */
    uint32_t independent_blocks;        /* != 0: independent-block sweep (MCMCinfo.independent_blocks,   */
                                        /* BayesABC.jl:190-255): every block starts from the same        */
                                        /* residual snapshot; reconcile r += sum_b X_b*dalpha_b afterwards */
    float    vare[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];        /* residual (co)variance, row-major t x t */
    float    var_effect[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];  /* BayesC: sigma2_alpha; BayesR: sigmaSq; MT: t x t (MEGA: diagonal used) */
    double   pi;                        /* BayesC/B scalar Pr(effect = 0); ignored if pi_vec != NULL */
    double   pi_classes[4];             /* BayesR class priors; ignored if pi_matrix != NULL.        */
                                        /* MEGABAYESC: pi_classes[k] = Pr(effect = 0) of trait k     */
    double   gamma[4];                  /* BayesR class variances (JWAS.jl:12)                       */
    double   log_prior_states[JWAS_HIP_MAX_STATES];  /* MT: log pi(state), state = sum delta_k << k  */
    const float*  var_effect_vec;       /* BayesB: p per-marker variances (host), else NULL          */
    const double* pi_vec;               /* BayesC/B: p per-marker pi (host), else NULL               */
    const double* pi_matrix;            /* BayesR: p x 4 row-major per-marker class priors, else NULL */
    const double* log_prior_states_matrix;  /* MT samplers I/II: p x 2^t row-major per-marker log pi(state) (marker-specific */
                                        /* joint priors: the reference's annotated multi-trait BayesC, MarkerSpecificPiPrior, */
                                        /* MTBayesABC.jl:22-47), else NULL; needs 2 traits and a block size <= 512 */
    const float*  var_effect_matrix;    /* MTBAYESB1: p x t x t row-major per-marker effect covariances (host); inverted on the   */
                                        /* device once per sweep; needs block_size * ntraits <= 2048.  NULL = the covariances     */
                                        /* resident on the device (an earlier sweep's, or jwas_hip_sample_marker_covariances)     */
    /* Float64 contexts (jwas_hip_set_precision(ctx, 64); runMCMC(double_precision=true)) read these instead of vare /     */
    /* var_effect / var_effect_vec -- the same quantities as Float64, as the reference holds them in that mode:           */
    double   vare_f64[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];
    double   var_effect_f64[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];
    const double* var_effect_vec_f64;   /* BayesB: p per-marker variances (host), else NULL                                */
    int32_t  section_solve;             /* != 0: Rule T -- dense chains as triangular solves.  Multi-trait sampler I (shared or     */
                                        /* per-marker covariance, <= 3 traits) on FULL 256-marker blocks: a 64-marker section's     */
                                        /* chain (MTBayesABC.jl:243-333) is evaluated as D = T y with the section's inverse         */
                                        /* T = (I + L)^-1 formed once per sweep on the device, every marker then verified with the  */
                                        /* literal evaluation (MTBayesABC.jl:85-120); a marker that is not in the model for every   */
                                        /* trait before and after is an EXCEPTION -- its literal evaluation replaces its row of the */
                                        /* solution and the rows behind it are corrected, in marker order; sections with many       */
                                        /* exceptions run the sequential chain.  The same conditional means and draws, another      */
                                        /* association (effects within float32 rounding of the sequential chain).  Needs nreps = 1, */
                                        /* no independent_blocks, no marker-specific priors; every other sweep ignores the flag.    */
                                        /* 0 = the sequential chain everywhere (bit-identical to earlier releases).                 */
    int32_t  group_launch;              /* != 0: GROUPED LAUNCHES -- every launch streams the 2 or 4 consecutive blocks that         */
                                        /* jwas_hip_setup_groups prepared and samples the previous group's blocks in order: the     */
                                        /* same chain with the per-launch cost shared by the group; the block right-hand sides are  */
                                        /* assembled from an older residual plus up to three cross-Gram corrections (float32        */
                                        /* rounding of the plain schedule).  Single-trait methods, nreps = 1, uniform blocks, no     */
                                        /* independent_blocks; every other sweep, and a context without jwas_hip_setup_groups,      */
                                        /* ignores the flag.  0 = one block per launch (bit-identical to earlier releases).         */
} jwas_sweep_params;

/* Reductions the host-side conjugate draws need (Pi.jl, variance_components.jl). */
typedef struct jwas_sweep_stats {
    double  sum_delta[JWAS_HIP_MAX_TRAITS];          /* BayesC/B, MT: sum_j delta_jk (MCMC_BayesianAlphabet.jl:309)   */
    double  alpha_ss[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];   /* alpha'alpha (t x t; [0] single trait)           */
    double  beta_ss[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];    /* beta'beta  (variance_components.jl:175-177)     */
    double  resid_ss[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];   /* r_i'r_j    (variance_components.jl:60-66,82-98) */
    double  resid_sum[JWAS_HIP_MAX_TRAITS];          /* sum_i r_ik (intercept-only location update)                   */
    double  class_counts[4];                         /* BayesR: markers per class (Pi.jl:11-17)                       */
    double  bayesr_ssq;                              /* BayesR: sum_{delta>1} alpha^2/gamma_delta                     */
    double  bayesr_nnz;                              /* BayesR: #{delta > 1}                                          */
    double  state_counts[JWAS_HIP_MAX_STATES];       /* MT: markers per joint state (Pi.jl:20-42)                     */
    double  n_events;                                /* markers whose effect changed this sweep (diagnostic)          */
    double  sweep_ms;                                /* device time of the sweep (hipEvent), milliseconds             */
    double  update_kernel_ms;                        /* sum of the sampled k_block_step event intervals (ms)          */
    double  update_kernel_samples;                   /* number of launches timed (see jwas_hip_set_kernel_timing)     */
    double  update_kernel_bytes;                     /* algorithmic bytes (4*n*b) of the timed launches               */
    double  event_overhead_ms;                       /* HIP-event interval around an EMPTY launch (dispatch gap), ms  */
} jwas_sweep_stats;

/* ---- context ------------------------------------------------------------------------------- */
int  jwas_hip_create(int device, jwas_hip_ctx** out);
void jwas_hip_destroy(jwas_hip_ctx* ctx);
const char* jwas_hip_last_error(const jwas_hip_ctx* ctx);   /* ctx may be NULL: create() errors */
/* Launch all work on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int  jwas_hip_set_stream(jwas_hip_ctx* ctx, void* hip_stream);
int  jwas_hip_device_info(jwas_hip_ctx* ctx, int* n_cu, int64_t* hbm_bytes_total, int64_t* hbm_bytes_free);

/* ---- genotype storage ------------------------------------------------------------------------ */
/* Copy a column-major (marker-major) n x p fp32 matrix from the host; ld_host >= n is the host
 * column stride in elements (Julia Matrix{Float32} / numpy order='F': ld_host = n). */
int  jwas_hip_load_dense_f32(jwas_hip_ctx* ctx, const float* X_host, int64_t n, int64_t p, int64_t ld_host);
/* Allocate an uninitialised n x p device matrix (filled later by jwas_hip_synth_genotypes). */
int  jwas_hip_alloc_dense_f32(jwas_hip_ctx* ctx, int64_t n, int64_t p);
/* ---- 2-bit packed storage: the reference's Packed2BitBackend kept packed in HBM (16x fewer bytes than fp32) ----
 * Layout (streaming_genotypes.jl:364-367,622-627): marker-major, marker j at bytes [j*stride, (j+1)*stride),
 * stride >= cld(n,4); individual i in byte i>>2 at bit shift (i&3)<<1; codes 0/1/2 = genotype, 3 = missing.
 * Every kernel decodes on the fly exactly as decode_marker! (:978-1002): v = code==3 ? mean_j : Float32(code),
 * x = centered ? v - mean_j : v, so all results equal those of the dense path on the decoded matrix.
 * jwas_hip_load_jgb2 replaces load_streaming_backend (:884-971): `path` is the prefix, or <prefix>.meta / .jgb2;
 * it reads the tab-separated manifest (nObs, nMarkers, stride_bytes, centered, data_path, mean_path) and the
 * .mean.f32 sidecar.  x'x is recomputed on the device; a host that wants the .xpRinvx.f32 sidecar values instead
 * passes them to jwas_hip_set_xpx after jwas_hip_setup_blocks.
 * Pad fields: when n is no multiple of 4 the unused fields of a marker's last byte (individuals n .. 4*cld(n,4)-1) may hold
 * anything.  Both loaders copy the cld(n,4) bytes of a marker as they are and no kernel reads those fields: every accessor masks
 * the rows >= n (PackedCols::load1 / load4 / the update role's row mask), so decoded columns, inner products, X*alpha, window sums
 * and sweeps do not depend on them (tests/test_gpu_packed.py).  Only jwas_hip_get_packed2bit, which returns the bytes as loaded,
 * shows them.  Bytes of a host row beyond cld(n,4) (stride_bytes > cld(n,4)) are not copied. */
int  jwas_hip_load_jgb2(jwas_hip_ctx* ctx, const char* path);
int  jwas_hip_load_packed2bit(jwas_hip_ctx* ctx, const uint8_t* payload, int64_t n, int64_t p, int64_t stride_bytes,
                              const float* marker_means, int32_t centered);
int  jwas_hip_alloc_packed2bit(jwas_hip_ctx* ctx, int64_t n, int64_t p, int32_t centered);   /* + jwas_hip_synth_genotypes */
/* ---- PLINK 1 binary filesets (.bed/.bim/.fam) straight into packed storage ----
 * Replaces prepare_streaming_genotypes (streaming_genotypes.jl:499-656,819-877) for genotypes that exist as a variant-major .bed
 * file: the same four-individuals-per-byte layout as .jgb2, with another meaning of the 2-bit field (0 = homozygous for the .bim's
 * first allele A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2).  Two calls, so that the quality control (:274-296) stays in the
 * host's one copy of it:
 *   jwas_hip_plink_scan    checks the file (magic 6C 1B 01, size 3 + p_file * cld(n_file,4)) and `rows` (the file rows of the
 *                          individuals to keep, in the order wanted, each at most once; NULL: all n_file in file order), streams the
 *                          file through pinned buffers of at most 64 MB, transcodes EVERY file marker on the device into a staging
 *                          buffer of the context ([p_file][ld/4] bytes, pad fields 0) and returns counts[j][c] = kept individuals of
 *                          marker j with code c (0/1/2 = copies of the counted allele, A1 if count_a1 else A2; 3 = missing).
 *   jwas_hip_plink_commit  allocates packed storage (n_rows, p_sel) as jwas_hip_load_packed2bit does, moves the rows of the markers
 *                          `selected` (0-based file indices, strictly ascending) into it, sets their means and `centered`, and frees
 *                          the staging buffer.  When every marker stays the staging buffer becomes the storage.  Needs a pending
 *                          scan (JWAS_HIP_ESTATE otherwise).
 *   jwas_hip_plink_discard drops a pending scan; so do every other load / allocation of genotypes and jwas_hip_destroy.
 * Device memory between the two calls: the staging buffer beside whatever the context held before; during a commit that drops
 * markers: the staging buffer and the final storage.  Float32 contexts only. */
int  jwas_hip_plink_scan(jwas_hip_ctx* ctx, const char* bed_path, int64_t n_file, int64_t p_file, const int64_t* rows, int64_t n_rows,
                         int32_t count_a1, int64_t* counts);
int  jwas_hip_plink_commit(jwas_hip_ctx* ctx, const int64_t* selected, int64_t p_sel, const float* marker_means, int32_t centered);
int  jwas_hip_plink_discard(jwas_hip_ctx* ctx);
/* The packed rows of markers [j0, j0 + m) back to the host, cld(n,4) bytes of each at stride_bytes >= cld(n,4): the payload of a
 * .jgb2 file (streaming_genotypes.jl:600-654) from a context with packed storage, however it was loaded. */
int  jwas_hip_get_packed2bit(jwas_hip_ctx* ctx, int64_t j0, int64_t m, uint8_t* out_host, int64_t stride_bytes);
/* ---- output rows in 2-bit packed storage: EBVs for individuals outside the training set, kept packed ----
 * Mi.output_genotypes (tools4genotypes.jl:290-296) for the output_ID of check_outputID (input_data_validation.jl:143-196) as a SECOND
 * packed matrix [p][ld_out/4], ld_out = n_out rounded up to 256, beside the packed training storage of a Float32 context.  It has no
 * means of its own: a field is decoded with the training storage's marker mean and `centered` (decode_marker!,
 * streaming_genotypes.jl:978-1002), so a missing code of an output individual decodes to the training mean (0 when centred); rows
 * >= n_out decode to 0 whatever their fields hold.  At most one output matrix is resident: loading a packed one frees a dense one
 * (jwas_hip_load_output_dense_f32) and the reverse; a load of genotypes and jwas_hip_destroy free both; a GWAS session on output rows
 * is dropped.  jwas_hip_mul_alpha_output and jwas_hip_window_sums / _sums2 (use_output_rows) run on packed output rows;
 * jwas_hip_gwas_begin(use_output_rows) answers JWAS_HIP_EUNSUP on them.  JWAS_HIP_ESTATE without packed training storage,
 * JWAS_HIP_EUNSUP on a Float64 context.
 *   jwas_hip_load_output_packed2bit  from a host payload in the .jgb2 field layout (streaming_genotypes.jl:364-367,622-627): p rows of
 *                                    cld(n_out,4) bytes at stride_bytes.  JWAS_HIP_EINVAL when p differs from the context's.
 *   jwas_hip_plink_commit_output     after a jwas_hip_plink_scan whose `rows` are the output individuals and whose count_a1 is the
 *                                    training's: the staging rows of `selected` -- the TRAINING selection, p_sel = the context's p
 *                                    (JWAS_HIP_EINVAL otherwise); the output individuals' own allele counts play no part -- become the
 *                                    output rows.  Training storage, state and blocks are untouched.  The pending scan is consumed;
 *                                    an error leaves the earlier output rows in place.
 *   jwas_hip_get_output_packed2bit   the twin of jwas_hip_get_packed2bit: cld(n_out,4) bytes of the markers [j0, j0 + m). */
int  jwas_hip_load_output_packed2bit(jwas_hip_ctx* ctx, const uint8_t* payload, int64_t n_out, int64_t p, int64_t stride_bytes);
int  jwas_hip_plink_commit_output(jwas_hip_ctx* ctx, const int64_t* selected, int64_t p_sel);
int  jwas_hip_get_output_packed2bit(jwas_hip_ctx* ctx, int64_t j0, int64_t m, uint8_t* out_host, int64_t stride_bytes);
int  jwas_hip_storage_info(jwas_hip_ctx* ctx, int32_t* kind, int64_t* n, int64_t* p, int64_t* bytes);
/* Device row stride (elements) of the padded marker-major layout, and its base device pointer. */
int  jwas_hip_dense_layout(jwas_hip_ctx* ctx, int64_t* n, int64_t* p, int64_t* ld_dev, void** X_dev);
/* Copy columns [j0, j0+count) back to the host (column-major, ld = n). */
int  jwas_hip_get_columns(jwas_hip_ctx* ctx, int64_t j0, int64_t count, float* out_host);
/* Overwrite columns [j0, j0+count) of an allocated dense matrix from the host (column-major, column stride ld_host >= n):
 * a matrix that is produced in marker chunks -- impute_genotypes (single_step/SSBR.jl:112-135: 1000 markers at a time) --
 * goes to HBM chunk by chunk and never exists on the host as a whole.  Resident block configurations are dropped. */
int  jwas_hip_set_columns(jwas_hip_ctx* ctx, int64_t j0, int64_t count, const float* cols_host, int64_t ld_host);
/* Memory guard (tools4genotypes.jl:99-235 analogue for HBM): bytes the dense path needs (2 or 3 traits on 256-marker
 * blocks: incl. the per-sweep section inverses of jwas_sweep_params.section_solve, p * 64 * ntraits^2 * 4 bytes). */
int64_t jwas_hip_estimate_bytes(int64_t n, int64_t p, int32_t ntraits, int32_t block_size);
/* Same for a given storage kind (estimate_marker_memory(...; storage_mode), tools4genotypes.jl:99-235). */
int64_t jwas_hip_estimate_bytes_storage(int64_t n, int64_t p, int32_t ntraits, int32_t block_size, int32_t storage);

/* Benchmark / test data generator (benchmarks/bayesr_parity_common.jl:34-41 shape): allele
 * frequency f_j ~ U(0.1,0.4), x_ij = Bernoulli(f_j)+Bernoulli(f_j), optionally centred by the
 * exact column mean.  kind 1 = X ~ U[0,1) (benchmarks/jwas_nonblock_benchmark.jl:34-51).
 * marker_offset = global index of column 0, so marker shards of one matrix can be generated
 * independently on different GPUs. */
int  jwas_hip_synth_genotypes(jwas_hip_ctx* ctx, uint64_t seed, int32_t kind, int32_t center, int64_t marker_offset);
/* Single-step shaped input (the dense real-valued matrix impute_genotypes hands to the sweep, single_step/SSBR.jl:83-142):
 * rows [0, n_genotyped) are 0/1/2 genotypes as above, rows [n_genotyped, n) are "imputed" -- the average of two
 * genotyped rows drawn per ROW (the same linear map for every marker, as A_ng A_gg^-1 M_g is).  Dense storage only. */
int  jwas_hip_synth_single_step(jwas_hip_ctx* ctx, uint64_t seed, int64_t n_genotyped, int32_t center, int64_t marker_offset);

/* Residual weights R^-1 (n floats; NULL = unit weights): mme.invweights = 1 ./ df.weights (build_MME.jl:305-310).
 * With non-unit weights x'x becomes x'R^-1 x (getXpRinvX, tools4genotypes.jl:28-31), the Grams X_b'R^-1 X_b (:263-266),
 * the block RHS X_b'R^-1 r (block_rhs!, :59-78) and the residual statistics r'R^-1 r / 1'R^-1 r
 * (variance_components.jl:82-98); the residual update itself uses the plain column (BayesABC.jl:48).
 * Call after loading genotypes and BEFORE jwas_hip_setup_blocks (resident block configurations are dropped). */
int  jwas_hip_set_weights(jwas_hip_ctx* ctx, const float* rinv_n);
/* The same for a Float64 context (jwas_hip_set_precision(ctx, 64)): the weights as the Float64 values the reference holds under
 * double_precision = true (invweights, build_MME.jl:310) -- jwas_hip_set_weights on such a context widens Float32 values.
 * A Float32 context rejects it (JWAS_HIP_ESTATE). */
int  jwas_hip_set_weights_f64(jwas_hip_ctx* ctx, const double* rinv_n);

/* ---- precompute: x'x and block Grams ----------------------------------------------------------- */
/* block_size in {64,128,256,512,1024}; markers are processed in consecutive blocks of this size. */
int  jwas_hip_setup_blocks(jwas_hip_ctx* ctx, int32_t block_size, int32_t gram_mode);
int  jwas_hip_get_xpx(jwas_hip_ctx* ctx, float* out_p);
/* Overwrite x'x (e.g. with the .xpRinvx.f32 sidecar of a streaming backend, streaming_genotypes.jl:283-285). */
int  jwas_hip_set_xpx(jwas_hip_ctx* ctx, const float* in_p);
int  jwas_hip_get_gram(jwas_hip_ctx* ctx, int64_t block, float* out_bxb);        /* row-major b x b */
int  jwas_hip_set_gram(jwas_hip_ctx* ctx, int64_t block, const float* in_bxb);
int  jwas_hip_num_blocks(jwas_hip_ctx* ctx, int64_t* nblocks, int32_t* block_size);
/* Overwrite the cross-Gram X_{block-1}' X_block (row-major b_{block-1} x b_block; block >= 1) -- with jwas_hip_set_xpx /
 * jwas_hip_set_gram this lets a host (or the test oracle) supply every precomputed inner product. */
int  jwas_hip_set_cross_gram(jwas_hip_ctx* ctx, int64_t block, const float* in);
/* Read a cross-Gram back (device to host on the context's stream, synchronised, as jwas_hip_get_gram).
 *   level 0: X_{index-1}' X_index of the selected block size, index >= 1 -- the layout jwas_hip_set_cross_gram takes
 *            (b_{index-1} rows, b_index columns, row stride b_index);
 *   level 1: the pair cross-Gram of grouped launches (jwas_hip_setup_groups): rows = the 2 * block_size markers of pair
 *            index - 1, columns = the markers of pair index (fewer on a ragged last pair), row stride = the column count.
 *            At 4 blocks per launch only the odd pairs are stored (the even ones are part of the fours): an even index is
 *            JWAS_HIP_EINVAL;
 *   level 2: the same for fours (4 blocks per launch only).
 * JWAS_HIP_ESTATE when the blocks, or the groups of that level, are not set up; JWAS_HIP_EINVAL for index 0 or an index out of
 * range; a Float64 context has no cross-Grams (JWAS_HIP_EUNSUP). */
int  jwas_hip_get_cross_gram(jwas_hip_ctx* ctx, int32_t level, int64_t index, float* out);
/* Geometry of the streaming (update) role chosen for this matrix: slices (256 rows, one wave each) per row group, row
 * groups, column groups.  The order in which a block's x'r is summed follows from it (fp64; slices of a row group in
 * order, then the row groups in order): the test oracle reproduces it to compare chains bit for bit. */
int  jwas_hip_update_geometry(jwas_hip_ctx* ctx, int32_t* slices_per_row_group, int32_t* row_groups, int32_t* column_groups);
/* Several block sizes can be resident (Grams + cross-Grams each: 8*p*block_size bytes).  The random draws do not depend
 * on the block size, so a host may switch between sweeps: large blocks amortise the per-launch cost when few markers
 * change per sweep, smaller ones keep the serial within-block chain short when many do (the reference's block size is
 * a free tuning knob too: fast_blocks=<number>, JWAS.jl:293-316).  get/set_gram and num_blocks act on the selected size. */
int  jwas_hip_add_block_size(jwas_hip_ctx* ctx, int32_t block_size, int32_t gram_mode);
int  jwas_hip_select_block_size(jwas_hip_ctx* ctx, int32_t block_size);
/* Grouped launches (jwas_sweep_params.group_launch) for the SELECTED block size: blocks_per_launch = 2 or 4 consecutive blocks
 * per launch of the step kernel (block_size * blocks_per_launch <= 4096), 0 = free the buffers again.  Builds the cross-Grams of
 * consecutive pairs (2 blocks per launch: 8 * p * block_size bytes) or of the odd pairs and the fours (4 blocks per launch:
 * 4 + 16 = 20 * p * block_size bytes) -- once; needs uniform blocks.  The
 * reference has no counterpart: like the block size it is a schedule knob of the device (BayesABC.jl:145-187 is the chain). */
int  jwas_hip_setup_groups(jwas_hip_ctx* ctx, int32_t blocks_per_launch, int32_t gram_mode);
/* Explicit, possibly non-uniform block partition: fast_blocks = a vector of block starts (JWAS.jl:298-304,
 * validate_fast_block_starts JWAS.jl:73-79).  starts: nblocks 0-based first markers, starts[0] = 0, strictly increasing;
 * block k = [starts[k], starts[k+1]) (the last one ends at p); at most 1024 markers per block and 32768 blocks.  With
 * jwas_sweep_params.nreps <= 0 every block runs its own size as repetition count (BayesABC.jl:153).  Replaces any resident
 * block configuration; independent_blocks and a second resident block size are not available on it. */
int  jwas_hip_setup_blocks_explicit(jwas_hip_ctx* ctx, const int64_t* starts, int64_t nblocks, int32_t gram_mode);

/* ---- chain state ---------------------------------------------------------------------------- */
/* Declare the sampler so state buffers can be sized: method + ntraits (delta is int32 classes for
 * BayesR, float 0/1 otherwise -- MCMC_BayesianAlphabet.jl:86,119). */
int  jwas_hip_init_state(jwas_hip_ctx* ctx, int32_t method, int32_t ntraits);
/* alpha/beta: p floats; delta: p floats (0/1) or p int32 (BayesR classes).  NULL = leave as is. */
int  jwas_hip_set_state(jwas_hip_ctx* ctx, int32_t trait, const float* alpha, const float* beta, const void* delta);
int  jwas_hip_get_state(jwas_hip_ctx* ctx, int32_t trait, float* alpha, float* beta, void* delta);
/* residual of trait k: n floats */
int  jwas_hip_set_residual(jwas_hip_ctx* ctx, int32_t trait, const float* r_host);
int  jwas_hip_get_residual(jwas_hip_ctx* ctx, int32_t trait, float* r_host);
/* Device pointer / stride of the residual block (t vectors of ld_dev floats) for in-place
 * collectives on it (marker-shard reconcile). */
int  jwas_hip_residual_dev(jwas_hip_ctx* ctx, void** r_dev, int64_t* ld_dev);
/* Device-to-device copies of residual k (n floats) from / to a caller-owned device buffer (e.g. a
 * torch tensor's data_ptr()), ordered on the context's stream -- used around the per-sweep RCCL
 * all-reduce of the residual delta. */
int  jwas_hip_residual_to_dev(jwas_hip_ctx* ctx, int32_t trait, void* dst_dev);
int  jwas_hip_residual_from_dev(jwas_hip_ctx* ctx, int32_t trait, const void* src_dev);
/* Several genotype categories in one model (MCMC_BayesianAlphabet.jl:224-226: `for Mi in mme.M` samples every category from the
 * one ycorr): each category is a context of its own, and the residual changes hands between them.  Copies all ntraits residual
 * vectors of src, pad rows included, into dst's resident residual, device to device, Float32 or Float64 contexts alike.  Ordered by
 * events, without a host round trip or a host wait: the copy is queued on dst's stream and runs after everything queued on src's
 * stream; src's stream in turn waits for the copy before it runs anything queued later.  A copy, not an alias: lifetimes stay per
 * context.  JWAS_HIP_EINVAL unless device, precision, n, leading dimension and ntraits agree; JWAS_HIP_ESTATE unless both contexts
 * hold genotypes and have had jwas_hip_init_state; dst == src is a no-op.  Errors are reported on dst. */
int  jwas_hip_residual_handover(jwas_hip_ctx* dst, jwas_hip_ctx* src);
/* r_k[i] = fl32(fl64(r_k[i]) + shift) for the n individuals: the residual correction of a location parameter whose design
 * column is all ones (the intercept step of the host's single-site Gibbs pass, solver.jl:143-162) without a host copy of
 * the residual -- with jwas_sweep_stats.resid_sum the intercept update needs no O(n) host traffic at all.  Asynchronous
 * (ordered on the context's stream). */
int  jwas_hip_residual_add_scalar(jwas_hip_ctx* ctx, int32_t trait, double shift);
/* r_k -= X * alpha_k for the current device alpha (initial ycorr; sequential fmaf in marker order). */
int  jwas_hip_residual_sub_xalpha(jwas_hip_ctx* ctx, int32_t trait);
/* out = X * alpha_k (n floats, fp64-accumulated). */
int  jwas_hip_mul_alpha(jwas_hip_ctx* ctx, int32_t trait, float* out_host);
/* The nonzero effects of trait k as (marker index, value) lists in marker order, compacted on the device: one saved
 * marker-effect sample as a sparse record instead of the reference's dense text row of p values (output.jl:443-526).
 * idx / val: caller arrays of `capacity` entries (capacity >= p is always enough); *nnz = number of nonzero effects. */
int  jwas_hip_get_alpha_sparse(jwas_hip_ctx* ctx, int32_t trait, int64_t capacity, int32_t* idx, float* val, int64_t* nnz);
/* Rows for which EBVs are reported when they are not exactly the training rows (individuals without records, a
 * user's outputEBV(model, IDs) list): X_out is n_out x p marker-major fp32 with leading dimension ld_host, processed
 * (imputed / centred with the training column means) like the training matrix; copied. */
int  jwas_hip_load_output_dense_f32(jwas_hip_ctx* ctx, const float* X_out_host, int64_t n_out, int64_t p, int64_t ld_host);
/* out = X_out * alpha_k (n_out floats, fp64-accumulated). */
int  jwas_hip_mul_alpha_output(jwas_hip_ctx* ctx, int32_t trait, float* out_host);
/* getEBV (output.jl:281-306) for ALL traits of the context in one call: out_host[k * n_out + i] = jwas_hip_mul_alpha_output of trait
 * k, bit for bit.  On 2-bit packed output rows one kernel reads every byte of a marker with a nonzero effect in any trait once and
 * keeps the sums of all traits (csrc/output.hpp: k_ebv_packed); on dense output rows the traits go one by one.  Float32 contexts. */
int  jwas_hip_ebv_output(jwas_hip_ctx* ctx, float* out_host);
/* Window genomic variances of ONE saved marker-effect sample -- the inner loop of the reference's window-based GWAS
 * (src/3.GWAS/src/GWAS.jl:152-165: genVar = var(X*alpha); per window var(X[:, w]*alpha[w])).  Window w owns the nonzero
 * effects idx[wptr[w] .. wptr[w+1]) (marker indices, any order the caller wants summed in) with values val[..];
 * windows may overlap (sliding windows) and window 0 is typically "all markers".  out_sum[w] = sum_i BV_w[i],
 * out_ss[w] = sum_i BV_w[i]^2 (fp64, deterministic) over the training individuals, or over the output rows of
 * jwas_hip_load_output_dense_f32 when use_output_rows != 0 (the reference uses Mi.output_genotypes). */
int  jwas_hip_window_sums(jwas_hip_ctx* ctx, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx,
                          const float* val, double* out_sum, double* out_ss);
/* Two effect vectors over the same markers (two traits' samples of the same iteration; idx = union of their nonzero
 * effects): additionally out_cross[w] = sum_i BV1_w[i] * BV2_w[i] -- the window genetic covariance / correlation of
 * src/3.GWAS/src/GWAS.jl:199-217. */
int  jwas_hip_window_sums2(jwas_hip_ctx* ctx, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx,
                           const float* val1, const float* val2, double* out_sum1, double* out_ss1, double* out_sum2,
                           double* out_ss2, double* out_cross);

/* ---- GWAS session: window variances and local EBVs of the saved samples, resident on the device -------------------
 * src/3.GWAS/src/GWAS.jl:149-173.  jwas_hip_gwas_begin uploads the windows once: window w is the column range
 * [col_start[w], col_end[w]) exactly as the host's build_windows returns them (sliding windows overlap).  Every device
 * buffer of the session is allocated here (the sample list grows on demand), never per sample.  local_ebv != 0: the
 * session also holds an n_rows x nwin Float64 accumulator and a sample counter, both zeroed; n_rows = the training rows,
 * or the rows of jwas_hip_load_output_dense_f32 / _f64 when use_output_rows != 0.  Dense Float32, 2-bit packed storage or
 * a Float64 context.  A second begin restarts the session; loading genotypes ends it. */
int  jwas_hip_gwas_begin(jwas_hip_ctx* ctx, int32_t use_output_rows, int32_t nwin, const int32_t* col_start, const int32_t* col_end,
                         int32_t local_ebv);
/* ONE saved sample (GWAS.jl:149-173) as the strictly ascending (idx, val) list of its nonzero effects -- a .bin record of
 * the sample files, or what jwas_hip_get_alpha_sparse returns; the library finds every window's slice of the list.
 * out_sum / out_ss hold nwin + 1 entries: entry 0 is "all markers" (genVar, GWAS.jl:155), entry 1 + w window w; they are
 * bit-identical to jwas_hip_window_sums on the CSR description of the same sample.  A session with local EBVs also adds
 * BV_w[i] = sum_j X[i, j] alpha_j of every window to its accumulator.  JWAS_HIP_EUNSUP on a Float64 context (use the
 * _f64 twin). */
int  jwas_hip_gwas_sample(jwas_hip_ctx* ctx, int32_t nnz, const int32_t* idx, const float* val, double* out_sum, double* out_ss);
/* The local EBVs (GWAS.jl:149-173, :164: the mean of BV_w over the samples): out[w * n_rows + i], window-major, the mean
 * over the *nsamples samples folded so far (zeros before the first). */
int  jwas_hip_gwas_local_ebv(jwas_hip_ctx* ctx, double* out, int64_t* nsamples);
/* Launch geometry of the session's partial kernel (GWAS.jl:149-173 has no counterpart; diagnostics): grid = nslices x
 * nchunks workgroups; chunk 0 is entry 0, every other chunk holds windows_per_chunk = max(1, cld(nwin * nslices, 2048))
 * windows. */
int  jwas_hip_gwas_geometry(jwas_hip_ctx* ctx, int32_t* nslices, int32_t* windows_per_chunk, int32_t* nchunks);
/* Free the session (GWAS.jl:149-173: after the last sample); jwas_hip_destroy does it too. */
int  jwas_hip_gwas_end(jwas_hip_ctx* ctx);
/* Device bytes of a session (GWAS.jl:149-173: localEBV is n x nwin), a pure function like jwas_hip_estimate_bytes: rows
 * padded to 256; local_ebv adds exactly 8 * padded_rows * nwin. */
int64_t jwas_hip_gwas_estimate_bytes(int64_t n_rows, int64_t nwin, int64_t max_nnz, int32_t local_ebv);

/* ---- threshold (binary / ordered categorical) and censored traits: the liabilities on the device ---------------------------
 * categorical_and_censored_trait/categorical_and_censored_trait.jl, called from MCMC/MCMC_BayesianAlphabet.jl:186-191 BEFORE the
 * location parameters.  The context owns, per trait, a kind (continuous / categorical / censored), the liability vector (n
 * elements of the context's element type), the category codes and the threshold table (categorical), the bounds (censored).
 * Everything works on the residual the context holds (jwas_hip_set_residual / _f64), whatever the genotype storage (dense
 * Float32, 2-bit packed, a Float64 context); the state is freed by jwas_hip_liability_end, jwas_hip_destroy or loading genotypes.
 * The truncated normals are ONE counter uniform per draw -- philox4x32_10(individual, iteration, 0x40000000 | Gibbs round,
 * 2 + 16 * trait), no rejection loop -- so the same seed gives the same chain whatever the launch geometry.  Every entry point
 * decides its errors before any launch: JWAS_HIP_ESTATE without a residual (jwas_hip_init_state) or before _begin,
 * JWAS_HIP_EINVAL for codes outside 0..ncat, unsorted thresholds or lower > upper, JWAS_HIP_EUNSUP with a communicator attached
 * (shards). */
typedef struct jwas_liability_params {
    uint32_t iteration;                 /* MCMC iteration (enters the RNG counter); jwas_hip_liability_init uses 0           */
    int32_t  ngibbs;                    /* Gibbs rounds over the traits: 5 when >= 2 traits carry liabilities, else 1 (:184-188) */
    uint64_t seed;                      /* runMCMC(seed=...)                                                                  */
    double   R[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];   /* residual covariance, row-major t x t (mme.R.val; 1 trait: R[0]) */
} jwas_liability_params;
/* Start (or restart) the liability state for the ntraits traits of jwas_hip_init_state: every trait continuous (:29-47). */
int  jwas_hip_liability_begin(jwas_hip_ctx* ctx, int32_t ntraits);
/* Trait `trait` is categorical (:50-70): codes[i] in 0..ncat (0 = missing: not truncated, :115-117), ncat = nthresholds - 1;
 * thresholds = {-Inf, t1, ..., +Inf}, strictly increasing, 3 <= nthresholds <= 16.  Record i is bounded by
 * [thresholds[code - 1], thresholds[code]] (:119-120).  The liability vector is set to the codes -- the placeholder phenotype
 * the reference holds in mme.ySparse before the set-up draw (:54). */
int  jwas_hip_liability_set_categorical(jwas_hip_ctx* ctx, int32_t trait, int64_t n, const int32_t* codes, int32_t nthresholds,
                                        const double* thresholds);
/* Trait `trait` is censored (:75-78): lower[i] <= upper[i], +-Inf allowed, lower == upper an exact record.  The liability vector
 * is set to the placeholder add_censored_trait_column! would build (:263-296): upper if lower = -Inf, 0 if both are infinite,
 * else lower. */
int  jwas_hip_liability_set_censored(jwas_hip_ctx* ctx, int32_t trait, int64_t n, const double* lower, const double* upper);
/* New thresholds of a categorical trait (:155,160), the count it was declared with. */
int  jwas_hip_liability_set_thresholds(jwas_hip_ctx* ctx, int32_t trait, int32_t nthresholds, const double* thresholds);
/* The set-up draw (:82-88).  The residual in the context must be y - cmean with y the placeholder CURRENTLY in the liability
 * vector (jwas_hip_get_liabilities right after _set_*), so cmean = liability - residual.  Every liability trait k on its own
 * (no conditioning, params->ngibbs ignored): liability = cmean + eps with eps ~ N(0, R[k][k]) truncated to
 * [lower - cmean, upper - cmean], residual = eps; an exact record (lower == upper): liability = lower, residual = lower - cmean.
 * Continuous traits are not touched.  jwas_hip_init_state zeroes the residual, so after it (and after _set_categorical /
 * _set_censored) jwas_hip_liability_sample answers JWAS_HIP_ESTATE until the set-up draw has been repeated. */
int  jwas_hip_liability_init(jwas_hip_ctx* ctx, const jwas_liability_params* params);
/* sample_liabilities! (:166-210): ngibbs rounds over the liability traits k in order; cmean = liability - residual (:175);
 * eps ~ N(R_12 R_22^-1 r_others, R_11 - R_12 R_22^-1 R_21) truncated to [lower - cmean, upper - cmean] (:196-202);
 * liability = cmean + eps, residual = eps (:203-204); exact records are left alone (:201).  B = R_12 R_22^-1 and the conditional
 * variance are formed once per call in double on the host.  Also leaves the per-category extremes jwas_hip_liability_minmax
 * reads.  params->iteration >= 1.  Asynchronous (ordered on the context's stream). */
int  jwas_hip_liability_sample(jwas_hip_ctx* ctx, const jwas_liability_params* params);
/* For the thresholds i = 1 .. nthresholds - 2 of a categorical trait (:152-155): max_below[i] = the largest liability of
 * category i, min_above[i] = the smallest of category i + 1 (records with code 0 take no part; an empty category gives
 * -Inf / +Inf); entries 0 and nthresholds - 1 are -Inf and +Inf.  Both arrays hold nthresholds doubles.  Exact (max / min of
 * the stored values). */
int  jwas_hip_liability_minmax(jwas_hip_ctx* ctx, int32_t trait, double* max_below, double* min_above);
/* The liabilities of a categorical or censored trait (mme.ySparse, output.jl:514-523) as n doubles: widened from Float32 in a
 * Float32 context. */
int  jwas_hip_get_liabilities(jwas_hip_ctx* ctx, int32_t trait, double* out_n);
int  jwas_hip_liability_end(jwas_hip_ctx* ctx);

/* ---- location parameters: intercepts, covariates, fixed and i.i.d. random class factors on the device ------------------------
 * Step 1 of the reference's iteration (MCMC/MCMC_BayesianAlphabet.jl:193-220): ycorr += X sol, rhs = X'Ri ycorr, one scan of
 * Gibbs(A, x, b[, vare]) (iterative_solver/solver.jl:143-162), ycorr -= X sol.  The levels of one term partition the records, so
 * given the other terms the levels of a term are conditionally independent: a whole term is sampled at once from the residual
 * the context holds and the residual is updated -- exactly that scan (csrc/locpar.hpp has the formulas).  The context owns the
 * term layouts, the solution vector `sol` (doubles: the terms in the order added, a covariate or intercept one entry, a factor one
 * per level) and its running means; all arithmetic is double in both precisions, the residual keeps the context's element type
 * and takes one rounding per term.  Works on any genotype storage; the weights are those in force at _begin.  The state is freed
 * by jwas_hip_locpar_end, jwas_hip_destroy or loading genotypes.  The normal of level l of term j (j counts the terms as added)
 * is rng.hpp's Box-Muller on philox4x32_10(l, iteration, 0x20000000 | j, 3 + 16 * trait): a seed fixes the chain whatever the
 * launch geometry, and every sum is formed in an order fixed by the term's layout (no floating-point atomics).  Every entry
 * point decides its errors before any launch: JWAS_HIP_ESTATE without a residual (jwas_hip_init_state), before _begin, or for a
 * term added after the first use of sol; JWAS_HIP_EINVAL for levels outside -1 .. nlevels - 1, non-finite covariates, a Gi / inv(R)
 * that is not finite and symmetric with a positive diagonal; JWAS_HIP_EUNSUP with a communicator attached (marker or row shards)
 * and for two terms of ONE trait in one random effect (correlated terms within a trait stay on the reference). */
#define JWAS_HIP_LOCPAR_MAX_GROUPS 8
typedef struct jwas_locpar_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    int32_t  first_term, last_term;     /* the terms first_term .. last_term - 1 of the scan, in the order added; last_term < 0: to the end */
    int32_t  reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    double   vare;                      /* one trait: the residual variance (the lambda form, random_effects.jl:232)              */
    double   Rinv[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];      /* several traits: inv(R), row-major t x t                   */
    double   Gi[JWAS_HIP_LOCPAR_MAX_GROUPS * 16];                  /* random effect g: inv(G), row-major k x k at Gi + 16 g, k = its member terms in the order added */
} jwas_locpar_params;
typedef struct jwas_locpar_stats {
    double utu[JWAS_HIP_LOCPAR_MAX_GROUPS * 16];                   /* random effect g: U'U of its member terms AFTER the step, row-major k x k at utu + 16 g (variance_components.jl:121-135) */
    double step_ms;                     /* device time of the step (HIP events on the context's stream)                          */
} jwas_locpar_stats;
/* Start (or restart) the location-parameter state for the ntraits traits of jwas_hip_init_state: no terms, sol empty. */
int  jwas_hip_locpar_begin(jwas_hip_ctx* ctx, int32_t ntraits);
/* Add a one-entry term to trait `trait`: the covariate x (n finite doubles), or the intercept when x == NULL (build_MME.jl:183-290).
 * Terms are sampled in the order they are added: add them trait by trait, term by term -- the reference's equation order. */
int  jwas_hip_locpar_add_covariate(jwas_hip_ctx* ctx, int32_t trait, int64_t n, const double* x);
/* Add a class factor of nlevels levels: level[i] in 0 .. nlevels - 1, or -1 for a record in no level; a level may be empty.
 * random_group -1: a fixed term; 0 .. JWAS_HIP_LOCPAR_MAX_GROUPS - 1: member of that i.i.d. random effect (set_random,
 * random_effects.jl:93-191) -- one term per trait, all of the same nlevels; its position among the members is its row of Gi. */
int  jwas_hip_locpar_add_factor(jwas_hip_ctx* ctx, int32_t trait, int64_t n, const int32_t* level, int64_t nlevels, int32_t random_group);
/* Number of entries of sol. */
int  jwas_hip_locpar_size(jwas_hip_ctx* ctx, int64_t* out_q);
int  jwas_hip_locpar_set_sol(jwas_hip_ctx* ctx, int64_t q, const double* sol);
int  jwas_hip_locpar_get_sol(jwas_hip_ctx* ctx, int64_t q, double* out_sol);
/* One scan over the terms first_term .. last_term - 1 (solver.jl:143-162 in residual-update form); stats (may be NULL) receives
 * the cross-products of EVERY random effect after the step.  Synchronous when stats is given. */
int  jwas_hip_locpar_step(jwas_hip_ctx* ctx, const jwas_locpar_params* params, jwas_locpar_stats* stats);
/* Running means of sol and sol^2 on the device (output.jl:556-560): mean += (sol - mean) / nsamples. */
int  jwas_hip_locpar_accumulate(jwas_hip_ctx* ctx, double nsamples);
int  jwas_hip_locpar_get_means(jwas_hip_ctx* ctx, int64_t q, double* out_mean, double* out_mean2);
/* Device bytes of the state for nterms terms with total_levels entries of sol over n records (pure; an upper bound). */
int64_t jwas_hip_locpar_estimate_bytes(int64_t n, int64_t nterms, int64_t total_levels);
int  jwas_hip_locpar_end(jwas_hip_ctx* ctx);
/* A random effect whose levels are correlated: the polygenic effect of set_random(model, "animal", ped, G) (random_effects.jl:52,
 * 164-172), covariance inv(V) (x) G with V the sparse A-inverse.  jwas_hip_lp_set_group_structure gives random effect
 * `random_group` the inverse covariance V among its nlevels levels as a FULL symmetric CSR matrix (int64 row pointers, int32
 * ascending column indices, doubles); it is called after _begin and before the effect's first member term is added, and every
 * member must then have nlevels levels.  The data sums of a member term are the ones of any term; the prior sum_j V_lj u_j couples
 * only neighbours in V, so the library colours the graph of V on the host (levels in ascending order, the smallest colour no
 * neighbour holds) and samples the levels of one colour per launch, the colours in order: a systematic-scan Gibbs sampler with a
 * fixed visiting order (csrc/locpar.hpp has the formulas and the layout; no floating-point atomics, identical bits run to run).
 * A level without records is drawn from its prior conditional.  jwas_locpar_stats.utu of such an effect holds U' V U.
 * JWAS_HIP_EINVAL: non-finite values, unsorted or duplicate columns, a missing or non-positive diagonal, a pattern or values that
 * are not exactly symmetric, a member added later with another nlevels; JWAS_HIP_ESTATE: before _begin, once a member of the effect
 * exists or sol was used; JWAS_HIP_EUNSUP: a communicator attached.  (The three entry points carry the prefix jwas_hip_lp_.) */
int  jwas_hip_lp_set_group_structure(jwas_hip_ctx* ctx, int32_t random_group, int64_t nlevels, const int64_t* indptr,
                                     const int32_t* indices, const double* values);
/* The colour of every level (0 .. *out_ncolors - 1) of the structure of random effect random_group: the visiting order. */
int  jwas_hip_lp_get_group_colors(jwas_hip_ctx* ctx, int32_t random_group, int64_t nlevels, int32_t* out_color, int32_t* out_ncolors);
/* Device bytes of a structure of nlevels levels and nnz stored entries (pure; an upper bound). */
int64_t jwas_hip_lp_structure_estimate_bytes(int64_t nlevels, int64_t nnz);

/* ---- multi-trait records that miss some traits (csrc/mtmiss.hpp) ---------------------------------------------------------------
 * The reference weights every record with the inverse of the OBSERVED block of R (mkRi / getRi, residual.jl:2-44) and redraws the
 * residuals of its missing traits from their conditional every iteration (sampleMissingResiduals, residual.jl:51-73); after the
 * first residual-variance draw it weights with kron(inv(R), diag(w)) again (MCMC_BayesianAlphabet.jl:357-361) and keeps imputing.
 * A record's CODE has bit k set when trait k is observed: 1 .. 2^t - 1, t <= JWAS_HIP_MAX_TRAITS.  The caller forms the
 * per-code tables in double, so that the device and any restatement read the same numbers; each is [2^t][t][t] doubles,
 * row-major, unused entries 0 (o = the observed traits ascending, m = the missing ones ascending):
 *   B[code]: |m| x |o|, R[m,o] inv(R[o,o]);   U[code]: |m| x |m|, the upper Cholesky factor of R[m,m] - R[m,o] inv(R[o,o]) R[o,m];
 *   C[code]: t x t, inv(R[o,o]) embedded in zeros (the RZ of getRi).
 * Imputation: e_m[c] = sum_j B[c][j] e_o[j] + sum_{a <= c} z_m[a] U[a][c] in that order, in double, rounded to the residual's
 * element type once; z_k is rng.hpp's Box-Muller normal on philox4x32_10(record, iteration, 0x10000000, 4 + 16 * k).  Observed
 * cells and complete records are not written.  Every entry point decides its errors before any launch: JWAS_HIP_EINVAL for a code
 * of 0 or >= 2^t, a wrong n, a non-finite table entry; JWAS_HIP_ESTATE without a residual, before _begin, after the number of
 * traits changed, or for record weights with one trait; JWAS_HIP_EUNSUP with a communicator attached.  The state is freed by
 * _end, jwas_hip_destroy or loading genotypes. */
typedef struct jwas_mtmiss_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    const double* B;                    /* host, [2^t][t][t]                                                                     */
    const double* U;                    /* host, [2^t][t][t]                                                                     */
} jwas_mtmiss_params;
/* Store the codes of the n records (residual.jl:17-21, mme.missingPattern).  After jwas_hip_init_state. */
int  jwas_hip_mtmiss_begin(jwas_hip_ctx* ctx, int64_t n, const int32_t* observed);
/* Redraw the residuals of the missing cells (residual.jl:51-73).  Asynchronous (ordered on the context's stream). */
int  jwas_hip_mtmiss_impute(jwas_hip_ctx* ctx, const jwas_mtmiss_params* params);
/* C != NULL: every later jwas_hip_locpar_step weights record i with C[code_i] (residual.jl:2-44 instead of build_MME.jl:339's
 * kron(inv(R), diag(w))): params->Rinv is ignored, s = 1, the Gi priors as before; the residual weights w stay in force.
 * NULL: back to kron(inv(R), diag(w)) (MCMC_BayesianAlphabet.jl:357-361). */
int  jwas_hip_mtmiss_set_record_weights(jwas_hip_ctx* ctx, const double* C);
/* Device bytes of the state over n records (pure; an upper bound). */
int64_t jwas_hip_mtmiss_estimate_bytes(int64_t n);
int  jwas_hip_mtmiss_end(jwas_hip_ctx* ctx);

/* ---- marker-annotation priors: the probit update from the resident delta (csrc/annot.hpp) --------------------------------------
 * The reference regresses the inclusion indicators on marker annotations between sweeps (MCMC/annotation_updates.jl:21-137,181-361:
 * truncated-normal liabilities, a coordinate Gibbs scan over the annotation coefficients, the rebuilt per-marker prior).  A session
 * keeps the design matrix, the coefficients, the liabilities and the prior table on the device; a step reads the indicators the
 * last sweep left (the context's element type; the int32 classes of BayesR) and writes the table where the next sweep reads it.
 *   JWAS_HIP_ANNOT_BAYESC   1 step,  table = pi_vec  (p)              needs JWAS_HIP_BAYESC
 *   JWAS_HIP_ANNOT_BAYESR   3 steps, table = pi_matrix (p x 4)        needs JWAS_HIP_BAYESR
 *   JWAS_HIP_ANNOT_TREE     3 steps, table = log_prior_states_matrix  needs JWAS_HIP_MTBAYESC1 / 2 with two traits (states 00, 10, 01, 11)
 * While a session is open, a sweep whose pi_vec / pi_matrix / log_prior_states_matrix is NULL reads the session's resident table
 * (the convention of var_effect_matrix == NULL); a host pointer in that field is JWAS_HIP_EINVAL.  The limits of the marker-specific
 * joint prior stay (two traits, block size <= 512).  All arithmetic is double in both precisions; csrc/annot.hpp has the formulas,
 * the order of every sum (fixed by p alone: no floating-point atomics, identical bits run to run) and the RNG counters
 * (philox4x32_10(marker | coefficient, iteration, 0x08000000 | step, 5 | 6)).  The shrinkage variance of a step's slopes is the
 * caller's draw (annotation_updates.jl:125-137), passed into the next step.  Errors are decided before any launch: JWAS_HIP_ESTATE
 * for _begin before jwas_hip_init_state or during a session, and for every other entry point without one; JWAS_HIP_EINVAL for a kind
 * that does not match the context's method or trait count, a wrong p, ncols outside 1 .. JWAS_HIP_ANNOT_MAX_COLS, a first column
 * that is not all ones, non-finite values, a variance that is not positive; JWAS_HIP_EUNSUP with a communicator attached and for
 * the constraint = true methods (JWAS_HIP_MEGABAYES*).  The session is freed by _end, jwas_hip_init_state, jwas_hip_destroy or
 * loading genotypes. */
#define JWAS_HIP_ANNOT_MAX_COLS 64
enum { JWAS_HIP_ANNOT_BAYESC = 0, JWAS_HIP_ANNOT_BAYESR = 1, JWAS_HIP_ANNOT_TREE = 2 };
typedef struct jwas_annot_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    double   variance[3];               /* the shrinkage variance of every step's slopes (not read when ncols == 1)              */
} jwas_annot_params;
typedef struct jwas_annot_stats {
    double  coef[3 * JWAS_HIP_ANNOT_MAX_COLS];  /* the coefficients AFTER the step: step s at coef + s * ncols                  */
    int64_t n_active[3];                /* |A_s| of every step                                                                   */
    double  means[4];                   /* column means of the table (the probabilities, not their logs); BayesC: means[0]       */
    double  step_ms;                    /* device time of the step (HIP events on the context's stream)                          */
} jwas_annot_stats;
/* Open a session.  D_rowmajor: the p x ncols design matrix, column 0 the intercept's ones; coef: [nsteps][ncols] start values;
 * variance: [nsteps] (checked only: every step takes its variances from its params; may be NULL); start_prior: the table the
 * first sweep reads -- p, p x 4 or the p x 4 logs.  Liabilities and mu start at 0. */
int  jwas_hip_annot_begin(jwas_hip_ctx* ctx, int32_t kind, int64_t p, int32_t ncols, const double* D_rowmajor, const double* coef,
                          const double* variance, const double* start_prior);
/* One update: every step's liabilities and coefficient scan from the resident delta, then the table.  Synchronous. */
int  jwas_hip_annot_step(jwas_hip_ctx* ctx, const jwas_annot_params* params, jwas_annot_stats* stats);
/* Running mean and mean of squares of the per-marker prior probabilities on the device: mean += (v - mean) / nsamples. */
int  jwas_hip_annot_accumulate(jwas_hip_ctx* ctx, double nsamples);
/* The resident table as the sweep reads it (nvalues = p for BayesC, 4 p otherwise). */
int  jwas_hip_annot_get_prior(jwas_hip_ctx* ctx, int64_t nvalues, double* out);
int  jwas_hip_annot_get_means(jwas_hip_ctx* ctx, int64_t nvalues, double* out_mean, double* out_mean2);
/* The liabilities / mu of every step, [nsteps][p] (for tests and sample files). */
int  jwas_hip_annot_get_liability(jwas_hip_ctx* ctx, int64_t nvalues, double* out);
int  jwas_hip_annot_get_mu(jwas_hip_ctx* ctx, int64_t nvalues, double* out);
/* Device bytes of a session (pure; an upper bound). */
int64_t jwas_hip_annot_estimate_bytes(int64_t p, int32_t ncols, int32_t kind);
int  jwas_hip_annot_end(jwas_hip_ctx* ctx);

/* ---- structural equation models: the recursive causal structure among the traits (csrc/sem.hpp) ------------------------------------
 * runMCMC(...; causal_structure = cs) samples the structural coefficients after the residual-variance draw of every iteration
 * (MCMC/MCMC_BayesianAlphabet.jl:165-169,372-377,410-412; structure_equation_model/SEM.jl:53-165; Wang et al. 2020, G3).  t traits
 * (2 <= t <= JWAS_HIP_MAX_TRAITS), n records, y (t x n) the constant phenotypes, cs the t x t strictly lower 0/1 structure
 * (cs[i][j] = 1: trait j acts on trait i), P_i the parents of trait i ascending.  The resident residual is the reference's
 * "Lambda ycorr", r_i = y_i - sum_{j in P_i} lambda_ij y_j - fitted_i; lambda starts at 0.  A session keeps y, S = y y' and the
 * coefficients on the device.  One step, for every trait i with parents, all arithmetic double without contraction:
 *     C_ji  = y_j'r_i                  j in P_i
 *     rhs_q = (C_{P_q,i} + sum_m S_{P_q,P_m} lambda_old_m) / R_ii       (m ascending, the sum starts from C)
 *     F_qm  = S_{P_q,P_m} / R_ii + (q == m)                              (prior lambda ~ N(0, 1), SEM.jl:134-138; only diag(R), SEM.jl:129)
 *     F = L L',  mu = inv(F) rhs,  lambda_new = mu + inv(L') z
 *     r_i,n = T(((double(r_i,n) + d_1 y_j1,n) + d_2 y_j2,n) + ...)       d = lambda_old - lambda_new, parents ascending
 * z_q, the normal of the q-th parent of trait i: Box-Muller as the location parameters' (u1 from words (1, 0), u2 from (3, 2)) on
 * philox4x32_10(q, iteration, 0x04000000 | i, 7).  The coefficient estimated from the design column (i, j) is lambda_ij: the
 * reference maps its draw back in column order, which differs from the row order of its design from t = 4 on.
 * Order of the sums: pieces of 1024 records, G = min(ceil(n / 1024), 512) workgroups of 256 threads (workgroup b: pieces b, b + G, ...),
 * a thread adds its records in ascending order, a wave meets in a shuffle tree, the four waves in wave order, the G partials in
 * ascending order in one workgroup -- a function of n alone, no floating-point atomics, identical bits from run to run.
 * jwas_hip_sem_accumulate: indirect_k = sum_j K[k][j] alpha_j (j ascending from 0), overall_k = alpha_k + indirect_k per marker,
 * K = sum_{m=1}^{t-1} Lambda^m from the caller (compute_indirect_effect, SEM.jl:245-252); running mean, mean of squares and frequency
 * of non-zero of both in double, mean += (v - mean) / nsamples.
 * Every t x t matrix of this section is row-major with stride t; only the strictly lower part is used.
 * Errors are decided before any launch: JWAS_HIP_ESTATE for _begin before jwas_hip_init_state or without a residual, for every
 * other entry point without a session, and after jwas_hip_init_state changed the number of traits; JWAS_HIP_EINVAL for one trait
 * (or ntraits that differs from the context's), a wrong n, a structure that is not 0/1 and strictly lower, non-finite y, lambda or
 * K, a lambda outside the structure, R_diag that is not positive and finite, iteration == 0, nsamples < 1, a kind or trait outside
 * its range; JWAS_HIP_EUNSUP with a communicator attached.  _begin on an open session replaces it.  The session is freed by _end,
 * jwas_hip_destroy or loading genotypes. */
typedef struct jwas_sem_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    double   R_diag[JWAS_HIP_MAX_TRAITS];   /* the diagonal of the residual covariance                                           */
} jwas_sem_params;
typedef struct jwas_sem_stats {
    double lambda[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];   /* the coefficients AFTER the step                               */
    double mean[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];     /* mu: the mean of their full conditional                        */
    double ypr[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];      /* C_ji = y_j'r_i at [i][j], from the residual BEFORE the step   */
    double step_ms;                     /* device time of the step (HIP events on the context's stream)                          */
} jwas_sem_stats;
/* Open a session: y_t_n the phenotypes (row-major t x n), structure_t_t the causal structure. */
int  jwas_hip_sem_begin(jwas_hip_ctx* ctx, int32_t ntraits, int64_t n, const double* y_t_n, const int32_t* structure_t_t);
/* One update of every coefficient and of the residual.  Synchronous. */
int  jwas_hip_sem_step(jwas_hip_ctx* ctx, const jwas_sem_params* params, jwas_sem_stats* stats);
int  jwas_hip_sem_get_lambda(jwas_hip_ctx* ctx, double* out_t_t);
/* The state only: the residual is not touched. */
int  jwas_hip_sem_set_lambda(jwas_hip_ctx* ctx, const double* lambda_t_t);
/* S = y y' as the step reads it. */
int  jwas_hip_sem_get_gram(jwas_hip_ctx* ctx, double* out_t_t);
int  jwas_hip_sem_accumulate(jwas_hip_ctx* ctx, const double* K_t_t, double nsamples);
/* kind 0: indirect, 1: overall; p values each, any of the three may be NULL. */
int  jwas_hip_sem_get_effects(jwas_hip_ctx* ctx, int32_t kind, int32_t trait, double* mean, double* mean2, double* freq);
/* Device bytes of a session (pure; an upper bound). */
int64_t jwas_hip_sem_estimate_bytes(int64_t n, int64_t p, int32_t ntraits);
int  jwas_hip_sem_end(jwas_hip_ctx* ctx);

/* ---- random regression models: every marker carries c regression coefficients (csrc/rrm.hpp) ----------------------------------------
 * runMCMC(...; RRM = Phi) fits longitudinal records: n individuals with up to T records each, one per time point, Phi (T x c) the
 * covariates of the time points (RRM/RRM.jl, RRM/MCMC_BayesianAlphabet_RRM.jl).  The session keeps a residual W (T x n doubles,
 * exactly 0 at every cell without a record -- the reference's yfull, RRM.jl:12-20,151), the coefficients alpha, beta, delta (c x p)
 * and their running means, all in double whatever the context's element type; the genotypes are the context's (dense Float32 or
 * Float64).  Per marker, in marker order (BayesABCRRM!, RRM.jl:101-158):
 *   xw = sum_i x_ij sum_t m_it phi_t W_it + M_j alpha_j,     M_j = sum_i x_ij^2 sum_t m_it phi_t phi_t'   (get_mΦΦarray, RRM.jl:43-57)
 *   every state delta in {0,1}^c (bit q of the state index = coefficient q): lhs = D M_j D / vare + inv(G), rhs = D xw / vare,
 *   logDelta = -0.5 (log det lhs - rhs'inv(lhs) rhs) + log pi(state);  state ~ Categorical(softmax(logDelta)) from ONE uniform (CDF walk
 *   in state-index order, the last state when rounding leaves u above the total);  beta = inv(lhs) rhs + chol(inv(lhs)) z with one
 *   shared z (the reference draws one MvNormal per candidate and picks by dictionary position, RRM.jl:123-141: the law is the same,
 *   the stream is not);  alpha = D beta;  W_it += m_it x_ij phi_t'(alpha_old - alpha).
 * The device runs the exact block form of this chain: per block of <= 256 markers the right-hand sides from the residual at block
 * entry, corrected inside the block through a block Gram tensor G_jk = sum_i x_ij x_ik sum_t m_it phi_t phi_t' (c (c + 1) / 2
 * doubles per marker pair of a block: 8 p b c (c + 1) / 2 bytes), the residual brought up to date at the next block's entry.
 * Draws: philox4x32_10(marker, iteration, 0x02000000, slot), slot 8 the uniform, slot 9 + 16 q the normal of coefficient q; they
 * do not depend on the block size.  No floating-point atomics: every sum has a fixed order, the same seed gives the same bits.
 * Limits: 2 <= c <= 4, 1 <= T <= 64, block size <= 256 (0: 64), uniform blocks.
 * Errors: JWAS_HIP_ESTATE without loaded genotypes or, for every other entry point, without an open session; JWAS_HIP_EUNSUP on 2-bit
 * packed storage (the reference refuses RRM on storage=:stream, input_data_validation.jl:97-98), with residual weights and on marker
 * or row shards; JWAS_HIP_EINVAL for c, T, n, the block size out of range, a record bit at or above T, non-finite Phi, vare or G, a
 * G that is not symmetric positive definite, a NaN or +Inf log prior.  A failed _begin opens nothing; _begin on an open session
 * replaces it.  The session is freed by _end, jwas_hip_destroy or loading genotypes. */
typedef struct jwas_rrm_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    double   vare;                      /* the residual variance (a scalar: RRM.jl:81)                                           */
    double   G[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];      /* c x c row-major in the first c c entries                      */
    double   log_pi[JWAS_HIP_MAX_STATES];                       /* log pi(state), 2^c entries (-Inf: the state is excluded)      */
} jwas_rrm_params;
typedef struct jwas_rrm_stats {
    double state_counts[JWAS_HIP_MAX_STATES];                   /* markers per state after the sweep (samplePi, Pi.jl)           */
    double beta_ss[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];  /* beta'beta, c x c row-major in the first c c entries           */
    double alpha_ss;                    /* sum of squares of all coefficients                                                    */
    double resid_ss;                    /* sum W^2 after the sweep                                                               */
    double n_changed;                   /* markers whose coefficients moved                                                      */
    double step_ms;                     /* device time of the sweep (HIP events on the context's stream)                         */
} jwas_rrm_stats;
/* Open a session: phi_T_c row-major T x c, mask_n one word per individual (bit t: a record at time t).  Builds M_j and the Grams
 * (get_mΦΦarray, RRM.jl:43-57, and its block extension). */
int  jwas_hip_rrm_begin(jwas_hip_ctx* ctx, int32_t T, int32_t c, int64_t n, const double* phi_T_c, const uint64_t* mask_n, int32_t block_size);
/* The residual, row-major T x n (yfull, MCMC_BayesianAlphabet_RRM.jl:62-73,123,144).  _set forces the cells without a record to 0. */
int  jwas_hip_rrm_set_residual(jwas_hip_ctx* ctx, int64_t nvalues, const double* W_T_n);
int  jwas_hip_rrm_get_residual(jwas_hip_ctx* ctx, int64_t nvalues, double* out_T_n);
/* alpha, beta, delta, each row-major c x p; any may be NULL (Mi.α, Mi.β, Mi.δ: MCMC_BayesianAlphabet_RRM.jl:52-57). */
int  jwas_hip_rrm_set_state(jwas_hip_ctx* ctx, const double* alpha, const double* beta, const double* delta);
int  jwas_hip_rrm_get_state(jwas_hip_ctx* ctx, double* alpha, double* beta, double* delta);
/* One sweep over all markers (BayesABCRRM!, RRM.jl:101-158).  Synchronous. */
int  jwas_hip_rrm_sweep(jwas_hip_ctx* ctx, const jwas_rrm_params* params, jwas_rrm_stats* stats);
/* Running mean, mean of squares and model frequency of every coefficient (MCMC_BayesianAlphabet_RRM.jl:214-218). */
int  jwas_hip_rrm_accumulate(jwas_hip_ctx* ctx, double nsamples);
/* ... of coefficient q: p values each, any may be NULL. */
int  jwas_hip_rrm_get_posterior(jwas_hip_ctx* ctx, int32_t q, double* mean, double* mean2, double* freq);
/* out_n = X alpha_q, the genomic values of coefficient q (getEBV, output.jl:281-306). */
int  jwas_hip_rrm_mul_alpha(jwas_hip_ctx* ctx, int32_t q, double* out_n);
/* M_j, p x c (c + 1) / 2 doubles (lower cells, cell(a, b) = a (a + 1) / 2 + b), and the Gram tensor of one block,
 * b x b x c (c + 1) / 2 with b the block's markers (mΦΦArray, RRM.jl:43-57). */
int  jwas_hip_rrm_get_m(jwas_hip_ctx* ctx, int64_t nvalues, double* out);
int  jwas_hip_rrm_get_gram(jwas_hip_ctx* ctx, int64_t block, int64_t nvalues, double* out);
/* Device bytes of a session (pure; an upper bound). */
int64_t jwas_hip_rrm_estimate_bytes(int64_t n, int64_t p, int32_t T, int32_t c, int32_t block_size);
int  jwas_hip_rrm_end(jwas_hip_ctx* ctx);

/* ---- mega-trait models: constraint = true with up to 64 traits (csrc/mega.hpp) --------------------------------------------------------
 * megaBayesABC! (markers/BayesianAlphabet/BayesABC.jl:1-8) runs T independent single-trait chains over ONE genotype matrix; the
 * sweep entry point above stops at JWAS_HIP_MAX_TRAITS.  A session keeps per trait k a residual r_k (n doubles), alpha_k, beta_k,
 * delta_k (p each) and their running means, and once for all traits x'x and the within-block Grams G_ij = x_i'x_j (8 p b bytes),
 * all in double whatever the context's element type; the genotypes are the context's (dense Float32 or Float64).  One marker of
 * one trait, markers in order (bayesabc_update_marker!, BayesABC.jl:24-58), with vare_k, the trait's effect variance v_k and pi_k:
 *   rhs = (x'r + x'x alpha) / vare,  lhs = x'x / vare + 1 / v,  gHat = rhs / lhs,
 *   logDelta1 = -0.5 (log lhs + log v - gHat rhs) + log(1 - pi),  logDelta0 = log pi,  probDelta1 = 1 / (1 + exp(logDelta0 - logDelta1)),
 *   u < probDelta1: delta = 1, beta = alpha = gHat + z / sqrt(lhs);  else delta = 0, alpha = 0, beta = z sqrt(v)   (BayesABC.jl:54);
 *   pi = 0 (RR-BLUP, megaBayesC0!) includes every marker.
 * The device runs the exact block form: per block of <= 256 markers the right-hand sides of ALL traits from the residuals at block
 * entry in one pass over the block's genotypes (a small GEMM X_b'R), corrected inside the block through the Gram, the residuals
 * brought up to date at the next block's entry.  Draws: philox4x32_10(marker, iteration, 0x01000000 | trait_id, slot), slot 10 the
 * uniform, slot 11 the normal; (record, iteration, 0x01000000 | trait_id, 12) the normal of a missing cell; trait_id = first_trait +
 * k.  No sum of trait k depends on T: trait k of a T-trait session is bit-equal to a one-trait session with first_trait = k.  No
 * floating-point atomics: the same seed gives the same bits.
 * Limits: 1 <= T <= 64 (JWAS_HIP_MEGA_MAX_TRAITS), block size <= 256 (0: 64), uniform blocks, first_trait + T <= 2^24.
 * Errors: JWAS_HIP_ESTATE without loaded genotypes or, for every other entry point, without an open session; JWAS_HIP_EUNSUP on 2-bit
 * packed storage, with residual weights and on marker or row shards; JWAS_HIP_EINVAL for T, the block size or first_trait out of
 * range, a trait index outside [0, T), a wrong length, non-finite values, vare or var_effect not positive and finite, pi outside
 * [0, 1].  A failed _begin opens nothing; _begin on an open session replaces it.  The session is freed by _end, jwas_hip_destroy or
 * loading genotypes. */
#define JWAS_HIP_MEGA_MAX_TRAITS 64
#define JWAS_HIP_MEGA_MAX_BLOCK 256
typedef struct jwas_mega_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    const double* vare;                 /* [T] vare[k,k]                                                                         */
    const double* var_effect;           /* [T] the marker-effect variance of every trait (_sweep only; _impute ignores it)       */
    const double* pi;                   /* [T] Pr(delta = 0) of every trait (_sweep only)                                        */
} jwas_mega_params;
typedef struct jwas_mega_stats {        /* every pointer: T doubles of the caller (any may be NULL)                              */
    double* sum_delta;                  /* markers in the model (samplePi, MCMC_BayesianAlphabet.jl:299)                         */
    double* beta_ss;                    /* beta'beta (sample_marker_effect_variance, constraint branch)                          */
    double* alpha_ss;                   /* alpha'alpha                                                                           */
    double* resid_ss;                   /* sum r^2 after the sweep (variance_components.jl:104-109)                              */
    double* resid_sum;                  /* sum r                                                                                 */
    double* n_changed;                  /* markers whose effect moved                                                            */
    double  step_ms;                    /* device time of the sweep (HIP events on the context's stream)                         */
} jwas_mega_stats;
/* Open a session of ntraits traits on the loaded genotypes: x'x and the block Grams; residuals, alpha and beta 0, delta 1
 * (BayesABC.jl:1-8: one BayesABC! per trait). */
int  jwas_hip_mega_begin(jwas_hip_ctx* ctx, int32_t ntraits, int32_t block_size, int32_t first_trait);
/* missing_T_n: row-major T x n bytes, nonzero where the record misses the trait (mme.missingPattern negated, residual.jl:17-21);
 * NULL: complete records. */
int  jwas_hip_mega_set_missing(jwas_hip_ctx* ctx, int64_t nvalues, const uint8_t* missing_T_n);
/* The residual of one trait, n doubles (wArray[i], MCMC_BayesianAlphabet.jl:131-157). */
int  jwas_hip_mega_set_residual(jwas_hip_ctx* ctx, int32_t trait, const double* r_n);
int  jwas_hip_mega_get_residual(jwas_hip_ctx* ctx, int32_t trait, double* out_n);
/* alpha, beta, delta of one trait, p doubles each; any may be NULL (genotypes.α[i], β[i], δ[i]). */
int  jwas_hip_mega_set_state(jwas_hip_ctx* ctx, int32_t trait, const double* alpha, const double* beta, const double* delta);
int  jwas_hip_mega_get_state(jwas_hip_ctx* ctx, int32_t trait, double* alpha, double* beta, double* delta);
/* Every missing cell redrawn from N(0, vare_k) (sampleMissingResiduals, residual.jl:51-73, with a diagonal R). */
int  jwas_hip_mega_impute(jwas_hip_ctx* ctx, const jwas_mega_params* params);
/* One sweep over all markers of all traits (megaBayesABC!, BayesABC.jl:1-8,24-58).  Synchronous. */
int  jwas_hip_mega_sweep(jwas_hip_ctx* ctx, const jwas_mega_params* params, jwas_mega_stats* stats);
/* Running mean, mean of squares and model frequency of every effect (output.jl:556-577). */
int  jwas_hip_mega_accumulate(jwas_hip_ctx* ctx, double nsamples);
/* ... of one trait: p values each, any may be NULL. */
int  jwas_hip_mega_get_posterior(jwas_hip_ctx* ctx, int32_t trait, double* mean, double* mean2, double* freq);
/* out = X alpha_k (getEBV, output.jl:281-306): n doubles over the context's rows, or n_out over the rows of the second resident
 * matrix (Mi.output_genotypes) when use_output_rows != 0. */
int  jwas_hip_mega_mul_alpha(jwas_hip_ctx* ctx, int32_t trait, int32_t use_output_rows, double* out);
/* The Gram of one block, b x b doubles with b the block's markers, and (out_xpx != NULL) the block's x'x, b doubles
 * (GibbsMats, tools4genotypes.jl:28-36). */
int  jwas_hip_mega_get_gram(jwas_hip_ctx* ctx, int64_t block, int64_t nvalues, double* out_gram, double* out_xpx);
/* ---- several chains of one model in a session: BayesR and the potential scale reduction factor ------------------------------------
 * K chains of one single-trait model are K traits whose record is the same: chain k is trait k of the session, with the Philox
 * trait id first_trait + k.  BayesC and RR-BLUP chains run on jwas_hip_mega_sweep; BayesR chains on jwas_hip_mega_sweep_r, the
 * same block walk under the 4-class law (markers/BayesianAlphabet/BayesR.jl:56-96), all in double.  Per chain vare, sigma2 =
 * var_effect, gamma[4] with gamma_1 = 0, pi[4]; one marker:
 *   rhs = (x'r + x'x alpha) / vare;  c = 2..4: v_c = gamma_c sigma2, lhs_c = x'x / vare + 1 / v_c, bHat_c = rhs / lhs_c,
 *   lp_c = 0.5 (log(1 / lhs_c) - log v_c + bHat_c rhs) + log pi_c;  lp_1 = log pi_1;  probs by the max-shifted log-sum-exp;
 *   the class by the CDF walk `while cp <= u` on the uniform of slot 10; class 1: alpha = 0, else alpha = bHat_c + z sqrt(1 / lhs_c)
 *   with the normal of slot 11; delta = the class, 1..4; beta = alpha.
 * gamma and pi are row-major [4][T]: value c of chain k at [c * T + k].  The statistics are summed in the order of the BayesC
 * statistics (lane order, the shuffle tree, the blocks in stream order): chain k of a K-chain session is bit-equal to a one-chain
 * session with first_trait = k.  jwas_hip_mega_set_state checks delta against {0, 1}: a BayesR chain is started from the session's
 * own starting state or from alpha alone (the law reads no delta).  The first _sweep_r and the first _psrf of a session allocate
 * 8 (18 T + 2 T ceil(n / 256)) and 8 p bytes beyond jwas_hip_mega_estimate_bytes.
 * Errors: as the session's; JWAS_HIP_EINVAL also for class probabilities of a chain that do not sum to 1 within 1e-8 or lie
 * outside [0, 1], gamma_1 != 0, another gamma or sigma2 not positive and finite; _psrf: fewer than 2 chains or nsamples < 2. */
typedef struct jwas_mega_r_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    const double* vare;                 /* [T] the residual variance of every chain                                              */
    const double* var_effect;           /* [T] sigma2 of every chain                                                             */
    const double* gamma;                /* [4][T] the class multipliers (gamma[0][k] = 0)                                        */
    const double* pi;                   /* [4][T] the class probabilities                                                        */
} jwas_mega_r_params;
typedef struct jwas_mega_r_stats {      /* every pointer: doubles of the caller (any may be NULL)                                */
    double* class_counts;               /* [4][T] markers per class (the Dirichlet update of pi)                                 */
    double* ssq;                        /* [T] sum alpha_j^2 / gamma_class(j) over the markers outside class 1                   */
    double* nnz;                        /* [T] the number of those markers                                                       */
    double* alpha_ss;                   /* [T] alpha'alpha                                                                       */
    double* resid_ss;                   /* [T] sum r^2 after the sweep                                                           */
    double* resid_sum;                  /* [T] sum r                                                                             */
    double* n_changed;                  /* [T] markers whose effect moved                                                        */
    double  step_ms;                    /* device time of the sweep                                                              */
} jwas_mega_r_stats;
/* One BayesR sweep over all markers of all chains.  Synchronous. */
int  jwas_hip_mega_sweep_r(jwas_hip_ctx* ctx, const jwas_mega_r_params* params, jwas_mega_r_stats* stats);
/* jwas_hip_mega_accumulate for BayesR chains: the model frequency is the frequency of class > 1. */
int  jwas_hip_mega_accumulate_r(jwas_hip_ctx* ctx, double nsamples);
/* The potential scale reduction factor of every marker effect (Gelman and Rubin) from the running means m_k and means of squares
 * q_k of the session's T >= 2 chains after nsamples >= 2 accumulated samples, p doubles:
 *   s_k^2 = N / (N - 1) (q_k - m_k^2),  W = mean_k s_k^2,  B / N = sum_k (m_k - mean m)^2 / (T - 1),
 *   V = (N - 1) / N W + B / N,  out = sqrt(V / W);  NaN where W = 0 (the marker never entered the model in any chain).
 * The chains are added in ascending order; a pure function of the accumulators. */
int  jwas_hip_mega_psrf(jwas_hip_ctx* ctx, double nsamples, double* out_p);
/* Device bytes of a session (pure; an upper bound). */
int64_t jwas_hip_mega_estimate_bytes(int64_t n, int64_t p, int32_t ntraits, int32_t block_size);
int  jwas_hip_mega_end(jwas_hip_ctx* ctx);

/* ---- unconstrained multi-trait BayesC with 5 to 8 traits: Gibbs sampler I (csrc/mtjoint.hpp) -------------------------------------------
 * _MTBayesABC_samplerI! (markers/BayesianAlphabet/MTBayesABC.jl:57-127) with a full T x T marker-effect covariance G common to all
 * markers, a full residual covariance R and Pi over the 2^T joint inclusion states, complete records; the sweep entry point above
 * stops at JWAS_HIP_MAX_TRAITS.  The session keeps what a mega-trait session keeps (residuals, alpha, beta, delta, their running
 * means, x'x and the within-block Grams, all double whatever the context's element type) and runs the same exact block form.  One
 * marker, with w_k = x'r_k + x'x alpha_k for every k at the marker's entry, Rinv = inv(R), Ginv = inv(G), then k = 0 .. T-1 in order:
 *   Ginv11 = Ginv[k][k],  C11 = Ginv11 + Rinv[k][k] x'x,
 *   gHat0 = -(sum_{l != k} Ginv[k][l] beta_l) / Ginv11,
 *   gHat1 = (sum_l w_l Rinv[l][k] - sum_{l != k} (Ginv[k][l] + x'x delta_l Rinv[k][l]) beta_l) / C11,
 *   logDelta0 = -0.5 (log Ginv11 - gHat0^2 Ginv11) + log pi[d0],  logDelta1 = -0.5 (log C11 - gHat1^2 C11) + log pi[d1]
 *     (d0 / d1: the marker's joint state, bit l = delta_l, with bit k cleared / set),  probDelta1 = 1 / (1 + exp(logDelta0 - logDelta1)),
 *   u < probDelta1: delta_k = 1, beta_k = alpha_k = gHat1 + z / sqrt(C11);  else delta_k = 0, alpha_k = 0, beta_k = gHat0 + z / sqrt(Ginv11);
 *   after the marker r_k += x (alpha_k,old - alpha_k,new).  A state with log pi = -Inf is never entered.
 * Draws: philox4x32_10(marker, iteration, 0x05000000 | trait, slot), slot 14 the uniform, slot 15 the normal.  No floating-point
 * atomics: the same seed gives the same bits.
 * Limits: 5 <= T <= 8, block size <= 256 (0: 64), uniform blocks.
 * Errors: JWAS_HIP_ESTATE without loaded genotypes or, for every other entry point, without an open session; JWAS_HIP_EUNSUP on 2-bit
 * packed storage, with residual weights and on marker or row shards; JWAS_HIP_EINVAL for T or the block size out of range, a trait
 * index outside [0, T), non-finite values, rinv or ginv not finite, not symmetric or not positive definite, npi != 2^T, a log pi
 * that is NaN or above 0, or no state of positive probability.  A failed _begin opens nothing; _begin on an open session replaces
 * it.  The session is freed by _end, jwas_hip_destroy or loading genotypes. */
#define JWAS_HIP_MTJ_MIN_TRAITS 5
#define JWAS_HIP_MTJ_MAX_TRAITS 8
typedef struct jwas_mtj_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    uint32_t reserved;
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    const double* rinv;                 /* [T][T] inv(vare), row-major                                                           */
    const double* ginv;                 /* [T][T] inv(G)                                                                         */
    const double* log_pi;               /* [npi] log Pr(joint state), state = sum_k delta_k 2^k; -Inf: probability 0             */
    int64_t npi;                        /* 2^T                                                                                   */
} jwas_mtj_params;
typedef struct jwas_mtj_stats {         /* every pointer: doubles of the caller (any may be NULL)                                */
    double* state_counts;               /* [2^T] markers per joint state (the Dirichlet update of Pi)                            */
    double* beta_ss;                    /* [T][T] sum_j beta_j beta_j' (symmetric bit for bit)                                   */
    double* alpha_ss;                   /* [T] alpha_k'alpha_k                                                                   */
    double* resid_cp;                   /* [T][T] sum_i r_k[i] r_l[i] after the sweep (symmetric bit for bit)                    */
    double* resid_sum;                  /* [T] sum r_k                                                                           */
    double  n_changed;                  /* markers with an effect that moved                                                     */
    double  step_ms;                    /* device time of the sweep (HIP events on the context's stream)                         */
} jwas_mtj_stats;
/* Open a session of ntraits traits on the loaded genotypes: x'x and the block Grams; residuals, alpha and beta 0, delta 1. */
int  jwas_hip_mtj_begin(jwas_hip_ctx* ctx, int32_t ntraits, int32_t block_size);
int  jwas_hip_mtj_set_residual(jwas_hip_ctx* ctx, int32_t trait, const double* r_n);
int  jwas_hip_mtj_get_residual(jwas_hip_ctx* ctx, int32_t trait, double* out_n);
/* alpha, beta, delta of one trait, p doubles each; any may be NULL. */
int  jwas_hip_mtj_set_state(jwas_hip_ctx* ctx, int32_t trait, const double* alpha, const double* beta, const double* delta);
int  jwas_hip_mtj_get_state(jwas_hip_ctx* ctx, int32_t trait, double* alpha, double* beta, double* delta);
/* The Gram of one block, b x b doubles, and (out_xpx != NULL) the block's x'x, b doubles. */
int  jwas_hip_mtj_gram(jwas_hip_ctx* ctx, int64_t block, int64_t nvalues, double* out_gram, double* out_xpx);
/* One sweep over all markers (MTBayesABC.jl:75-126).  Synchronous. */
int  jwas_hip_mtj_sweep(jwas_hip_ctx* ctx, const jwas_mtj_params* params, jwas_mtj_stats* stats);
/* Running mean, mean of squares and model frequency of every effect (output.jl:556-577). */
int  jwas_hip_mtj_accumulate(jwas_hip_ctx* ctx, double nsamples);
/* ... of one trait: p values each, any may be NULL. */
int  jwas_hip_mtj_posterior(jwas_hip_ctx* ctx, int32_t trait, double* mean, double* mean2, double* freq);
/* out = X alpha_k over the context's rows, or over the output rows when use_output_rows != 0 (getEBV, output.jl:281-306). */
int  jwas_hip_mtj_mul_alpha(jwas_hip_ctx* ctx, int32_t trait, int32_t use_output_rows, double* out);
int  jwas_hip_mtj_end(jwas_hip_ctx* ctx);

/* ---- GBLUP: the genomic relationship matrix and the sampler on pseudo-markers (csrc/gblup.hpp) -------------------------------------
 * The relationship matrix of the context's dense n x p matrix X (Float32 or Float64, as loaded): with divisor[j] = sqrt(2 p_j (1 - p_j))
 * in the matrix's element type (the host takes the square root; the device divides, so Z = X ./ divisor is the host's Z bit for bit),
 *   K = (Z Z' + 1e-5 I) / p      (readgenotypes.jl:406-407; + 1e-5 and / p in the matrix's precision),
 * n x n values of the element type, row-major and symmetric bit for bit, formed in a device buffer that lives for the call.  Float32:
 * v_mfma_f32_32x32x2_f32 over fp32 chunks of JWAS_HIP_GRM_CHUNK markers folded into doubles; Float64: v_mfma_f64_16x16x4_f64.
 * Errors: JWAS_HIP_ESTATE without genotypes; JWAS_HIP_EUNSUP on 2-bit packed storage and on shards; JWAS_HIP_EINVAL for a divisor
 * that is not positive and finite. */
#define JWAS_HIP_GRM_CHUNK 64
int  jwas_hip_grm(jwas_hip_ctx* ctx, const void* divisor_p, void* K_host);
/* The same matrix (readgenotypes.jl:403-408) of the context's 2-bit packed genotypes (jwas_hip_load_packed2bit, jwas_hip_load_jgb2,
 * jwas_hip_plink_commit), Float32: X is what the storage decodes to (code 3 -> the marker mean; minus the mean when centered), and K is
 * bit for bit what jwas_hip_grm returns for the dense matrix of those columns -- the tiles, the fp32 chunks and their fold are the same;
 * the four possible x / divisor[j] of a marker are divided once per workgroup, by the same IEEE division.  The stray fields of a
 * marker's last byte are not read as genotypes.  The storage, the state and any open session are left untouched.
 * Errors: JWAS_HIP_EINVAL for a NULL context or argument and for a divisor that is not positive and finite; JWAS_HIP_ESTATE when the
 * context holds no 2-bit packed genotypes; JWAS_HIP_EUNSUP in a Float64 context, on shards and beyond the tile grid; JWAS_HIP_ENOMEM. */
int  jwas_hip_grm_packed2bit(jwas_hip_ctx* ctx, const float* divisor_p, float* K_host);
/* Device bytes of that call beyond the loaded matrix (pure). */
int64_t jwas_hip_grm_estimate_bytes(int64_t n, int64_t p, int32_t precision_bits);
/* The sampler (markers/BayesianAlphabet/GBLUP.jl): the context's dense matrix is n x n, column i the i-th eigenvector l_i of the
 * relationship matrix, D_i > 0 its eigenvalue; pseudo-marker i has the prior variance D_i G.  A step works on the context's own
 * residual r_k and effects alpha_k (jwas_hip_init_state with T traits, T <= 4), in double with one rounding to the element type
 * on store, the matrix read once per pass for all traits:
 *   r+_k = r_k + L alpha_k;   s_ik = l_i' r+_k;   the draw;   r_k = r+_k - L alpha_k.
 *   diagonal != 0 (one trait, or constraint = true; GBLUP!, megaGBLUP!):  lhs = 1 + vare_kk / (G_kk D_i),
 *       alpha_ik = s_ik / lhs + z sqrt(vare_kk / lhs)
 *   diagonal == 0 (MTGBLUP!):  lhs_i = inv(vare) + inv(G) / D_i,  S = inv(lhs_i),  alpha_i = S inv(vare) s_i + chol_lower(S) z_i
 * Draws: philox4x32_10(pseudo-marker, iteration, 0x03000000, 13 + 16 q) the normal of coefficient q = first_trait + k (both modes).
 * No sum of trait k depends on T and there are no floating-point atomics: trait k of a diagonal T-trait step is bit-equal to a
 * one-trait step with first_trait = k, and two runs give the same bits.  beta is set to alpha; delta and the running means are the context's.
 * Errors: JWAS_HIP_ESTATE without a residual (jwas_hip_init_state) or, after _begin, without an open session or with another number
 * of traits; JWAS_HIP_EINVAL for p != n, more than 4 traits, a D that is not positive and finite, variances that are not positive
 * (definite) and finite; JWAS_HIP_EUNSUP with residual weights, 2-bit packed storage or shards.  The session is freed by _end,
 * jwas_hip_destroy or loading genotypes. */
typedef struct jwas_gblup_params {
    uint32_t iteration;                 /* MCMC iteration >= 1 (enters the RNG counter)                                          */
    int32_t  diagonal;                  /* != 0: trait by trait from the diagonals of vare and G                                 */
    uint64_t seed;                      /* runMCMC(seed=...)                                                                     */
    uint32_t first_trait;               /* trait k draws with coefficient q = first_trait + k; first_trait + T <= 4              */
    uint32_t reserved;
    double   vare[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];      /* T x T, row-major                                         */
    double   G[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];         /* T x T the genetic (co)variance                            */
} jwas_gblup_params;
typedef struct jwas_gblup_stats {
    double alpha_ss[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];    /* T x T: sum_i alpha_ik alpha_il / D_i                     */
    double resid_ss[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS];    /* T x T: sum r_k r_l after the step                        */
    double resid_sum[JWAS_HIP_MAX_TRAITS];                         /* sum r_k                                                  */
    double step_ms;                     /* device time of the step                                                               */
} jwas_gblup_stats;
int  jwas_hip_gblup_begin(jwas_hip_ctx* ctx, const double* D_n);
int  jwas_hip_gblup_step(jwas_hip_ctx* ctx, const jwas_gblup_params* params, jwas_gblup_stats* stats);
/* The right-hand sides s of the last step: n x T doubles, row-major. */
int  jwas_hip_gblup_get_rhs(jwas_hip_ctx* ctx, int64_t nvalues, double* out);
/* Device bytes of a session (pure; an upper bound). */
int64_t jwas_hip_gblup_estimate_bytes(int64_t n, int32_t ntraits, int32_t precision_bits);
int  jwas_hip_gblup_end(jwas_hip_ctx* ctx);

/* ---- single-step analysis: imputing the genotypes of non-genotyped relatives (single_step/SSBR.jl:83-159) --------------------
 * runMCMC(...; single_step_analysis=true, pedigree=ped) orders the pedigree as [non-genotyped; genotyped] (calc_Ai, SSBR.jl:71-79)
 * and imputes, 1000 markers at a time, M_n = A^nn \ (-A^ng M_g) (impute_genotypes, SSBR.jl:83-135); the rows of [M_n; M_g] of the
 * phenotyped individuals become the matrix the sweep runs on, those of the output IDs the output matrix, both cast to the
 * genotypes' element type (SSBR.jl:137-138).  The session below does that on the device as a sparse solve with many right-hand
 * sides (csrc/ssbr.hpp): one thread per marker column walks the rows of L, then of U, in place; a thread reads only what it wrote
 * itself, so there is nothing to wait for.  A session of its own: it needs no genotype matrix to begin, and touches the context's
 * matrices only in jwas_hip_ss_impute.
 *
 * jwas_hip_ss_begin (SSBR.jl:71-79,94): the factors of A^nn as the host's sparse LU left them, Pr A^nn Pc = L U.  n_n / g: the
 * numbers of non-genotyped / genotyped individuals of the pedigree.  L and U: CSR over n_n rows, int64 row pointers, int32
 * columns STRICTLY ASCENDING within a row, double values; L unit lower triangular with its diagonal stored (the last entry of every
 * row, exactly 1), U upper triangular with its diagonal stored (the first entry, finite and not 0).  perm_r[i] = the position of
 * row i of A^nn in the permuted system, x[i] = z[perm_c[i]] brings the solution back (scipy.sparse.linalg.splu's perm_r / perm_c).
 * Ai_ng: A^ng as CSR, n_n rows, g columns.  budget_bytes: what the session may allocate -- it sizes the markers per chunk, ldc =
 * the largest multiple of 64 (at most 65 536) with jwas_hip_ss_estimate_bytes(.., ldc) <= budget_bytes, returned in *ldc_out
 * (the work matrix is 8 n_n ldc bytes, the two genotyped blocks 16 g ldc).  Everything is validated before any allocation or
 * launch: JWAS_HIP_EINVAL for unsorted or duplicate columns, indices out of range, non-finite values, a zero or non-finite U
 * diagonal, permutations that are not permutations, L not unit lower triangular, U not upper triangular; JWAS_HIP_ENOMEM when the
 * budget does not pay for one chunk of 64 markers; JWAS_HIP_EUNSUP on a context with a communicator (marker or row shards).  A
 * second call replaces the session.  The arrays are copied. */
int  jwas_hip_ss_begin(jwas_hip_ctx* ctx, int64_t n_n, int64_t g, const int64_t* L_rowptr, const int32_t* L_col, const double* L_val,
                       const int64_t* U_rowptr, const int32_t* U_col, const double* U_val, const int32_t* perm_r, const int32_t* perm_c,
                       const int64_t* Ai_ng_rowptr, const int32_t* Ai_ng_col, const double* Ai_ng_val, int64_t budget_bytes, int64_t* ldc_out);
/* The rows a chunk is written to (Z and Zo of SSBR.jl:110-111,129-130).  target 0: the context's dense sweep matrix (rows = the
 * records of the phenotype file, duplicates allowed), target 1: its output matrix (jwas_hip_load_output_dense_f32 / _f64; rows = the
 * output IDs).  prow[r] = the row of [M_n; M_g] (pedigree order, 0 .. n_n + g - 1) behind row r of the target; nrows must be the
 * target's number of rows (JWAS_HIP_EINVAL), the target must exist (JWAS_HIP_ESTATE).  Copied. */
int  jwas_hip_ss_set_rows(jwas_hip_ctx* ctx, int32_t target, int64_t nrows, const int32_t* prow);
/* One chunk (SSBR.jl:122-131): Mg = the g x count block of the genotyped individuals (pedigree order) for markers [j0, j0 + count),
 * column-major with leading dimension ldg, in the context's element type (float, or double in a Float64 context).  Uploaded,
 * transposed into double, solved, and the rows of every target that has been set are written to columns [j0, j0 + count) of that
 * matrix in its element type (data_type.(Mpheno), SSBR.jl:137-138); the pad rows of those columns are zero, other columns are not
 * touched.  Both targets have the sweep matrix's markers (an output matrix is loaded next to a sweep matrix): without a sweep matrix
 * the call returns JWAS_HIP_ESTATE.  count <= ldc (JWAS_HIP_EINVAL); no target, a target replaced by a matrix of another size, or a sweep matrix whose
 * blocks have been set up (x'x and the Grams depend on it): JWAS_HIP_ESTATE.  Synchronous. */
int  jwas_hip_ss_impute(jwas_hip_ctx* ctx, int64_t j0, int64_t count, const void* Mg, int64_t ldg);
/* Columns [j0, j0 + count) of a target as they lie in device memory: ld x count values in the context's element type, ALL ld rows --
 * the n rows and the pad rows behind them (ld = n rounded up to 256; JWAS_HIP_EINVAL when `ld` is not the target's).  For tests: the
 * other column readers return the n rows only, and the unweighted Gram tiles sum over all ld rows, so pad rows must be exactly 0. */
int  jwas_hip_ss_get_columns(jwas_hip_ctx* ctx, int32_t target, int64_t j0, int64_t count, int64_t ld, void* out);
/* The same path for a few columns, in double from end to end: out (nrows x count, column-major) = rows prow of [A^nn \ (-A^ng Mg); Mg].
 * How J is obtained -- the column whose genotyped entries are all -1 (make_JVecs, SSBR.jl:146-159) -- and how tests see the solve
 * before the cast to Float32.  Touches no matrix of the context. */
int  jwas_hip_ss_solve_host(jwas_hip_ctx* ctx, int64_t count, const double* Mg_f64, int64_t ldg, int64_t nrows, const int32_t* prow, double* out_f64);
/* Device bytes of a session with `markers_per_chunk` (rounded up to a multiple of 64) columns per chunk, the target row lists
 * (4 bytes per row) aside: 24 (n_n + 1) + 12 (nnz_l + nnz_u + nnz_a) + 8 n_n + 8 ldc (n_n + 2 g).  Pure. */
int64_t jwas_hip_ss_estimate_bytes(int64_t n_n, int64_t g, int64_t nnz_l, int64_t nnz_u, int64_t nnz_a, int64_t markers_per_chunk);
int  jwas_hip_ss_end(jwas_hip_ctx* ctx);

/* ---- the sweep ------------------------------------------------------------------------------ */
/* Time every `stride`-th k_block_step launch of subsequent sweeps with HIP events on the
 * sweep's stream (0 = off); the sums come back in jwas_sweep_stats.update_kernel_*. */
int  jwas_hip_set_kernel_timing(jwas_hip_ctx* ctx, int32_t stride);
int  jwas_hip_sweep(jwas_hip_ctx* ctx, const jwas_sweep_params* params, jwas_sweep_stats* stats);
/* Diagnostics of the LAST sweep (no reference counterpart; what JWAS_HIP_DEBUG_PHASES prints): the sampler's counters, n <= 32
 * values -- [0] effect changes, [1] Gram rows fetched on demand, [2..6] phase cycles, [7] rounds / sections walked again,
 * [16] / [17] compact-chain blocks tried / fallen back, or (section_solve) sections solved / fallen back to the walk,
 * [23] (section_solve) exceptions taken inside the solved sections, [24] hand-over words that never arrived (the sweep fails),
 * [29] ping-pong blocks staged a second time, [30] / [31] multi-trait skip and verify: blocks in which the serial wave took the
 * chain over again / 64-marker sub-blocks evaluated by a helper wave. */
int  jwas_hip_last_sweep_counters(jwas_hip_ctx* ctx, uint64_t* out, int32_t n);
/* Which schedule the LAST sweep ran (no reference counterpart).  The library picks among several kernel instantiations and
 * placements per sweep -- from the block size, the previous sweep's number of effect changes and the JWAS_HIP_* switches; all of
 * them are the same chain.  One bit per decision, so that a test can prove which variant it covered.  0 before the first sweep
 * of a chain and on Float64 contexts (one schedule). */
enum jwas_hip_schedule_flags {
    JWAS_HIP_SCHED_INDEPENDENT      = 1u << 0,   /* independent blocks (jwas_sweep_params.independent_blocks) */
    JWAS_HIP_SCHED_GROUPED          = 1u << 1,   /* grouped launches (jwas_sweep_params.group_launch took effect) */
    JWAS_HIP_SCHED_GROUP_PP_KERNEL  = 1u << 2,   /* grouped: the instantiation with ping-pong samplers / cooperative apply compiled in
                                                    (clear: the steady-state instantiation) */
    JWAS_HIP_SCHED_GROUP_PINGPONG   = 1u << 3,   /* grouped: at least one launch sampled with one workgroup per block */
    JWAS_HIP_SCHED_GROUP_COOP       = 1u << 4,   /* grouped: cooperative apply of the merged change list */
    JWAS_HIP_SCHED_QUIET_XCD        = 1u << 5,   /* at least one step launch kept workgroup ids = 0 mod 8 off the streaming work
                                                    (clear: every launch streamed on all eight XCDs) */
    JWAS_HIP_SCHED_COOP_APPLY       = 1u << 6,   /* one block per launch: cooperative apply of the block's changes */
    JWAS_HIP_SCHED_DENSE_BIG        = 1u << 7,   /* single-trait sweep under a uniform pi = 0 (the Rule D instantiation) */
    JWAS_HIP_SCHED_DENSE_MT         = 1u << 8,   /* multi-trait: at least one block sampled by the dense-walk-only instantiation */
    JWAS_HIP_SCHED_CORR_HELPER      = 1u << 9,   /* single-trait dense sweep: at least one block's lookahead correction formed by the
                                                    helper workgroup */
    JWAS_HIP_SCHED_SECTION_SOLVE    = 1u << 10,  /* Rule T section inverses were formed (jwas_sweep_params.section_solve took effect) */
    JWAS_HIP_SCHED_COMPACT_OFF_SHIFT = 11,       /* two bits: the low two bits of JWAS_HIP_COMPACT_OFF (0: the compact candidate chain) */
    JWAS_HIP_SCHED_COMPACT_OFF_MASK = 3u << 11
};
int  jwas_hip_last_sweep_schedule(jwas_hip_ctx* ctx, uint32_t* flags);

/* ---- marker shards over the GPUs of one node (one context per GPU / process) -------------------------------
 * The single-site chain is sequential in the marker index; what the reference ships for parallel blocks is
 * independent_blocks=true (BayesABC.jl:190-255): every block starts from the same residual snapshot and the residual is
 * reconciled once per sweep by r += sum_b X_b * (alpha_old_b - alpha_new_b) (BayesABC.jl:251-253).  These entry points
 * are that mode with one "block" per GPU: the context holds the rank's marker columns (marker_offset = global index of
 * its first column) and a replicated residual.
 *   jwas_hip_comm_unique_id   rank 0 creates the 128-byte RCCL id (ncclGetUniqueId) and hands it to the other ranks by
 *                             whatever means the host has (a file, a socket, MPI, torch.distributed ...);
 *   jwas_hip_comm_init        every rank joins (ncclCommInitRank on the context's device; collective);
 *   jwas_hip_sweep_sharded    jwas_hip_sweep on the own markers from the snapshot, then ON THE DEVICE, on the context's
 *                             stream: delta r = fl64(r_local) - fl64(r_snapshot) and the packed marker statistics in one
 *                             buffer, ONE ncclAllReduce(sum, fp64) over xGMI, r = fl32(r_snapshot + sum of delta r).
 *                             On return every rank holds the same residual (jwas_hip_get_residual) and `stats` holds the
 *                             ALL-RANK sums (sum_delta, alpha_ss, class / state counts, n_events ...) and the residual
 *                             statistics of the reconciled residual.  Approximate unless X_g'X_h = 0 between shards
 *                             (docs/src/manual/block_bayesc.md:95-134); world = 1 is the exact chain.
 * librccl.so is loaded on first use (dlopen); a single-GPU host never needs it. */
int  jwas_hip_comm_unique_id(void* id_out_128_bytes);
int  jwas_hip_comm_init(jwas_hip_ctx* ctx, const void* unique_id_128_bytes, int32_t rank, int32_t world);
int  jwas_hip_comm_destroy(jwas_hip_ctx* ctx);
/* Rank and size of the attached communicator as the TRANSPORT reports them (ncclCommUserRank / ncclCommCount): what a
 * host must report as its GPU count.  Without a communicator: rank 0 of 1. */
int  jwas_hip_comm_info(jwas_hip_ctx* ctx, int32_t* rank, int32_t* world);
int  jwas_hip_sweep_sharded(jwas_hip_ctx* ctx, const jwas_sweep_params* params, jwas_sweep_stats* stats);
/* ---- exact ROW shards (SURVEY 8e "exact alternative"): every rank holds a slice of the individuals and ALL markers.
 * jwas_hip_comm_row_shards(ctx, 1) after jwas_hip_comm_init and BEFORE jwas_hip_setup_blocks: x'x, the block Grams and the
 * cross-Grams are summed over the ranks at setup, every block's partial right-hand side X_b'r is summed over the ranks
 * (one small all-reduce per block launch, on the context's stream) before its sampler runs -- replicated, on identical
 * inputs, so every rank holds the same effects and its own slice of the residual.  jwas_hip_sweep then IS the exact chain
 * of the pooled data (the sums are formed in a different order than on one GPU, nothing else); r'r / sum r come back summed
 * over the ranks.  Needs the same number of 256-row groups on every rank (pad with zero rows) and the same markers.
 * jwas_hip_comm_init_loopback: test transport (both sharding modes: jwas_hip_sweep_sharded and the row shards) -- the ranks are contexts of ONE process driven by different host threads,
 * the exchange goes through host memory (slot 0..3 = one group of ranks). */
int  jwas_hip_comm_row_shards(jwas_hip_ctx* ctx, int32_t enable);
int  jwas_hip_comm_init_loopback(jwas_hip_ctx* ctx, int32_t slot, int32_t rank, int32_t world);

/* ---- multi-trait BayesA/B: the per-marker effect covariances on the device ------------------------------------------------
 * The reference redraws every marker's t x t effect covariance each iteration, G_j ~ InverseWishart(df + 1, scale + b_j b_j')
 * (sample_variance(data, 1, df, scale) per marker, variance_components.jl:181-186): O(p) small matrix draws that would
 * otherwise make the host the bottleneck.  jwas_hip_sample_marker_covariances draws all p of them on the device from the
 * CURRENT beta (Bartlett's decomposition on the counter RNG, keyed by (seed, iteration, global marker)); `df` is the
 * inverse-Wishart's degrees of freedom as passed to the distribution (the reference's df + 1), `scale` its t x t row-major
 * scale matrix.  The next jwas_hip_sweep with jwas_sweep_params.var_effect_matrix == NULL uses them in place.  Asynchronous. */
int  jwas_hip_sample_marker_covariances(jwas_hip_ctx* ctx, double df, const double* scale_txt, uint64_t seed,
                                        uint32_t iteration, uint32_t marker_offset);
int  jwas_hip_get_marker_covariances(jwas_hip_ctx* ctx, float* out_p_t_t);      /* p x t x t row-major */

/* ---- Float64 mode: runMCMC(double_precision=true) (JWAS.jl:349-366; genotypes read as Float64, readgenotypes.jl:298,345) ----
 * In that mode the reference holds EVERYTHING as Float64 -- genotypes, ycorr, alpha / beta / delta, x'x -- and its scalar
 * kernels run in Float64.  jwas_hip_set_precision(ctx, 64) BEFORE genotypes are loaded makes the context a Float64 context:
 * the data entry points below replace their Float32 namesakes (same meaning, double host arrays; delta is double 0/1, or
 * int32 classes for BayesR); jwas_hip_setup_blocks (any block size 1 .. 1024), jwas_hip_setup_blocks_explicit (blocks of at
 * most 1024 markers), jwas_hip_set_weights (the Float32 values, widened), jwas_hip_init_state, jwas_hip_sweep (reading
 * jwas_sweep_params.vare_f64 / var_effect_f64 / var_effect_vec_f64; nreps and independent_blocks as in a Float32 context),
 * jwas_hip_residual_sub_xalpha, jwas_hip_accumulate and jwas_hip_num_blocks are shared.  Samplers: single-trait BayesA/B/C,
 * BayesR, multi-trait BayesC and BayesA/B (MTBAYESC1 / C2 / B1 / B2) under Gibbs sampler I and II, with marker-specific joint
 * priors (jwas_sweep_params.log_prior_states_matrix, 2 traits); dense storage; block size x traits <= 2048.  Multi-trait
 * BayesA/B keeps its p x t x t covariances in double on the device: jwas_hip_set_marker_covariances_f64 uploads them,
 * jwas_hip_sample_marker_covariances draws them from the double beta, jwas_hip_get_marker_covariances_f64 reads them back;
 * jwas_sweep_params.var_effect_matrix (float) is refused.  The output side follows the state: jwas_hip_load_output_dense_f64 /
 * jwas_hip_mul_alpha_output_f64 (EBVs of the output rows), jwas_hip_get_alpha_sparse_f64 (a saved sample as a sparse record)
 * and jwas_hip_window_sums_f64 / jwas_hip_window_sums2_f64 (the window GWAS) are the twins of the Float32 calls, with double
 * arrays; called on a Float32 context they return JWAS_HIP_ESTATE.  Everything else of the Float32 surface (packed storage, a
 * second block size, shards, constraint = true: MEGABAYESC / MEGABAYESB, and the Float32 namesakes of the calls above) returns
 * JWAS_HIP_EUNSUP on a Float64 context. */
int  jwas_hip_set_precision(jwas_hip_ctx* ctx, int32_t bits);                     /* 32 (default) or 64 */
int  jwas_hip_load_dense_f64(jwas_hip_ctx* ctx, const double* X_host, int64_t n, int64_t p, int64_t ld_host);
int  jwas_hip_get_xpx_f64(jwas_hip_ctx* ctx, double* out_p);
int  jwas_hip_set_state_f64(jwas_hip_ctx* ctx, int32_t trait, const double* alpha, const double* beta, const void* delta);
int  jwas_hip_get_state_f64(jwas_hip_ctx* ctx, int32_t trait, double* alpha, double* beta, void* delta);
int  jwas_hip_set_residual_f64(jwas_hip_ctx* ctx, int32_t trait, const double* r_host);
int  jwas_hip_get_residual_f64(jwas_hip_ctx* ctx, int32_t trait, double* r_host);
/* out = X * alpha_k (n doubles; one fma per nonzero effect in marker order: getEBV, output.jl:281-306, T = Float64). */
int  jwas_hip_mul_alpha_f64(jwas_hip_ctx* ctx, int32_t trait, double* out_host);
/* Mi.output_genotypes in Float64 (tools4genotypes.jl:290-296 after JWAS.jl:353): n_out x p marker-major doubles with leading
 * dimension ld_host; copied.  A second call replaces the matrix; it is freed with the context. */
int  jwas_hip_load_output_dense_f64(jwas_hip_ctx* ctx, const double* X_out_host, int64_t n_out, int64_t p, int64_t ld_host);
/* out = X_out * alpha_k (n_out doubles): EBV = output_genotypes * alpha of a saved sample (output.jl:281-306); row i equals the
 * jwas_hip_mul_alpha_f64 value of the training row it was copied from, bit for bit. */
int  jwas_hip_mul_alpha_output_f64(jwas_hip_ctx* ctx, int32_t trait, double* out_host);
/* One saved marker-effect sample as (marker index, value) lists in marker order instead of the dense row of p values
 * (output.jl:443-526).  *nnz is filled even when the lists do not fit `capacity` (JWAS_HIP_EINVAL: grow and call again). */
int  jwas_hip_get_alpha_sparse_f64(jwas_hip_ctx* ctx, int32_t trait, int64_t capacity, int32_t* idx, double* val, int64_t* nnz);
/* jwas_hip_window_sums / jwas_hip_window_sums2 with T = Float64: the reference forms X*alpha in the element type of
 * output_genotypes (GWAS.jl:148,152-165,199-217), Float64 after double_precision=true.  Same CSR description and outputs;
 * use_output_rows != 0: the rows of jwas_hip_load_output_dense_f64. */
int  jwas_hip_window_sums_f64(jwas_hip_ctx* ctx, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx,
                              const double* val, double* out_sum, double* out_ss);
int  jwas_hip_window_sums2_f64(jwas_hip_ctx* ctx, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx,
                               const double* val1, const double* val2, double* out_sum1, double* out_ss1, double* out_sum2,
                               double* out_ss2, double* out_cross);
/* jwas_hip_gwas_sample with T = Float64 (GWAS.jl:148-173): double effects over a Float64 context's matrices; bit-identical to
 * jwas_hip_window_sums_f64.  JWAS_HIP_ESTATE on a Float32 context. */
int  jwas_hip_gwas_sample_f64(jwas_hip_ctx* ctx, int32_t nnz, const int32_t* idx, const double* val, double* out_sum, double* out_ss);
int  jwas_hip_get_posterior_f64(jwas_hip_ctx* ctx, int32_t trait, double* mean_alpha, double* mean_alpha2, double* mean_delta);
int  jwas_hip_set_marker_covariances_f64(jwas_hip_ctx* ctx, const double* p_t_t);   /* p x t x t row-major */
int  jwas_hip_get_marker_covariances_f64(jwas_hip_ctx* ctx, double* out_p_t_t);

/* ---- posterior accumulators (output.jl:568-577) ---------------------------------------------- */
int  jwas_hip_accumulate(jwas_hip_ctx* ctx, double nsamples);
int  jwas_hip_get_posterior(jwas_hip_ctx* ctx, int32_t trait, float* mean_alpha, float* mean_alpha2, float* mean_delta);

#ifdef __cplusplus
}
#endif
#endif
