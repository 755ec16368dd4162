// ctx.hpp -- the context behind the C ABI (include/jwas_hip.h) and the host plumbing its units share: jwas_hip.hip and the session
// units (session_*.hip, each with its own kernels header).  Host code only, no kernel.  What crosses units is JW_LOCAL (hidden):
// the library exports the entry points of include/jwas_hip.h and nothing more.
#pragma once
#include "../../include/jwas_hip.h"
#include "device_util.hpp"      // (the sessions' limits and codes; it defines no kernel either)

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

namespace jw { struct Events; struct DevParams; }          // kernels.hpp   (the sweep's: jwas_hip.hip only)
namespace jw64 { struct Events64; struct Params64; }       // f64_path.hpp  (likewise)

#define JW_LOCAL __attribute__((visibility("hidden")))

// An owner of device allocations: release() frees what alloc() made, so a buffer cannot be added to a session and forgotten in its
// free function.  Plain data: nothing is freed implicitly.
struct JW_LOCAL DevOwner {
    std::vector<void*> ptrs;
    template <class T>
    hipError_t alloc(T** p, size_t bytes)
    {
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) ptrs.push_back((void*)*p);
        return e;
    }
    template <class T>
    void free_one(T*& p)                                   // (NULL, or not this owner's: nothing is freed)
    {
        auto at = std::find(ptrs.begin(), ptrs.end(), (void*)p);
        if (at != ptrs.end()) { ptrs.erase(at); (void)hipFree((void*)p); }
        p = nullptr;
    }
    template <class S>
    static void reset(S& session) { session.mem.release(); session = S(); }       // the free function of a session struct
    void adopt(DevOwner& other) { for (void* q : other.ptrs) ptrs.push_back(q); other.ptrs.clear(); }
    void release() { for (void* q : ptrs) (void)hipFree(q); ptrs.clear(); }
};

// The marker state of a session with a sweep of its own (Rrm, Mega): alpha, beta, delta and their running means (of alpha, alpha^2
// and the model frequency), each [rows][p] doubles.  Plain data; marker_state.hpp has what is done with it.
struct MarkerState {
    double *alpha = nullptr, *beta = nullptr, *delta = nullptr;
    double *mean_a = nullptr, *mean_a2 = nullptr, *mean_d = nullptr;
};

// What the sessions that sweep blocks of markers with mega.hpp's update kernel hold alike (Mega, Mtj; block_session.hpp has what is
// done with it): a sweep of their own with their own residuals and state, all double, on the context's genotypes.  Plain data.
struct BlockSession {
    bool active = false;
    int nt = 0, bs = 0;                                     // traits, block size
    int64_t nblocks = 0, row_cap = 0;
    DevOwner mem;
    double* R = nullptr;                                    // [nt][ld] the residuals (pad rows 0)
    double* xpx = nullptr;                                  // [p]
    double* gram = nullptr;                                 // [nblocks][bs][bs]
    MarkerState ms;                                         // [nt][p]
    double* partials = nullptr;                             // [nslices][nt][bs]
    double* par = nullptr;                                  // the parameters of the running sweep
    double* stat = nullptr;                                 // the sweep's statistics | the residual sums per slice
    double* row = nullptr;                                  // [row_cap] X alpha_k
    void* ev = nullptr;                                     // jwg::Events: the change lists of the last sampled block
    std::vector<double> par_host;                           // what par was filled from (kept until the sweep has finished)
};

// What exists once per precision, under one name in both: the Float32 context holds a Side<float> (as its base: c->alpha), a Float64
// context a Side<double> besides (c->f64->alpha); side<T>(c) picks one.  Two owners: chain_mem for what jwas_hip_init_state replaces,
// load_mem for what a load of genotypes replaces; dropping is release() and a value reset, so no member can be forgotten in a free list.
template <class T>
struct ChainState {
    DevOwner chain_mem;
    T *alpha = nullptr, *beta = nullptr;        // [t][p]
    void* delta = nullptr;                      // T [t][p], or int32 [p] (BayesR classes)
    T *mean_a = nullptr, *mean_a2 = nullptr, *mean_d = nullptr;
    T* var_vec = nullptr;                       // [p] BayesB
    T* var_mat = nullptr;                       // [p][t][t] per-marker effect covariances (multi-trait BayesA/B)
    T* ginv_mat = nullptr;                      // [p][t][t] their inverses
    bool var_mat_resident = false;              // var_mat holds this chain's covariances (uploaded or drawn on the device)
    void drop_chain() { chain_mem.release(); *this = ChainState(); }
};
template <class T>
struct Side : ChainState<T> {
    typedef T real;
    DevOwner load_mem;
    T* X = nullptr;                             // [p][ld] dense genotypes, marker-major (NULL: none, or 2-bit packed storage)
    T* r = nullptr;                             // [2][kMaxT][ld] residuals, ping-pong; buffer 0 is current between sweeps
    T* w = nullptr;                             // [ld] residual weights R^-1 (ones unless jwas_hip_set_weights; pad rows 0)
    bool weighted = false;                      // w differs from ones
    T* xpx = nullptr;                           // [p]
    T* Xout = nullptr;                          // [p][ld_out] output (EBV) rows: Mi.output_genotypes (tools4genotypes.jl:290-296)
    int64_t n_out = 0, ld_out = 0;
    int32_t* cmp_idx = nullptr;                 // [p] + [1] compacted nonzero effects of one trait (k_compact_alpha) and their number
    T* cmp_val = nullptr;                       // [p]
    void drop() { this->chain_mem.release(); load_mem.release(); *this = Side(); }
};

struct jwas_hip_ctx : Side<float> {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    int64_t n = 0, p = 0, ld = 0;
    int nslices = 0;                    // 256-row slices
    int upd_nslices = 0;                // slices of the UPDATE role: = nslices (dense), 1024-row slices on 2-bit packed storage (update_role_wide)
    int nrg = 0, ncg = 1;               // k_update_partial grid: row groups x column groups
    int spg = 8;                        // slices per row group
    uint8_t* Q = nullptr;               // the reference's 2-bit packed storage [p][ld/4] + per-marker means, in the place of the dense X
    float* qmean = nullptr;
    bool packed = false;
    int centered = 1;
    // Output rows in 2-bit packed form beside packed training storage (jwas_hip_load_output_packed2bit, jwas_hip_plink_commit_output):
    // [p][ld_out / 4], no means of its own -- decoded with qmean / centered above; n_out, ld_out: the base's.  At most one of Xout and
    // Qout is set.  load_mem owns it, and the union list of jwas_hip_ebv_output below.
    uint8_t* Qout = nullptr;
    int32_t* ebv_idx = nullptr;         // [p] + [1] the markers with a nonzero effect in any trait, ascending, and their number
    float* ebv_val = nullptr;           // [kMaxT][p] their effects, trait-major (0 where only another trait's is nonzero)

    // Active block configuration (a view of one entry of `sets`; several block sizes can be resident so the host
    // can pick per sweep: big blocks when few markers change, smaller ones when many do).
    struct BlockSet {
        int bs; int64_t nblocks; float *gram, *cross, *corr; double* partials;
        // grouped launches (jwas_hip_setup_groups; k_group_step): gm = 2 or 4 blocks per launch (0: not set up); gcross[0]: cross-Grams
        // of consecutive PAIRS of blocks (2 bs markers: pair q at q (2 bs)^2, rows = markers of pair q-1), gcross[1] (gm = 4): of
        // consecutive groups of four; gcbuf: the corrections [2][gm bs] cG | [2][bs] cW | [2 bs] cP | [bs] zeros; gidx / gdelta:
        // [2][gm bs] the merged change lists of a group (ping-pong; header lines: ctx.ev[parity])
        int gm; float* gcross[2]; float* gcbuf; int32_t* gidx; float* gdelta;
        unsigned long long* gpp;        // tagged hand-over words of the ping-pong samplers (SamplerArgs::pp_*, GroupArgs::pp_*): (6 + 3 gm) bs + 8
    };
    unsigned pp_epoch = 0;              // tag of the last ping-pong launch (31 bits, never 0: a word of the zeroed buffer matches no launch)
    int set_index = 0;                  // entry of `sets` that is selected
    std::vector<BlockSet> sets;
    std::vector<int64_t> starts;        // explicit block starts (nblocks + 1 entries, last = p), empty = uniform blocks
    int64_t* d_starts = nullptr;        // ... on the device
    int block_size = 0;
    int64_t nblocks = 0;
    float* gram = nullptr;
    float* cross = nullptr;             // cross-Grams X_{b-1}'X_b, block b at offset b*bs*bs (block 0 unused)
    float* corr = nullptr;              // [2][kMaxT][bs] lookahead corrections (ping-pong: read by launch k, written for k+1)

    int method = -1, ntraits = 0;
    double* partials = nullptr;
    jw::Events* ev = nullptr;               // [2]
    // independent-block mode (allocated on first use)
    double* ipartials = nullptr;        // [nblocks][t][nrg][bs]
    jw::Events* ev_all = nullptr;           // [nblocks] per-block change lists
    int32_t* ev_offs = nullptr;         // [nblocks + 1] exclusive scan of the counts; [nblocks] = total
    int32_t* idx_all = nullptr;         // [p] compacted change list, (block, marker) order
    float* delta_all = nullptr;         // [kMaxT][p]
    int ind_traits = 0;
    jw::DevParams* dparams = nullptr;
    unsigned long long* counters = nullptr;
    double* fin_out = nullptr;          // [nslices][kMaxT*kMaxT + kMaxT]
    int* sync_cnt = nullptr;            // [2][nrg] arrival counters of the update role's cooperative dense apply
    double* stat_out = nullptr;         // [kStatGrid][kNStat]
    double* host_buf = nullptr;         // pinned staging for fin_out + stat_out + counters
    double* prep_d = nullptr;           // [kPrepD][p] per-sweep marker constants (k_prepare)
    float*  prep_f = nullptr;           // [kPrepF][p]
    double* mt2_tab = nullptr;          // sampler II, <= 3 traits: [2^t * (t(t+1)/2 + 1)][p] state tables
    float*  tsec = nullptr;             // Rule T (section_solve): the section inverses of the current sweep, [sections][(64 t)^2]
    size_t  tsec_cap = 0;               // ... capacity in floats
    unsigned long long* xch = nullptr;  // Rule T: [kMaxT][256] {value, tag} words: the sampler workgroup's hand-over to the helper workgroup
    int     xch_epoch = 0;              // ... grows by 8 per launch
    double* pi_vec = nullptr;
    double* pi_mat = nullptr;
    double* lpr_mat = nullptr;          // p x 2^t marker-specific multi-trait log priors
    bool    lpr_active = false;         // ... in use by the current sweep
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    hipEvent_t ev_hand = nullptr;       // jwas_hip_residual_handover: recorded on this context's stream only (no timing)
    int timing_stride = 0;
    double last_events = -1.0;          // effect changes of the previous sweep (-1: none yet)
    static constexpr int kCounters = 32;                    // = jw::kNCounters of kernels.hpp (jwas_hip.hip asserts it)
    static constexpr int64_t kRowPad = 256;                 // = jw::kSliceRows: ld is n rounded up to it (likewise)
    unsigned long long last_counters[kCounters] = {};       // the sampler's diagnostics counters of the previous sweep
    uint32_t last_schedule = 0;         // JWAS_HIP_SCHED_* bits of the last sweep sweep_enqueue put on the stream
    double event_overhead_ms = 0.0;     // mean HIP-event interval around an empty launch (calibration)
    std::vector<hipEvent_t> kev;        // pairs of events around sampled k_update_partial launches
    // marker-shard reconcile (jwas_hip_comm_init / jwas_hip_sweep_sharded): RCCL communicator on this context's device
    void* comm = nullptr;               // ncclComm_t
    int comm_rank = 0, comm_world = 1;
    float* r_snap = nullptr;            // [kMaxT][ld] residual snapshot of the running sweep
    double* shard_buf = nullptr;        // [kMaxT*ld + kShardStats] delta r (fp64) + packed marker statistics: ONE all-reduce
    // exact ROW shards (jwas_hip_comm_row_shards): this context holds a slice of the individuals and ALL markers; x'x, the
    // Grams and every block's partial RHS are summed over the ranks, the sampler then runs replicated
    bool row_mode = false;
    int loop_slot = -1;                 // >= 0: loopback transport (ranks = contexts of one process on different host threads)
    double* row_buf = nullptr;          // [32] small exchanges
    // Float64 mode (runMCMC(double_precision=true); csrc/f64_path.hpp): its own storage / state, created by jwas_hip_set_precision
    struct F64 : Side<double> {
        double* gram = nullptr;             // [nblocks][bs][bs]
        double* partials = nullptr;         // [kMaxT][nslices][bstride]  (independent blocks: one such set per block)
        size_t partials_cap = 0;            // ... in doubles
        jw64::Events64* ev = nullptr;       // [2]  (independent blocks: ev_all, one per block)
        jw64::Events64* ev_all = nullptr;
        int64_t ev_all_cap = 0;
        jw64::Params64* dparams = nullptr;
        std::vector<int64_t> starts;        // block starts (nblocks + 1 entries, 0-based): uniform or explicit partition
        int bstride = 0;                    // largest block of the partition, rounded up to a multiple of 8
        bool explicit_part = false;
    };
    F64* f64 = nullptr;
    // GWAS session (jwas_hip_gwas_begin .. jwas_hip_gwas_end; GWAS.jl:149-173): everything a saved sample needs stays resident
    struct Gwas {
        bool active = false, local_ebv = false, out_rows = false;
        int nwin = 0, wpc = 1, nchunks = 0, nsl = 0;       // launch geometry: grid = (nsl, nchunks), wpc windows per chunk
        int64_t n_rows = 0, ld = 0, nsamples = 0;
        const void* mat = nullptr;                          // the matrix the session was begun on (a reload ends the session)
        int32_t *cs = nullptr, *ce = nullptr;               // [nwin] column ranges
        int32_t *lo = nullptr, *hi = nullptr;               // [nwin + 1] the sample's list slice of every entry
        int32_t* idx = nullptr; void* val = nullptr;        // [cap] the sample's nonzero effects (float | double)
        int64_t cap = 0;
        double *part = nullptr, *out = nullptr;             // [nwin + 1][nsl][2] slice partials, [2][nwin + 1] sums
        double* acc = nullptr;                              // [nwin][ld] running sum of the local EBVs (window-major)
        double* host_out = nullptr;                         // pinned [2][nwin + 1]
    } gw;
    // Liability state of threshold / censored traits (jwas_hip_liability_begin .. _end; categorical_and_censored_trait.jl)
    struct Liab {
        bool active = false, inited = false;
        int nt = 0, nparts = 0;
        DevOwner mem;                                       // every device buffer below
        int kind[jwl::kMaxT] = {}, ncat[jwl::kMaxT] = {};
        void* y[jwl::kMaxT] = {};                           // [ld] liabilities, the context's element type
        int32_t* codes[jwl::kMaxT] = {};                    // [n] categories (0 = missing)
        double *lower[jwl::kMaxT] = {}, *upper[jwl::kMaxT] = {};      // [n] bounds of a censored trait
        double* thr = nullptr;                              // [kMaxT][kMaxThr] threshold tables (device) ...
        double thr_host[jwl::kMaxT][jwl::kMaxThr] = {};     // ... and their host copy
        double* part[jwl::kMaxT] = {};                      // [nparts][kMM] per-workgroup {max, min} of every category
        bool part_valid[jwl::kMaxT] = {};                   // ... left by the last draw and still describing the liabilities
        double* mm = nullptr;                               // [kMM] reduced
    } lb;
    // Location parameters (jwas_hip_locpar_begin .. _end; MCMC_BayesianAlphabet.jl:193-220, solver.jl:143-162; csrc/locpar.hpp)
    struct Locpar {
        struct Term {
            int trait = 0, group = -1, pos = 0, G = 1, npieces = 0;
            int64_t nlevels = 0, off = 0, nin = 0;
            double* x = nullptr;                            // [n] covariate values (NULL: ones)
            int32_t* level = nullptr;                       // [n] level of every record, -1 = none (NULL: all records in level 0)
            int32_t* rec = nullptr;                         // [nin] records sorted by (level, record) (NULL: 0 .. n - 1)
            double* wx = nullptr;                           // [nin] w x in that order
            int32_t *piece_lo = nullptr, *level_piece = nullptr;      // [npieces + 1], [nlevels + 1]
            double* d = nullptr;                            // [nlevels] sum w x^2
        };
        struct Group { int nmembers = 0; int term[jwp::kMaxT] = {}; int64_t nlevels = 0; };
        struct Structure {                                  // jwas_hip_lp_set_group_structure: V of a random effect, coloured
            bool set = false;
            int64_t nlevels = 0, nnz = 0;
            int ncolors = 0, nwg = 0;                       // nwg: workgroups of k_locpar_quad_rows
            std::vector<int32_t> color;                     // [nlevels] colour of every level
            std::vector<int32_t> color_lo, nshort;          // colour c: lv[color_lo[c] .. color_lo[c + 1]), its first nshort[c] the short rows
            int64_t* rowptr = nullptr;                      // [nlevels + 1]
            int32_t* col = nullptr;                         // [nnz]
            double* val = nullptr;                          // [nnz]
            int32_t* lv = nullptr;                          // [nlevels] the levels colour by colour
            double* qpart = nullptr;                        // [nwg][kMaxPairs]
            DevOwner mem;                                   // the five device buffers above (a structure may be replaced)
        };
        bool active = false, finalized = false;
        int nt = 0, ngroups = 0;
        DevOwner mem;                                       // the terms' buffers and the session's own (not the structures')
        std::vector<double> w_host;                         // [n] the residual weights in force at _begin
        std::vector<Term> terms;
        Group groups[jwp::kMaxGroups];
        Structure structs[jwp::kMaxGroups];
        int64_t q = 0;                                      // entries of sol
        double *sol = nullptr, *mean = nullptr, *mean2 = nullptr;     // [q]
        double *part = nullptr, *delta = nullptr;           // [max npieces], [max nlevels] scratch of the running term
        double* part2 = nullptr;                            // [max npieces] the piece sums of D under per-record weights (first such step)
        int64_t maxp = 1;
        int64_t* cross_offs = nullptr;                      // [kMaxGroups][16][2] member offsets of every cross-product
        double* cross_out = nullptr;                        // [kMaxGroups][16]
    } lp;
    // Multi-trait records that miss some traits (jwas_hip_mtmiss_begin .. _end; residual.jl:2-73; csrc/mtmiss.hpp)
    struct Mtmiss {
        bool active = false, weights = false;               // weights: jwas_hip_locpar_step uses the per-record Ri
        int nt = 0;
        DevOwner mem;
        int32_t* code = nullptr;                            // [n] the pattern of every record
        double* tab = nullptr;                              // [3][kMaxCodes * 16] the tables B, U, C (each [2^t][t][t] at its start)
    } mt;
    // Marker-annotation priors (jwas_hip_annot_begin .. _end; MCMC/annotation_updates.jl; csrc/annot.hpp).  The table lives in
    // pi_vec / pi_mat / lpr_mat above: where the sweep reads it.
    struct Annot {
        bool active = false;
        int kind = 0, nsteps = 0, K = 0, npieces = 0;
        DevOwner mem;                                       // (not the table: it belongs to the context and outlives the session)
        double* D = nullptr;                                // [K - 1][p] the design matrix without its column of ones
        double *liab = nullptr, *mu = nullptr;              // [nsteps][p]
        double* e = nullptr;                                // [p] the latent residual of the running step
        double *part = nullptr, *part4 = nullptr;           // [npieces][3] piece sums of a coefficient, [npieces][4] of the table's columns
        double* scal = nullptr;                             // coef [3][K] | n_A [3] | column means [4] | c_k - c_k' [1] | dsq [K]
        double *mean = nullptr, *mean2 = nullptr;           // [table size] running means of the prior probabilities
    } an;
    // Structural equation model (jwas_hip_sem_begin .. _end; structure_equation_model/SEM.jl; csrc/sem.hpp)
    struct Sem {
        bool active = false;
        int nt = 0, G = 0;
        DevOwner mem;
        uint32_t mask = 0, ymask = 0, rmask = 0;            // bit cell(i, j): cs[i][j]; bit k: trait k is a parent / has parents
        double* y = nullptr;                                // [nt][n] the phenotypes
        double* part = nullptr;                             // [G][kGramCells] workgroup partials (the step uses kMaxPairs of every row)
        double* S = nullptr;                                // [16] y y'
        double* rec = nullptr;                              // [kRecSize] lambda | d | mu | C
        double* acc = nullptr;                              // [2][3][nt][p] indirect | overall: mean, mean of squares, frequency
    } sm;
    // Random regression model (jwas_hip_rrm_begin .. _end; RRM/RRM.jl, RRM/MCMC_BayesianAlphabet_RRM.jl; csrc/rrm.hpp): a sweep of its
    // own with its own residual and state, all double, on the context's genotypes
    struct Rrm {
        bool active = false;
        int T = 0, C = 0, bs = 0;                           // time points, coefficients per marker, block size
        int64_t nblocks = 0;
        DevOwner mem;
        std::vector<uint64_t> mask_host;                    // [n] bit t: the individual has a record at time t
        uint64_t* mask = nullptr;                           // [ld] (pad rows 0)
        double* phi = nullptr;                              // [T][C]
        double* O = nullptr;                                // [cells][ld] O_i = sum_t m_it phi_t phi_t'
        double* W = nullptr;                                // [T][ld] the residual, 0 at every unobserved cell
        double* M = nullptr;                                // [p][cells]
        double* gram = nullptr;                             // [nblocks][bs][bs][cells]
        MarkerState ms;                                     // [C][p]
        double* partials = nullptr;                         // [nslices][bs C]
        double* stat = nullptr;                             // [kStSize] the sweep's statistics | [nslices] sum W^2 per slice
        double* row = nullptr;                              // [ld] X alpha_q
        void* ev = nullptr;                                 // jwr::Events: the change list of the last sampled block
    } rr;
    // Mega-trait model (jwas_hip_mega_begin .. _end; markers/BayesianAlphabet/BayesABC.jl:1-58; csrc/mega.hpp): T independent
    // single-trait chains over the context's genotypes, a sweep of its own with its own residuals and state, all double
    struct Mega : BlockSession {
        uint32_t first_trait = 0;                           // the trait id of trait 0 in the RNG counter
        int64_t mask_words = 0;
        std::vector<uint8_t> miss_host;                     // [nt][n] 1: the cell is missing (empty: none)
        uint32_t* mask = nullptr;                           // [nt][ld / 32] bit i: record i misses the trait
        // par: [kParSize][nt] the per-trait parameters; stat: [nt][kStSize] | [nt][nslices][2] sum r^2, sum r per slice
        // BayesR chains (jwas_hip_mega_sweep_r) and the PSRF of the chains: allocated at their first call
        double* par_r = nullptr;                            // [kParRSize][nt]
        double* stat_r = nullptr;                           // [nt][kStRSize] | [nt][nslices][2]
        double* psrf = nullptr;                             // [p]
    } mg;
    // Unconstrained multi-trait BayesC with 5 to 8 traits (jwas_hip_mtj_begin .. _end; markers/BayesianAlphabet/MTBayesABC.jl:57-127;
    // csrc/mtjoint.hpp): Gibbs sampler I on the block form of the mega-trait session, a sweep of its own with its own residuals and
    // state, all double.  par: [kParSize] Rinv | Ginv | log pi; stat: [kStSize] | [nslices][kFinSize] residual sums per slice
    struct Mtj : BlockSession {
    } mj;
    // Single-step imputation (jwas_hip_ss_begin .. _end; single_step/SSBR.jl:83-159; csrc/ssbr.hpp): the factors of A^nn, A^ng and the
    // chunk buffers of a sparse solve with many right-hand sides.  It is bound to no matrix: the targets are checked at every chunk.
    struct Ssbr {
        bool active = false;
        int64_t nn = 0, g = 0, ldc = 0;                     // non-genotyped, genotyped, markers per chunk
        int64_t nnz_l = 0, nnz_u = 0, nnz_a = 0;
        DevOwner mem;
        int64_t *Lp = nullptr, *Up = nullptr, *Ap = nullptr;          // [nn + 1]
        int32_t *Lc = nullptr, *Uc = nullptr, *Ac = nullptr;
        double *Lv = nullptr, *Uv = nullptr, *Av = nullptr;
        int32_t *rsrc = nullptr, *perm_c = nullptr;         // [nn] the inverse of perm_r, perm_c
        double *Gt = nullptr, *W = nullptr;                 // [g][ldc], [nn][ldc]
        void* stage = nullptr;                              // [ldc][g] doubles: the uploaded block before its transpose
        int32_t* prow[2] = {};                              // the rows of [M_n; M_g] behind the rows of target 0 (sweep matrix), 1 (output)
        int64_t nrows[2] = {};                              // (0: the target is not set)
    } ss;
    // GBLUP (jwas_hip_gblup_begin .. _end; markers/BayesianAlphabet/GBLUP.jl; csrc/gblup.hpp): the context's dense n x n matrix holds the
    // eigenvectors of the relationship matrix; a step runs on the context's own residual and effects
    struct Gblup {
        bool active = false;
        int nt = 0, nparts = 0, len = 0, nwg = 0;           // traits; column parts of a pass and their length; workgroups of the sampler
        const void* mat = nullptr;                          // the matrix the session was begun on
        DevOwner mem;
        double* D = nullptr;                                // [n] eigenvalues
        void* rplus = nullptr;                              // [nt][ld] r + L alpha, the context's element type
        double* s = nullptr;                                // [n][nt] the right-hand sides of the last step
        double* part = nullptr;                             // [nparts][nt][ld] column-part sums of L alpha
        double* par = nullptr;                              // [kParSize] the parameters of the running step
        double* stat = nullptr;                             // [nwg][nt nt] | [nslices][nt nt + nt]
    } gb;
    // A scanned PLINK .bed file that waits for its commit (jwas_hip_plink_scan .. _commit / _discard; csrc/plink.hpp): every file
    // marker transcoded to 2-bit codes in the layout of packed storage.  It is bound to no matrix; any load or allocation drops it.
    struct Plink {
        bool pending = false;
        int64_t n_rows = 0, p_file = 0, ld = 0;             // kept individuals, file markers, n_rows rounded up to kRowPad
        DevOwner mem;
        uint8_t* stage = nullptr;                           // [p_file][ld / 4] (+ 1 KB, as packed storage has)
    } pk;
};

// ---- errors ------------------------------------------------------------------------------------------------------------------------
JW_LOCAL int fail(jwas_hip_ctx* ctx, int code, const char* fmt, ...);      // (jwas_hip.hip; ctx == NULL: the creating thread's message)

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((ctx), JWAS_HIP_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                       \
    } while (0)

#define NEED(ctx, cond, code, ...)                                                                 \
    do { if (!(cond)) return fail((ctx), (code), __VA_ARGS__); } while (0)

#define IS_F64(c) ((c)->f64 != nullptr)
#define NOT_F64(c, what) NEED(c, !IS_F64(c), JWAS_HIP_EUNSUP, "%s is not available in a Float64 context (double_precision=true)", what)
#define ONLY_F64(c) NEED(c, IS_F64(c), JWAS_HIP_ESTATE, "this entry point needs a Float64 context (jwas_hip_set_precision(ctx, 64))")

#define HAVE_STORAGE(c) ((c)->X != nullptr || (c)->Q != nullptr)      // (of a Float32 context)
#define NEED_TRAIT(c, trait)                                                                       \
    NEED(c, c->method >= 0, JWAS_HIP_ESTATE, "jwas_hip_init_state has not been called");           \
    NEED(c, trait >= 0 && trait < c->ntraits, JWAS_HIP_EINVAL, "trait %d outside [0,%d)", trait, c->ntraits)

static inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// f(T{}) with T the context's element type: one launch of k<T> instead of a float / double pair
template <class F>
static void with_real(jwas_hip_ctx* c, F&& f) { if (IS_F64(c)) f(double{}); else f(float{}); }

// f(std::integral_constant<int, NT>{}) with NT = t, a context's number of traits: one launch of k<NT> instead of a ladder over t.
// jwas_hip_init_state admits 1 .. JWAS_HIP_MAX_TRAITS and nothing else reaches a sweep.
template <class F>
static void with_traits(int t, F&& f)
{
    static_assert(JWAS_HIP_MAX_TRAITS == 4, "one arm per number of traits");
    if (t == 1) f(std::integral_constant<int, 1>{});
    else if (t == 2) f(std::integral_constant<int, 2>{});
    else if (t == 3) f(std::integral_constant<int, 3>{});
    else if (t == 4) f(std::integral_constant<int, 4>{});
}

// the context's half of element type T (double: of a Float64 context only)
template <class T> static inline Side<T>& side(jwas_hip_ctx* c);
template <> inline Side<float>& side<float>(jwas_hip_ctx* c) { return *c; }
template <> inline Side<double>& side<double>(jwas_hip_ctx* c) { return *c->f64; }

// f(S) with S the half of the context's own precision
template <class F>
static auto on_side(jwas_hip_ctx* c, F&& f) { return IS_F64(c) ? f(side<double>(c)) : f(side<float>(c)); }

// Members of that half as the sessions read them, in the context's element type.
static inline void* residual_ptr(jwas_hip_ctx* c) { return on_side(c, [](auto& S) { return (void*)S.r; }); }      // [kMaxT][ld] (NULL: no genotypes loaded)
static inline const void* genotypes_ptr(jwas_hip_ctx* c) { return on_side(c, [](auto& S) { return (const void*)S.X; }); }      // the dense matrix (NULL: none, or packed)
static inline bool is_weighted(jwas_hip_ctx* c) { return on_side(c, [](auto& S) { return S.weighted; }); }
static inline void* alpha_ptr(jwas_hip_ctx* c) { return on_side(c, [](auto& S) { return (void*)S.alpha; }); }
static inline void* beta_ptr(jwas_hip_ctx* c) { return on_side(c, [](auto& S) { return (void*)S.beta; }); }
// the output rows (NULL: none loaded), their number and leading dimension
static inline const void* output_rows_ptr(jwas_hip_ctx* c, int64_t* n_out, int64_t* ld_out)
{
    return on_side(c, [&](auto& S) { *n_out = S.n_out; *ld_out = S.ld_out; return (const void*)S.Xout; });
}

// t x t inverse (t <= JWAS_HIP_MAX_TRAITS): Gauss-Jordan in double with partial pivoting, rounded to the element type at the end (float: it
// stands in for Julia's inv(::Matrix{Float32}), MTBayesABC.jl:66-67).  Same operation sequence as the oracle's.
template <class T>
static int inv_small(const T* A, int t, T* Ainv)
{
    double M[JWAS_HIP_MAX_TRAITS][2 * JWAS_HIP_MAX_TRAITS];
    for (int i = 0; i < t; ++i)
        for (int j = 0; j < t; ++j) { M[i][j] = A[i * t + j]; M[i][t + j] = (i == j); }
    for (int c = 0; c < t; ++c) {
        int piv = c;
        for (int i = c + 1; i < t; ++i) if (std::fabs(M[i][c]) > std::fabs(M[piv][c])) piv = i;
        if (M[piv][c] == 0.0) return -1;
        if (piv != c) for (int j = 0; j < 2 * t; ++j) { double tmp = M[c][j]; M[c][j] = M[piv][j]; M[piv][j] = tmp; }
        const double d = M[c][c];
        for (int j = 0; j < 2 * t; ++j) M[c][j] /= d;
        for (int i = 0; i < t; ++i) if (i != c) {
            const double f = M[i][c];
            if (f != 0.0) for (int j = 0; j < 2 * t; ++j) M[i][j] -= f * M[c][j];
        }
    }
    for (int i = 0; i < t; ++i) for (int j = 0; j < t; ++j) Ainv[i * t + j] = (T)M[i][t + j];
    return 0;
}

// ---- what the sessions share -------------------------------------------------------------------------------------------------------
// Each session frees what it owns and value-resets its struct (DevOwner::reset); free_storage (jwas_hip.hip) calls all of them.
JW_LOCAL void liab_free(jwas_hip_ctx* c);
JW_LOCAL void locpar_free(jwas_hip_ctx* c);
JW_LOCAL void mtmiss_free(jwas_hip_ctx* c);
JW_LOCAL void annot_free(jwas_hip_ctx* c);
JW_LOCAL void sem_free(jwas_hip_ctx* c);
JW_LOCAL void rrm_free(jwas_hip_ctx* c);
JW_LOCAL void mega_free(jwas_hip_ctx* c);
JW_LOCAL void mtj_free(jwas_hip_ctx* c);
JW_LOCAL void ss_free(jwas_hip_ctx* c);
JW_LOCAL void gblup_free(jwas_hip_ctx* c);
JW_LOCAL void gwas_free(jwas_hip_ctx* c);                                  // (output.hip: the GWAS session)
JW_LOCAL void plink_free(jwas_hip_ctx* c);                                 // (a pending scan: it goes with any load, too)

// The output rows of a Float32 context go, dense or packed, and with them a GWAS session that runs on them (the stream is idle).
static inline void drop_output_rows(jwas_hip_ctx* c)
{
    if (c->gw.out_rows) gwas_free(c);
    c->load_mem.free_one(c->Xout);
    c->load_mem.free_one(c->Qout);
    c->n_out = c->ld_out = 0;
}

// Storage of an n x p matrix and everything sized by it (jwas_hip.hip); whatever the context held before is freed first.  adopt: a
// buffer of (ld / 4) p + 1024 bytes that becomes the packed payload in the place of a new allocation (the context owns it from here on,
// also when the call fails).
JW_LOCAL int alloc_storage(jwas_hip_ctx* c, int64_t n, int64_t p, bool packed = false, uint8_t* adopt = nullptr);

// `words` ("liabilities", "annotation priors", ...) are not driven from a context that holds a marker or row shard
static inline int refuse_shards(jwas_hip_ctx* c, const char* words)
{
    NEED(c, !c->comm && !c->row_mode && c->loop_slot < 0, JWAS_HIP_EUNSUP, "%s are not driven from marker or row shards", words);
    return JWAS_HIP_OK;
}

// what a _begin checks first
static inline int begin_guard(jwas_hip_ctx* c, const char* words)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, residual_ptr(c) && c->method >= 0, JWAS_HIP_ESTATE, "no residual: load genotypes and call jwas_hip_init_state first");
    return refuse_shards(c, words);
}

// What every entry point of an open session checks first.  session: the context's member; begin: the entry point that opens it.
template <class S>
static int session_guard(jwas_hip_ctx* c, S jwas_hip_ctx::*session, const char* begin)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, (c->*session).active, JWAS_HIP_ESTATE, "%s has not been called", begin);
    return JWAS_HIP_OK;
}

// ... of a session with per-trait state: the traits are still those of its _begin; words: refuse_shards' (NULL: not refused here)
template <class S>
static int session_guard(jwas_hip_ctx* c, S jwas_hip_ctx::*session, const char* begin, const char* words)
{
    if (int rc = session_guard(c, session, begin)) return rc;
    NEED(c, residual_ptr(c) && c->method >= 0 && c->ntraits == (c->*session).nt, JWAS_HIP_ESTATE,
         "jwas_hip_init_state changed the number of traits after %s", begin);
    return words ? refuse_shards(c, words) : JWAS_HIP_OK;
}

// wait for the stream, then free the session: the body of every _end, and how a _begin drops an earlier session
static inline int session_drop(jwas_hip_ctx* c, void (*free_session)(jwas_hip_ctx*))
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_session(c);
    return JWAS_HIP_OK;
}

// owner.alloc, or the session freed and JWAS_HIP_ENOMEM with its name in the message
template <class T>
static int alloc_or_nomem(jwas_hip_ctx* c, DevOwner& owner, T** p, size_t bytes, const char* name, void (*free_session)(jwas_hip_ctx*))
{
    if (owner.alloc(p, bytes) == hipSuccess) return JWAS_HIP_OK;
    free_session(c);
    return fail(c, JWAS_HIP_ENOMEM, "%s: device allocation of %zu bytes failed", name, bytes);
}

static inline void split_seed(uint64_t seed, uint32_t& lo, uint32_t& hi) { lo = (uint32_t)(seed & 0xFFFFFFFFu); hi = (uint32_t)(seed >> 32); }

// dev -> host on the context's stream, then wait for it
static inline int to_host(jwas_hip_ctx* c, void* out, const void* dev, size_t bytes)
{
    HIPCHK(c, hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// a getter of `have` doubles: the caller's length is checked first
static inline int download(jwas_hip_ctx* c, const double* dev, int64_t have, int64_t nvalues, double* out)
{
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, nvalues == have, JWAS_HIP_EINVAL, "nvalues (%lld) differs from the session's (%lld)", (long long)nvalues, (long long)have);
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, out, dev, sizeof(double) * (size_t)have);
}

// The device time of a step (jwas_*_stats.step_ms): the context's two events around its launches.  _end records the second, brings
// the step's results to the host behind it, waits once and reads the time between the two.
static inline int step_timer_begin(jwas_hip_ctx* c) { HIPCHK(c, hipEventRecord(c->ev_start, c->stream)); return JWAS_HIP_OK; }

static inline int step_timer_end(jwas_hip_ctx* c, void* results, const void* dev, size_t bytes, double* step_ms)
{
    HIPCHK(c, hipEventRecord(c->ev_stop, c->stream));
    if (int rc = to_host(c, results, dev, bytes)) return rc;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
    *step_ms = (double)ms;
    return JWAS_HIP_OK;
}
