// session_annot.hip -- marker-annotation priors (annot.hpp), jwas_hip_annot_begin .. _end: MCMC/annotation_updates.jl:21-137,181-361.
#include "ctx.hpp"
#include "annot.hpp"

static_assert(jwa::kMaxCols == JWAS_HIP_ANNOT_MAX_COLS, "column limit mismatch");

static int need_annot(jwas_hip_ctx* c) { return session_guard(c, &jwas_hip_ctx::an, "jwas_hip_annot_begin"); }

void annot_free(jwas_hip_ctx* c) { DevOwner::reset(c->an); }      // (the table stays: it belongs to the context, see annot_table_slot)

static int64_t annot_table_size(int kind, int64_t p) { return kind == jwa::kBayesC ? p : 4 * p; }

static double** annot_table_slot(jwas_hip_ctx* c, int kind) { return kind == jwa::kBayesC ? &c->pi_vec : kind == jwa::kBayesR ? &c->pi_mat : &c->lpr_mat; }

// the indicators of trait `trait` as the sweep leaves them
static const void* annot_delta(jwas_hip_ctx* c, int trait)
{
    if (IS_F64(c)) return c->method == JWAS_HIP_BAYESR ? c->f64->delta : (const void*)((const double*)c->f64->delta + (size_t)trait * c->p);
    return (const void*)((const float*)c->delta + (size_t)trait * c->p);
}

template <class DT, int KIND>
static void annot_launch_step(jwas_hip_ctx* c, const jwa::StepArgs& A, bool first)
{
    const dim3 grid((unsigned)c->an.npieces), blk(256);
    if (first) hipLaunchKernelGGL((jwa::k_annot_liab<DT, KIND>), grid, blk, 0, c->stream, A);
    else       hipLaunchKernelGGL((jwa::k_annot_sums<DT, KIND>), grid, blk, 0, c->stream, A);
}

static void annot_launch_any(jwas_hip_ctx* c, const jwa::StepArgs& A, bool first)
{
    switch (c->an.kind) {
        case jwa::kBayesC: with_real(c, [&](auto real) { annot_launch_step<decltype(real), jwa::kBayesC>(c, A, first); }); break;
        case jwa::kBayesR: annot_launch_step<int32_t, jwa::kBayesR>(c, A, first); break;
        default:           with_real(c, [&](auto real) { annot_launch_step<decltype(real), jwa::kTree>(c, A, first); }); break;
    }
}

extern "C" {

int jwas_hip_annot_begin(jwas_hip_ctx* c, int32_t kind, int64_t p, int32_t ncols, const double* D_rowmajor, const double* coef,
                         const double* variance, const double* start_prior)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, residual_ptr(c) && c->method >= 0, JWAS_HIP_ESTATE, "no chain state: load genotypes and call jwas_hip_init_state first");
    NEED(c, !c->an.active, JWAS_HIP_ESTATE, "an annotation session is already open (jwas_hip_annot_end first)");
    if (int rc = refuse_shards(c, "annotation priors")) return rc;
    NEED(c, c->method != JWAS_HIP_MEGABAYESC && c->method != JWAS_HIP_MEGABAYESB, JWAS_HIP_EUNSUP, "annotation priors are not available with constraint = true (megaBayesABC)");
    NEED(c, kind >= jwa::kBayesC && kind <= jwa::kTree, JWAS_HIP_EINVAL, "unknown annotation kind %d", kind);
    const bool fits = kind == jwa::kBayesC ? (c->method == JWAS_HIP_BAYESC && c->ntraits == 1)
                    : kind == jwa::kBayesR ? (c->method == JWAS_HIP_BAYESR && c->ntraits == 1)
                                           : ((c->method == JWAS_HIP_MTBAYESC1 || c->method == JWAS_HIP_MTBAYESC2) && c->ntraits == 2);
    NEED(c, fits, JWAS_HIP_EINVAL, "annotation kind %d does not match the context's method %d with %d trait(s)", kind, c->method, c->ntraits);
    NEED(c, p == c->p, JWAS_HIP_EINVAL, "p (%lld) differs from the number of markers (%lld)", (long long)p, (long long)c->p);
    NEED(c, p >= 1 && p < ((int64_t)1 << 31) - jwa::kPiece, JWAS_HIP_EINVAL, "p must be 1 .. 2^31 - 1025 (got %lld)", (long long)p);
    NEED(c, ncols >= 1 && ncols <= jwa::kMaxCols, JWAS_HIP_EINVAL, "ncols must be 1 .. %d (got %d)", jwa::kMaxCols, ncols);
    NEED(c, D_rowmajor && coef && start_prior, JWAS_HIP_EINVAL, "NULL argument");
    const int ns = jwa::annot_nsteps(kind), K = ncols;
    const int64_t tab = annot_table_size(kind, p);
    for (int i = 0; i < ns * K; ++i) NEED(c, std::isfinite(coef[i]), JWAS_HIP_EINVAL, "coefficient %d is not finite (%g)", i, coef[i]);
    if (variance)
        for (int s = 0; s < ns; ++s) NEED(c, std::isfinite(variance[s]) && variance[s] > 0.0, JWAS_HIP_EINVAL, "variance[%d] must be positive and finite (%g)", s, variance[s]);
    for (int64_t i = 0; i < tab; ++i)
        NEED(c, !std::isnan(start_prior[i]) && start_prior[i] != INFINITY, JWAS_HIP_EINVAL, "start_prior[%lld] is not a probability or its log (%g)", (long long)i, start_prior[i]);
    std::vector<double> Dt((size_t)std::max(K - 1, 1) * (size_t)p);
    for (int64_t i = 0; i < p; ++i) {
        NEED(c, D_rowmajor[(size_t)i * K] == 1.0, JWAS_HIP_EINVAL, "marker %lld: column 0 of the design matrix must be the intercept's ones (%g)", (long long)i, D_rowmajor[(size_t)i * K]);
        for (int k = 1; k < K; ++k) {
            const double v = D_rowmajor[(size_t)i * K + k];
            NEED(c, std::isfinite(v), JWAS_HIP_EINVAL, "marker %lld, column %d: the annotation is not finite (%g)", (long long)i, k, v);
            Dt[(size_t)(k - 1) * p + i] = v;
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    auto& b = c->an;
    b.kind = kind; b.nsteps = ns; b.K = K;
    b.npieces = (int)((p + jwa::kPiece - 1) / jwa::kPiece);
    const size_t pb = sizeof(double) * (size_t)p;
    const size_t nscal = (size_t)jwa::kMaxSteps * K + 3 + 4 + 1 + K;
    const size_t colb = pb * (size_t)std::max(K - 1, 1), tabb = sizeof(double) * (size_t)tab;
    const struct { double** ptr; size_t bytes; } bufs[] = {
        {&b.D, colb}, {&b.liab, pb * ns}, {&b.mu, pb * ns}, {&b.e, pb},
        {&b.part, sizeof(double) * 3 * (size_t)b.npieces * (size_t)std::max(K - 1, 1)},      // (set-up: the piece sums of every column's squares)
        {&b.part4, sizeof(double) * 4 * (size_t)b.npieces}, {&b.scal, sizeof(double) * nscal}, {&b.mean, tabb}, {&b.mean2, tabb}};
    for (const auto& w : bufs)
        if (int rc = alloc_or_nomem(c, b.mem, w.ptr, w.bytes, "annotation session", annot_free)) return rc;
    double** slot = annot_table_slot(c, kind);              // (the context's, not the session's: it outlives jwas_hip_annot_end)
    if (!*slot && hipMalloc((void**)slot, tabb) != hipSuccess) {
        annot_free(c);
        return fail(c, JWAS_HIP_ENOMEM, "annotation session: device allocation of %zu bytes failed", tabb);
    }
    HIPCHK(c, hipMemcpyAsync(b.D, Dt.data(), colb, hipMemcpyHostToDevice, c->stream));
    for (const auto& w : bufs)
        if (w.ptr != &b.D) HIPCHK(c, hipMemsetAsync(*w.ptr, 0, w.bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.scal, coef, sizeof(double) * (size_t)ns * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(*slot, start_prior, tabb, hipMemcpyHostToDevice, c->stream));
    if (K > 1) {                        // d_k over all markers, for the steps whose active set is all markers
        double* dsq = b.scal + (size_t)jwa::kMaxSteps * K + 8;
        hipLaunchKernelGGL(jwa::k_annot_colsq, dim3((unsigned)b.npieces, (unsigned)(K - 1)), dim3(256), 0, c->stream, b.D, p, (int32_t)b.npieces, b.part);
        hipLaunchKernelGGL(jwa::k_annot_colsq_reduce, dim3((unsigned)(K - 1)), dim3(256), 0, c->stream, b.part, (int32_t)b.npieces, dsq);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the caller's arrays and Dt may go away once this returns)
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_annot_step(jwas_hip_ctx* c, const jwas_annot_params* P, jwas_annot_stats* S)
{
    if (int rc = need_annot(c)) return rc;
    NEED(c, P && S, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_annot_step: iteration must be >= 1");
    if (int rc = refuse_shards(c, "annotation priors")) return rc;
    auto& b = c->an;
    const int K = b.K, ns = b.nsteps;
    if (K > 1)
        for (int s = 0; s < ns; ++s)
            NEED(c, std::isfinite(P->variance[s]) && P->variance[s] > 0.0, JWAS_HIP_EINVAL, "variance[%d] must be positive and finite (%g)", s, P->variance[s]);
    HIPCHK(c, hipSetDevice(c->device));
    double* coef = b.scal;
    double* nA = b.scal + (size_t)jwa::kMaxSteps * K;
    double* means = nA + 3;
    double* dc = means + 4;
    double* dsq = dc + 1;
    if (int rc = step_timer_begin(c)) return rc;
    for (int s = 0; s < ns; ++s) {
        jwa::StepArgs A = {};
        A.d1 = annot_delta(c, 0); A.d2 = b.kind == jwa::kTree ? annot_delta(c, 1) : nullptr;
        A.D = b.D; A.coef = coef + (size_t)s * K; A.liab = b.liab + (size_t)s * c->p; A.e = b.e; A.part = b.part; A.dc = dc;
        A.p = c->p; A.K = K; A.s = s; A.all_active = s == 0;
        A.iter = P->iteration; split_seed(P->seed, A.seed_lo, A.seed_hi);
        jwa::DrawArgs W = {};
        W.part = b.part; W.dsq = dsq; W.coef = coef + (size_t)s * K; W.nA = nA + s; W.dc = dc; W.var = K > 1 ? P->variance[s] : 1.0;
        W.npieces = b.npieces; W.s = s; W.all_active = A.all_active; W.iter = A.iter; W.seed_lo = A.seed_lo; W.seed_hi = A.seed_hi;
        for (int k = 0; k < K; ++k) {
            A.k = k; W.k = k;
            annot_launch_any(c, A, k == 0);
            hipLaunchKernelGGL(jwa::k_annot_draw, dim3(1), dim3(256), 0, c->stream, W);
        }
    }
    jwa::TableArgs T = {};
    T.D = b.D; T.coef = coef; T.mu = b.mu; T.table = *annot_table_slot(c, b.kind); T.part = b.part4; T.p = c->p; T.K = K;
    const dim3 grid((unsigned)b.npieces), blk(256);
    if (b.kind == jwa::kBayesC)      hipLaunchKernelGGL((jwa::k_annot_table<jwa::kBayesC>), grid, blk, 0, c->stream, T);
    else if (b.kind == jwa::kBayesR) hipLaunchKernelGGL((jwa::k_annot_table<jwa::kBayesR>), grid, blk, 0, c->stream, T);
    else                             hipLaunchKernelGGL((jwa::k_annot_table<jwa::kTree>), grid, blk, 0, c->stream, T);
    hipLaunchKernelGGL(jwa::k_annot_colmeans, dim3(1), dim3(256), 0, c->stream, b.part4, (int32_t)b.npieces, b.kind == jwa::kBayesC ? 1 : 4, (double)c->p, means);
    HIPCHK(c, hipGetLastError());
    std::vector<double> host((size_t)jwa::kMaxSteps * K + 7);
    std::memset(S, 0, sizeof *S);
    if (int rc = step_timer_end(c, host.data(), b.scal, sizeof(double) * host.size(), &S->step_ms)) return rc;
    for (int i = 0; i < ns * K; ++i) S->coef[i] = host[(size_t)i];
    for (int s = 0; s < ns; ++s) S->n_active[s] = (int64_t)host[(size_t)jwa::kMaxSteps * K + s];
    for (int q = 0; q < 4; ++q) S->means[q] = host[(size_t)jwa::kMaxSteps * K + 3 + q];
    return JWAS_HIP_OK;
}

int jwas_hip_annot_accumulate(jwas_hip_ctx* c, double nsamples)
{
    if (int rc = need_annot(c)) return rc;
    NEED(c, nsamples >= 1.0, JWAS_HIP_EINVAL, "nsamples must be >= 1 (got %g)", nsamples);
    auto& b = c->an;
    const int64_t q = annot_table_size(b.kind, c->p);
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(jwa::k_annot_accumulate, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, c->stream, (const double*)*annot_table_slot(c, b.kind),
                       b.mean, b.mean2, q, nsamples, (int32_t)(b.kind == jwa::kTree));
    HIPCHK(c, hipGetLastError());
    return JWAS_HIP_OK;
}

int jwas_hip_annot_get_prior(jwas_hip_ctx* c, int64_t nvalues, double* out)
{
    if (int rc = need_annot(c)) return rc;
    return download(c, *annot_table_slot(c, c->an.kind), annot_table_size(c->an.kind, c->p), nvalues, out);
}

int jwas_hip_annot_get_means(jwas_hip_ctx* c, int64_t nvalues, double* out_mean, double* out_mean2)
{
    if (int rc = need_annot(c)) return rc;
    if (int rc = download(c, c->an.mean, annot_table_size(c->an.kind, c->p), nvalues, out_mean)) return rc;
    return out_mean2 ? download(c, c->an.mean2, annot_table_size(c->an.kind, c->p), nvalues, out_mean2) : JWAS_HIP_OK;
}

int jwas_hip_annot_get_liability(jwas_hip_ctx* c, int64_t nvalues, double* out)
{
    if (int rc = need_annot(c)) return rc;
    return download(c, c->an.liab, (int64_t)c->an.nsteps * c->p, nvalues, out);
}

int jwas_hip_annot_get_mu(jwas_hip_ctx* c, int64_t nvalues, double* out)
{
    if (int rc = need_annot(c)) return rc;
    return download(c, c->an.mu, (int64_t)c->an.nsteps * c->p, nvalues, out);
}

int64_t jwas_hip_annot_estimate_bytes(int64_t p, int32_t ncols, int32_t kind)
{
    // D, the liabilities and mu of every step, e, the table and its two running means, the piece sums, the scalars
    const int64_t ns = jwa::annot_nsteps(kind), K = std::max<int64_t>(ncols, 1), tab = annot_table_size(kind, p);
    const int64_t npieces = (p + jwa::kPiece - 1) / jwa::kPiece;
    return 8 * (std::max<int64_t>(K - 1, 1) * p + 2 * ns * p + p + 3 * tab + 3 * npieces * std::max<int64_t>(K - 1, 1) + 4 * npieces + 4 * K + 8);
}

int jwas_hip_annot_end(jwas_hip_ctx* c) { return session_drop(c, annot_free); }

}  // extern "C"
