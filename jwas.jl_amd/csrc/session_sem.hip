// session_sem.hip -- structural equation models (sem.hpp), jwas_hip_sem_begin .. _end: structure_equation_model/SEM.jl:53-165,245-252.
#include "ctx.hpp"
#include "sem.hpp"

static int need_sem(jwas_hip_ctx* c) { return session_guard(c, &jwas_hip_ctx::sm, "jwas_hip_sem_begin", "structural equation models"); }

void sem_free(jwas_hip_ctx* c) { DevOwner::reset(c->sm); }

// the 4 x 4 device layout <-> the caller's t x t
static void sem_pack(const double* dev16, int t, double* out) { for (int i = 0; i < t; ++i) for (int j = 0; j < t; ++j) out[i * t + j] = dev16[i * jws::kMaxT + j]; }

// a 4 x 4 matrix of the session to the caller's t x t: S (gram), or the record's lambda
static int sem_get16(jwas_hip_ctx* c, bool gram, double* out)
{
    if (int rc = need_sem(c)) return rc;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    double host[16];
    if (int rc = to_host(c, host, gram ? c->sm.S : c->sm.rec + jws::kRecLambda, sizeof host)) return rc;
    sem_pack(host, c->sm.nt, out);
    return JWAS_HIP_OK;
}

extern "C" {

int jwas_hip_sem_begin(jwas_hip_ctx* c, int32_t ntraits, int64_t n, const double* y, const int32_t* cs)
{
    if (int rc = begin_guard(c, "structural equation models")) return rc;
    NEED(c, ntraits >= 2, JWAS_HIP_EINVAL, "Causal strutures are only allowed in multi-trait analysis (got %d trait)", ntraits);
    NEED(c, ntraits <= jws::kMaxT && ntraits == c->ntraits, JWAS_HIP_EINVAL, "ntraits (%d) differs from the context's (%d)", ntraits, c->ntraits);
    NEED(c, n == c->n, JWAS_HIP_EINVAL, "n (%lld) differs from the number of records (%lld)", (long long)n, (long long)c->n);
    NEED(c, y && cs, JWAS_HIP_EINVAL, "NULL argument");
    const int t = ntraits;
    uint32_t mask = 0, ymask = 0, rmask = 0;
    for (int i = 0; i < t; ++i)
        for (int j = 0; j < t; ++j) {
            const int v = cs[i * t + j];
            NEED(c, v == 0 || v == 1, JWAS_HIP_EINVAL, "causal structure [%d][%d] = %d is not 0 or 1", i, j, v);
            NEED(c, v == 0 || i > j, JWAS_HIP_EINVAL, "The causal structue needs to be a lower triangular matrix. ([%d][%d] is set)", i, j);
            if (v) { mask |= 1u << jws::cell(i, j); ymask |= 1u << j; rmask |= 1u << i; }
        }
    for (int64_t i = 0; i < (int64_t)t * n; ++i)
        NEED(c, std::isfinite(y[i]), JWAS_HIP_EINVAL, "phenotype %lld of trait %lld is not finite (%g)", (long long)(i % n), (long long)(i / n), y[i]);
    if (int rc = session_drop(c, sem_free)) return rc;
    auto& b = c->sm;
    b.nt = t; b.G = jws::sem_grid(n); b.mask = mask; b.ymask = ymask; b.rmask = rmask;
    const size_t accb = sizeof(double) * 6 * (size_t)t * (size_t)c->p;
    auto alloc = [&](double** ptr, size_t bytes) { return alloc_or_nomem(c, b.mem, ptr, bytes, "SEM session", sem_free); };
    if (int rc = alloc(&b.y, sizeof(double) * (size_t)t * (size_t)n)) return rc;
    if (int rc = alloc(&b.part, sizeof(double) * (size_t)b.G * jws::kGramCells)) return rc;
    if (int rc = alloc(&b.S, sizeof(double) * 16)) return rc;
    if (int rc = alloc(&b.rec, sizeof(double) * jws::kRecSize)) return rc;
    if (int rc = alloc(&b.acc, accb)) return rc;
    HIPCHK(c, hipMemcpyAsync(b.y, y, sizeof(double) * (size_t)t * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.rec, 0, sizeof(double) * jws::kRecSize, c->stream));
    HIPCHK(c, hipMemsetAsync(b.acc, 0, accb, c->stream));
    hipLaunchKernelGGL(jws::k_sem_gram, dim3((unsigned)b.G), dim3(256), 0, c->stream, (const double*)b.y, n, (int32_t)t, b.part);
    hipLaunchKernelGGL(jws::k_sem_gram_sum, dim3(1), dim3(64), 0, c->stream, (const double*)b.part, (int32_t)b.G, b.S);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the caller's arrays may go away once this returns)
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_sem_step(jwas_hip_ctx* c, const jwas_sem_params* P, jwas_sem_stats* S)
{
    if (int rc = need_sem(c)) return rc;
    NEED(c, P && S, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_sem_step: iteration must be >= 1");
    auto& b = c->sm;
    const int t = b.nt;
    for (int i = 0; i < t; ++i)
        NEED(c, std::isfinite(P->R_diag[i]) && P->R_diag[i] > 0.0, JWAS_HIP_EINVAL, "R_diag[%d] must be positive and finite (%g)", i, P->R_diag[i]);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = step_timer_begin(c)) return rc;
    jws::DotArgs D = {};
    D.r = residual_ptr(c); D.y = b.y; D.part = b.part; D.n = c->n; D.ld = c->ld; D.mask = b.mask; D.ymask = b.ymask; D.rmask = b.rmask; D.nt = t;
    jws::DrawArgs W = {};
    W.part = b.part; W.S = b.S; W.rec = b.rec; W.G = b.G; W.nt = t; W.mask = b.mask;
    for (int i = 0; i < t; ++i) W.Rdiag[i] = P->R_diag[i];
    W.iter = P->iteration; split_seed(P->seed, W.seed_lo, W.seed_hi);
    jws::ApplyArgs A = {};
    A.r = residual_ptr(c); A.y = b.y; A.d = b.rec + jws::kRecD; A.n = c->n; A.ld = c->ld; A.mask = b.mask; A.ymask = b.ymask; A.rmask = b.rmask; A.nt = t;
    if (b.mask) {                                               // (a structure without an edge: nothing to sample)
        const dim3 grid((unsigned)b.G), rows((unsigned)((c->n + 255) / 256));
        with_real(c, [&](auto real) { hipLaunchKernelGGL((jws::k_sem_dots<decltype(real)>), grid, dim3(256), 0, c->stream, D); });
        hipLaunchKernelGGL(jws::k_sem_draw, dim3(1), dim3(64), 0, c->stream, W);
        with_real(c, [&](auto real) { hipLaunchKernelGGL((jws::k_sem_apply<decltype(real)>), rows, dim3(256), 0, c->stream, A); });
        HIPCHK(c, hipGetLastError());
    }
    double host[jws::kRecSize];
    std::memset(S, 0, sizeof *S);
    if (int rc = step_timer_end(c, host, b.rec, sizeof host, &S->step_ms)) return rc;
    sem_pack(host + jws::kRecLambda, t, S->lambda);
    sem_pack(host + jws::kRecMu, t, S->mean);
    sem_pack(host + jws::kRecC, t, S->ypr);
    return JWAS_HIP_OK;
}

int jwas_hip_sem_get_lambda(jwas_hip_ctx* c, double* out) { return sem_get16(c, false, out); }

int jwas_hip_sem_set_lambda(jwas_hip_ctx* c, const double* in)
{
    if (int rc = need_sem(c)) return rc;
    NEED(c, in, JWAS_HIP_EINVAL, "NULL argument");
    const int t = c->sm.nt;
    double host[16] = {0.0};
    for (int i = 0; i < t; ++i)
        for (int j = 0; j < t; ++j) {
            const double v = in[i * t + j];
            NEED(c, std::isfinite(v), JWAS_HIP_EINVAL, "lambda[%d][%d] is not finite (%g)", i, j, v);
            const bool edge = i > j && ((c->sm.mask >> jws::cell(i, j)) & 1u);
            NEED(c, edge || v == 0.0, JWAS_HIP_EINVAL, "lambda[%d][%d] = %g lies outside the causal structure", i, j, v);
            host[i * jws::kMaxT + j] = v;
        }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->sm.rec + jws::kRecLambda, host, sizeof host, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_sem_get_gram(jwas_hip_ctx* c, double* out) { return sem_get16(c, true, out); }

int jwas_hip_sem_accumulate(jwas_hip_ctx* c, const double* K, double nsamples)
{
    if (int rc = need_sem(c)) return rc;
    NEED(c, K, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, nsamples >= 1.0, JWAS_HIP_EINVAL, "nsamples must be >= 1 (got %g)", nsamples);
    const int t = c->sm.nt;
    jws::AccArgs A = {};
    for (int i = 0; i < t; ++i)
        for (int j = 0; j < t; ++j) {
            NEED(c, std::isfinite(K[i * t + j]), JWAS_HIP_EINVAL, "K[%d][%d] is not finite (%g)", i, j, K[i * t + j]);
            A.K[i * jws::kMaxT + j] = K[i * t + j];
        }
    A.alpha = alpha_ptr(c);
    A.acc = c->sm.acc; A.nsamples = nsamples; A.p = c->p; A.nt = t;
    HIPCHK(c, hipSetDevice(c->device));
    const dim3 grid((unsigned)((c->p + 255) / 256));
    with_real(c, [&](auto real) { hipLaunchKernelGGL((jws::k_sem_accumulate<decltype(real)>), grid, dim3(256), 0, c->stream, A); });
    HIPCHK(c, hipGetLastError());
    return JWAS_HIP_OK;
}

int jwas_hip_sem_get_effects(jwas_hip_ctx* c, int32_t kind, int32_t trait, double* mean, double* mean2, double* freq)
{
    if (int rc = need_sem(c)) return rc;
    NEED(c, kind == 0 || kind == 1, JWAS_HIP_EINVAL, "kind must be 0 (indirect) or 1 (overall), got %d", kind);
    NEED(c, trait >= 0 && trait < c->sm.nt, JWAS_HIP_EINVAL, "trait %d outside [0,%d)", trait, c->sm.nt);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t stat = (size_t)c->sm.nt * c->p, nb = sizeof(double) * (size_t)c->p;
    const double* base = c->sm.acc + (size_t)kind * 3 * stat + (size_t)trait * c->p;
    if (mean) HIPCHK(c, hipMemcpyAsync(mean, base, nb, hipMemcpyDeviceToHost, c->stream));
    if (mean2) HIPCHK(c, hipMemcpyAsync(mean2, base + stat, nb, hipMemcpyDeviceToHost, c->stream));
    if (freq) HIPCHK(c, hipMemcpyAsync(freq, base + 2 * stat, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int64_t jwas_hip_sem_estimate_bytes(int64_t n, int64_t p, int32_t ntraits)
{
    // the phenotypes, the six accumulators per marker and trait, the workgroup partials, S and the record
    const int64_t t = std::max<int64_t>(ntraits, 1);
    return 8 * (t * n + 6 * t * p + (int64_t)jws::kMaxGrid * jws::kGramCells + 16 + jws::kRecSize);
}

int jwas_hip_sem_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::sm, "jwas_hip_sem_begin")) return rc;
    return session_drop(c, sem_free);
}

}  // extern "C"
