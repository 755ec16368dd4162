// session_mtmiss.hip -- multi-trait records that miss some traits (mtmiss.hpp), jwas_hip_mtmiss_begin .. _end: residual.jl:2-73.
#include "ctx.hpp"
#include "mtmiss.hpp"

static int need_mtmiss(jwas_hip_ctx* c) { return session_guard(c, &jwas_hip_ctx::mt, "jwas_hip_mtmiss_begin", "missing-trait records"); }

void mtmiss_free(jwas_hip_ctx* c) { DevOwner::reset(c->mt); }

// every entry of a [2^t][t][t] table is finite
static bool mtmiss_table_finite(const double* tab, int t)
{
    for (int i = 0; i < (1 << t) * t * t; ++i) if (!std::isfinite(tab[i])) return false;
    return true;
}

extern "C" {

int jwas_hip_mtmiss_begin(jwas_hip_ctx* c, int64_t n, const int32_t* observed)
{
    if (int rc = begin_guard(c, "missing-trait records")) return rc;
    NEED(c, observed, JWAS_HIP_EINVAL, "observed is NULL");
    NEED(c, n == c->n, JWAS_HIP_EINVAL, "n (%lld) differs from the number of records (%lld)", (long long)n, (long long)c->n);
    const int t = c->ntraits;
    NEED(c, t >= 1 && t <= jwm::kMaxT, JWAS_HIP_EINVAL, "the number of traits (%d) is outside 1..%d", t, jwm::kMaxT);
    for (int64_t i = 0; i < n; ++i)
        NEED(c, observed[i] >= 1 && observed[i] < (1 << t), JWAS_HIP_EINVAL, "record %lld: code %d outside 1..%d", (long long)i, observed[i], (1 << t) - 1);
    if (int rc = session_drop(c, mtmiss_free)) return rc;
    auto& b = c->mt;
    HIPCHK(c, b.mem.alloc(&b.code, sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1)));
    HIPCHK(c, b.mem.alloc(&b.tab, sizeof(double) * 3 * jwm::kMaxCodes * 16));
    HIPCHK(c, hipMemcpy(b.code, observed, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(b.tab, 0, sizeof(double) * 3 * jwm::kMaxCodes * 16, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.nt = t;
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_mtmiss_impute(jwas_hip_ctx* c, const jwas_mtmiss_params* P)
{
    if (int rc = need_mtmiss(c)) return rc;
    NEED(c, P && P->B && P->U, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_mtmiss_impute: iteration must be >= 1");
    auto& b = c->mt;
    const int t = b.nt;
    NEED(c, mtmiss_table_finite(P->B, t) && mtmiss_table_finite(P->U, t), JWAS_HIP_EINVAL, "jwas_hip_mtmiss_impute: a table entry is not finite");
    if (t == 1) return JWAS_HIP_OK;                             // (one trait: every record is complete)
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(double) * (size_t)(1 << t) * t * t;
    HIPCHK(c, hipMemcpyAsync(b.tab, P->B, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.tab + jwm::kMaxCodes * 16, P->U, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // (the caller's tables may go away once this returns)
    jwm::ImputeArgs A = {};
    A.r = residual_ptr(c); A.ld = c->ld; A.n = c->n; A.code = b.code; A.B = b.tab; A.U = b.tab + jwm::kMaxCodes * 16; A.nt = t;
    A.iter = P->iteration; split_seed(P->seed, A.seed_lo, A.seed_hi);
    const dim3 grid((unsigned)((c->n + 255) / 256));
    with_real(c, [&](auto real) { hipLaunchKernelGGL((jwm::k_mtmiss_impute<decltype(real)>), grid, dim3(256), 0, c->stream, A); });
    HIPCHK(c, hipGetLastError());
    return JWAS_HIP_OK;
}

int jwas_hip_mtmiss_set_record_weights(jwas_hip_ctx* c, const double* C)
{
    if (int rc = need_mtmiss(c)) return rc;
    auto& b = c->mt;
    if (!C) { b.weights = false; return JWAS_HIP_OK; }
    const int t = b.nt;
    NEED(c, t > 1, JWAS_HIP_ESTATE, "per-record weights need more than one trait");
    NEED(c, mtmiss_table_finite(C, t), JWAS_HIP_EINVAL, "jwas_hip_mtmiss_set_record_weights: a table entry is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b.tab + 2 * jwm::kMaxCodes * 16, C, sizeof(double) * (size_t)(1 << t) * t * t, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.weights = true;
    return JWAS_HIP_OK;
}

int64_t jwas_hip_mtmiss_estimate_bytes(int64_t n)
{
    // the codes (int32), the piece sums of D of the largest term (at most one piece per record), the three tables
    return 4 * n + 8 * n + (int64_t)sizeof(double) * 3 * jwm::kMaxCodes * 16;
}

int jwas_hip_mtmiss_end(jwas_hip_ctx* c) { return session_drop(c, mtmiss_free); }

}  // extern "C"
