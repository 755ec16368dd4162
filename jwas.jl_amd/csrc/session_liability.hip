// session_liability.hip -- threshold / censored traits: the liabilities (liability.hpp), jwas_hip_liability_begin .. _end.
#include "ctx.hpp"
#include "liability.hpp"

static int need_liab(jwas_hip_ctx* c) { return session_guard(c, &jwas_hip_ctx::lb, "jwas_hip_liability_begin", nullptr); }
#define NEED_LIAB_TRAIT(c, trait) NEED(c, trait >= 0 && trait < c->lb.nt, JWAS_HIP_EINVAL, "trait %d outside [0,%d)", trait, c->lb.nt)

void liab_free(jwas_hip_ctx* c) { DevOwner::reset(c->lb); }

static int liab_check_thresholds(jwas_hip_ctx* c, int32_t nthr, const double* thr)
{
    NEED(c, thr, JWAS_HIP_EINVAL, "thresholds is NULL");
    NEED(c, nthr >= 3 && nthr <= jwl::kMaxThr, JWAS_HIP_EINVAL, "nthresholds must be 3..%d, -Inf and +Inf included (got %d)", jwl::kMaxThr, nthr);
    NEED(c, thr[0] == -INFINITY && thr[nthr - 1] == INFINITY, JWAS_HIP_EINVAL, "thresholds must start with -Inf and end with +Inf");
    for (int i = 1; i < nthr; ++i)
        NEED(c, thr[i] > thr[i - 1], JWAS_HIP_EINVAL, "thresholds must be strictly increasing (entry %d: %g after %g)", i, thr[i], thr[i - 1]);
    return JWAS_HIP_OK;
}

// (re)allocate the liability vector of a trait and drop what an earlier declaration of it left
static int liab_reset_trait(jwas_hip_ctx* c, int trait)
{
    auto& b = c->lb;
    b.mem.free_one(b.codes[trait]); b.mem.free_one(b.lower[trait]); b.mem.free_one(b.upper[trait]); b.mem.free_one(b.part[trait]);
    b.part_valid[trait] = false;
    b.kind[trait] = jwl::kContinuous; b.ncat[trait] = 0;
    if (!b.y[trait]) HIPCHK(c, b.mem.alloc(&b.y[trait], (IS_F64(c) ? 8 : 4) * (size_t)c->ld));
    return JWAS_HIP_OK;
}

static int liab_upload_placeholder(jwas_hip_ctx* c, int trait, const std::vector<double>& y0)
{
    std::vector<float> y32;                                 // (a Float64 context uploads y0 itself)
    if (!IS_F64(c)) y32.assign(y0.begin(), y0.end());
    const void* src = IS_F64(c) ? (const void*)y0.data() : (const void*)y32.data();
    HIPCHK(c, hipMemcpyAsync(c->lb.y[trait], src, (IS_F64(c) ? 8 : 4) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

template <class T>
static void liab_launch(jwas_hip_ctx* c, const jwl::LiabArgs& A)
{
    const dim3 grid((unsigned)c->lb.nparts), block(256);
    switch (c->lb.nt) {
        case 1: hipLaunchKernelGGL((jwl::k_liability_sample<1, T>), grid, block, 0, c->stream, A); break;
        case 2: hipLaunchKernelGGL((jwl::k_liability_sample<2, T>), grid, block, 0, c->stream, A); break;
        case 3: hipLaunchKernelGGL((jwl::k_liability_sample<3, T>), grid, block, 0, c->stream, A); break;
        default: hipLaunchKernelGGL((jwl::k_liability_sample<4, T>), grid, block, 0, c->stream, A); break;
    }
}

static int liab_draw(jwas_hip_ctx* c, const jwas_liability_params* P, bool init, const char* who)
{
    if (int rc = need_liab(c)) return rc;
    NEED(c, P, JWAS_HIP_EINVAL, "params is NULL");
    auto& b = c->lb;
    const int t = b.nt;
    NEED(c, init || b.inited, JWAS_HIP_ESTATE, "jwas_hip_liability_init has not been called");
    NEED(c, init || P->iteration >= 1, JWAS_HIP_EINVAL, "%s: iteration must be >= 1 (0 is the set-up draw)", who);
    NEED(c, init || (P->ngibbs >= 1 && P->ngibbs <= 1000), JWAS_HIP_EINVAL, "%s: ngibbs must be 1..1000 (got %d)", who, P->ngibbs);
    int nliab = 0;
    for (int k = 0; k < t; ++k) nliab += b.kind[k] != jwl::kContinuous;
    NEED(c, nliab > 0, JWAS_HIP_ESTATE, "%s: no trait was declared categorical or censored", who);
    jwl::LiabArgs A = {};
    for (int k = 0; k < t; ++k) {
        for (int j = 0; j < t; ++j)
            NEED(c, std::isfinite(P->R[k * t + j]) && P->R[k * t + j] == P->R[j * t + k], JWAS_HIP_EINVAL, "%s: R must be finite and symmetric", who);
        double var = P->R[k * t + k];
        if (!init && t > 1) {                     // B = R_12 R_22^-1, s^2 = R_11 - R_12 R_22^-1 R_21 (:196-197), "2" = the other traits in order
            double R22[9], R22i[9], R12[3];
            int o[3], m = 0;
            for (int j = 0; j < t; ++j) if (j != k) o[m++] = j;
            for (int a = 0; a < m; ++a) { R12[a] = P->R[k * t + o[a]]; for (int e = 0; e < m; ++e) R22[a * m + e] = P->R[o[a] * t + o[e]]; }
            NEED(c, inv_small(R22, m, R22i) == 0, JWAS_HIP_EINVAL, "%s: R is singular", who);
            for (int a = 0; a < m; ++a) {
                double acc = 0.0;
                for (int e = 0; e < m; ++e) acc += R12[e] * R22i[e * m + a];
                A.B[k][o[a]] = acc;
            }
            for (int a = 0; a < m; ++a) var -= A.B[k][o[a]] * R12[a];
        }
        NEED(c, var > 0.0 && std::isfinite(var), JWAS_HIP_EINVAL, "%s: R is not positive definite (conditional variance of trait %d: %g)", who, k, var);
        A.sd[k] = std::sqrt(var);
    }
    A.n = c->n; A.ld = c->ld; A.r = residual_ptr(c); A.thr = b.thr;
    for (int k = 0; k < t; ++k) {
        A.kind[k] = b.kind[k]; A.ncat[k] = b.ncat[k];
        A.y[k] = b.kind[k] != jwl::kContinuous ? b.y[k] : nullptr;
        A.codes[k] = b.codes[k]; A.lower[k] = b.lower[k]; A.upper[k] = b.upper[k];
        A.part[k] = b.kind[k] == jwl::kCategorical ? b.part[k] : nullptr;
    }
    A.ngibbs = init ? 1 : P->ngibbs; A.init = init ? 1 : 0;
    A.iter = init ? 0u : P->iteration; split_seed(P->seed, A.seed_lo, A.seed_hi);
    HIPCHK(c, hipSetDevice(c->device));
    with_real(c, [&](auto real) { liab_launch<decltype(real)>(c, A); });
    HIPCHK(c, hipGetLastError());
    for (int k = 0; k < t; ++k) b.part_valid[k] = A.part[k] != nullptr;
    if (init) b.inited = true;
    return JWAS_HIP_OK;
}

extern "C" {

int jwas_hip_liability_begin(jwas_hip_ctx* c, int32_t ntraits)
{
    if (int rc = begin_guard(c, "liabilities")) return rc;
    NEED(c, ntraits == c->ntraits, JWAS_HIP_EINVAL, "ntraits (%d) differs from jwas_hip_init_state's (%d)", ntraits, c->ntraits);
    if (int rc = session_drop(c, liab_free)) return rc;
    auto& b = c->lb;
    b.nt = ntraits;
    b.nparts = (int)((c->n + 255) / 256);
    HIPCHK(c, b.mem.alloc(&b.thr, sizeof(double) * jwl::kMaxT * jwl::kMaxThr));
    HIPCHK(c, b.mem.alloc(&b.mm, sizeof(double) * jwl::kMM));
    HIPCHK(c, hipMemset(b.thr, 0, sizeof(double) * jwl::kMaxT * jwl::kMaxThr));
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_liability_set_categorical(jwas_hip_ctx* c, int32_t trait, int64_t n, const int32_t* codes, int32_t nthr, const double* thr)
{
    if (int rc = need_liab(c)) return rc;
    NEED_LIAB_TRAIT(c, trait);
    NEED(c, codes, JWAS_HIP_EINVAL, "codes is NULL");
    NEED(c, n == c->n, JWAS_HIP_EINVAL, "n (%lld) differs from the number of records (%lld)", (long long)n, (long long)c->n);
    if (int rc = liab_check_thresholds(c, nthr, thr)) return rc;
    const int ncat = nthr - 1;
    for (int64_t i = 0; i < n; ++i)
        NEED(c, codes[i] >= 0 && codes[i] <= ncat, JWAS_HIP_EINVAL, "record %lld: category %d outside 0..%d", (long long)i, codes[i], ncat);
    auto& b = c->lb;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = liab_reset_trait(c, trait)) return rc;
    HIPCHK(c, b.mem.alloc(&b.codes[trait], 4 * (size_t)n));
    HIPCHK(c, b.mem.alloc(&b.part[trait], sizeof(double) * (size_t)b.nparts * jwl::kMM));
    HIPCHK(c, hipMemcpy(b.codes[trait], codes, 4 * (size_t)n, hipMemcpyHostToDevice));
    std::memcpy(b.thr_host[trait], thr, sizeof(double) * nthr);
    HIPCHK(c, hipMemcpy(b.thr + trait * jwl::kMaxThr, thr, sizeof(double) * nthr, hipMemcpyHostToDevice));
    std::vector<double> y0((size_t)n);
    for (int64_t i = 0; i < n; ++i) y0[(size_t)i] = (double)codes[i];
    if (int rc = liab_upload_placeholder(c, trait, y0)) return rc;
    b.kind[trait] = jwl::kCategorical; b.ncat[trait] = ncat; b.inited = false;
    return JWAS_HIP_OK;
}

int jwas_hip_liability_set_censored(jwas_hip_ctx* c, int32_t trait, int64_t n, const double* lower, const double* upper)
{
    if (int rc = need_liab(c)) return rc;
    NEED_LIAB_TRAIT(c, trait);
    NEED(c, lower && upper, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, n == c->n, JWAS_HIP_EINVAL, "n (%lld) differs from the number of records (%lld)", (long long)n, (long long)c->n);
    for (int64_t i = 0; i < n; ++i)
        NEED(c, lower[i] <= upper[i] && lower[i] < INFINITY && upper[i] > -INFINITY, JWAS_HIP_EINVAL,
             "record %lld: bounds [%g, %g] (lower > upper, NaN, or an infinite exact value)", (long long)i, lower[i], upper[i]);
    auto& b = c->lb;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = liab_reset_trait(c, trait)) return rc;
    HIPCHK(c, b.mem.alloc(&b.lower[trait], 8 * (size_t)n));
    HIPCHK(c, b.mem.alloc(&b.upper[trait], 8 * (size_t)n));
    HIPCHK(c, hipMemcpy(b.lower[trait], lower, 8 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(b.upper[trait], upper, 8 * (size_t)n, hipMemcpyHostToDevice));
    std::vector<double> y0((size_t)n);
    for (int64_t i = 0; i < n; ++i) y0[(size_t)i] = lower[i] == -INFINITY ? (upper[i] == INFINITY ? 0.0 : upper[i]) : lower[i];
    if (int rc = liab_upload_placeholder(c, trait, y0)) return rc;
    b.kind[trait] = jwl::kCensored; b.inited = false;
    return JWAS_HIP_OK;
}

int jwas_hip_liability_set_thresholds(jwas_hip_ctx* c, int32_t trait, int32_t nthr, const double* thr)
{
    if (int rc = need_liab(c)) return rc;
    NEED_LIAB_TRAIT(c, trait);
    auto& b = c->lb;
    NEED(c, b.kind[trait] == jwl::kCategorical, JWAS_HIP_ESTATE, "trait %d is not categorical", trait);
    NEED(c, nthr == b.ncat[trait] + 1, JWAS_HIP_EINVAL, "trait %d has %d thresholds (got %d)", trait, b.ncat[trait] + 1, nthr);
    if (int rc = liab_check_thresholds(c, nthr, thr)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    std::memcpy(b.thr_host[trait], thr, sizeof(double) * nthr);
    // (from the context's own copy: the caller's array need not outlive the call)
    HIPCHK(c, hipMemcpyAsync(b.thr + trait * jwl::kMaxThr, b.thr_host[trait], sizeof(double) * nthr, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_liability_init(jwas_hip_ctx* c, const jwas_liability_params* P) { return liab_draw(c, P, true, "jwas_hip_liability_init"); }

int jwas_hip_liability_sample(jwas_hip_ctx* c, const jwas_liability_params* P) { return liab_draw(c, P, false, "jwas_hip_liability_sample"); }

int jwas_hip_liability_minmax(jwas_hip_ctx* c, int32_t trait, double* max_below, double* min_above)
{
    if (int rc = need_liab(c)) return rc;
    NEED_LIAB_TRAIT(c, trait);
    NEED(c, max_below && min_above, JWAS_HIP_EINVAL, "NULL argument");
    auto& b = c->lb;
    NEED(c, b.kind[trait] == jwl::kCategorical, JWAS_HIP_ESTATE, "trait %d is not categorical", trait);
    const int ncat = b.ncat[trait];
    HIPCHK(c, hipSetDevice(c->device));
    if (!b.part_valid[trait]) {
        with_real(c, [&](auto real) {
            hipLaunchKernelGGL((jwl::k_liability_minmax<decltype(real)>), dim3((unsigned)b.nparts), dim3(256), 0, c->stream, (const decltype(real)*)b.y[trait], b.codes[trait], c->n, ncat, b.part[trait]); });
        b.part_valid[trait] = true;
    }
    hipLaunchKernelGGL(jwl::k_liability_minmax_reduce, dim3(1), dim3(256), 0, c->stream, b.part[trait], b.nparts, ncat, b.mm);
    HIPCHK(c, hipGetLastError());
    double mm[jwl::kMM];
    if (int rc = to_host(c, mm, b.mm, sizeof(double) * 2 * ncat)) return rc;
    max_below[0] = min_above[0] = -INFINITY;
    max_below[ncat] = min_above[ncat] = INFINITY;
    for (int i = 1; i < ncat; ++i) {                // threshold i separates categories i and i + 1
        max_below[i] = mm[2 * (i - 1)];
        min_above[i] = mm[2 * i + 1];
    }
    return JWAS_HIP_OK;
}

int jwas_hip_get_liabilities(jwas_hip_ctx* c, int32_t trait, double* out)
{
    if (int rc = need_liab(c)) return rc;
    NEED_LIAB_TRAIT(c, trait);
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    auto& b = c->lb;
    NEED(c, b.kind[trait] != jwl::kContinuous, JWAS_HIP_ESTATE, "trait %d is continuous: it has no liabilities", trait);
    HIPCHK(c, hipSetDevice(c->device));
    if (IS_F64(c)) return to_host(c, out, b.y[trait], 8 * (size_t)c->n);
    std::vector<float> y32((size_t)c->n);
    if (int rc = to_host(c, y32.data(), b.y[trait], 4 * (size_t)c->n)) return rc;
    for (int64_t i = 0; i < c->n; ++i) out[i] = (double)y32[(size_t)i];
    return JWAS_HIP_OK;
}

int jwas_hip_liability_end(jwas_hip_ctx* c) { return session_drop(c, liab_free); }

}  // extern "C"
