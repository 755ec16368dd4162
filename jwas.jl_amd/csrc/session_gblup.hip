// session_gblup.hip -- GBLUP (gblup.hpp): jwas_hip_grm, the genomic relationship matrix of the context's dense matrix
// (readgenotypes.jl:403-408), jwas_hip_grm_packed2bit, the same matrix of the context's 2-bit packed genotypes, and jwas_hip_gblup_begin .. _end, GBLUP! / megaGBLUP! / MTGBLUP! on the eigenvectors of that matrix
// (markers/BayesianAlphabet/GBLUP.jl) with the context's own residual and effects.
#include "ctx.hpp"
#include "gblup.hpp"

static_assert(jwb::kMaxT == JWAS_HIP_MAX_TRAITS && jwb::kGrmChunk == JWAS_HIP_GRM_CHUNK, "the header's limits are gblup.hpp's");

void gblup_free(jwas_hip_ctx* c) { DevOwner::reset(c->gb); }

// what jwas_hip_grm and jwas_hip_gblup_begin ask of the storage
static int need_dense(jwas_hip_ctx* c, const char* words)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, !c->packed, JWAS_HIP_EUNSUP, "%s need dense genotypes (2-bit packed storage is not supported)", words);
    NEED(c, genotypes_ptr(c) && c->n > 0 && c->p > 0, JWAS_HIP_ESTATE, "no genotype matrix loaded");
    return refuse_shards(c, words);
}

static int need_gblup(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::gb, "jwas_hip_gblup_begin", "GBLUP steps")) return rc;
    NEED(c, c->gb.mat == genotypes_ptr(c), JWAS_HIP_ESTATE, "the genotypes were reloaded after jwas_hip_gblup_begin");
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "GBLUP does not run with residual weights");
    return JWAS_HIP_OK;
}

// the column parts of a pass over L: enough workgroups for the device whatever n, at least 64 columns each
static void gblup_parts(int64_t n, int nslices, int& nparts, int& len)
{
    const int want = std::min(jwb::kMaxParts, std::max(1, (512 + nslices - 1) / nslices));
    len = (int)round_up(std::max<int64_t>(64, (n + want - 1) / want), 4);
    nparts = (int)((n + len - 1) / len);
}

static int64_t gblup_bytes(int64_t n, int T, int bits)
{
    const int64_t ld = round_up(n, jwb::kRows), nsl = ld / jwb::kRows, el = bits == 64 ? 8 : 4;
    int nparts, len;
    gblup_parts(n, (int)nsl, nparts, len);
    return 8 * (n + n * T + (int64_t)nparts * T * ld + jwb::kParSize + ((n + 255) / 256) * T * T + nsl * (T * T + T)) + el * T * ld;
}

template <int T>
static bool spd_small(const double* A)
{
    double L[T][T] = {};
    for (int a = 0; a < T; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = A[a * T + b];
            for (int k = 0; k < b; ++k) s -= L[a][k] * L[b][k];
            if (a == b) { if (!(s > 0.0) || !std::isfinite(s)) return false; L[a][a] = std::sqrt(s); }
            else L[a][b] = s / L[b][b];
        }
    return true;
}

template <class real, int T>
static void gblup_launch(jwas_hip_ctx* c, const jwb::SampleArgs& A)
{
    auto& b = c->gb;
    const real* L = (const real*)genotypes_ptr(c);
    real* r = (real*)residual_ptr(c);
    real* rplus = (real*)b.rplus;
    const real* alpha = (const real*)alpha_ptr(c);
    const int64_t n = c->n, ld = c->ld;
    const dim3 grid((unsigned)c->nslices, (unsigned)b.nparts);
    double* fin = b.stat + (size_t)b.nwg * T * T;
    hipLaunchKernelGGL((jwb::k_gblup_mul<real, T>), grid, dim3(256), 0, c->stream, L, ld, n, (int32_t)b.len, alpha, b.part);
    hipLaunchKernelGGL((jwb::k_gblup_add<real, T>), dim3((unsigned)c->nslices), dim3(256), 0, c->stream, (const real*)r, (const double*)b.part, (int32_t)b.nparts, ld, rplus);
    hipLaunchKernelGGL((jwb::k_gblup_rhs<real, T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, L, ld, n, (const real*)rplus, b.s);
    hipLaunchKernelGGL((jwb::k_gblup_sample<real, T>), dim3((unsigned)b.nwg), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL((jwb::k_gblup_mul<real, T>), grid, dim3(256), 0, c->stream, L, ld, n, (int32_t)b.len, alpha, b.part);
    hipLaunchKernelGGL((jwb::k_gblup_sub<real, T>), dim3((unsigned)c->nslices), dim3(256), 0, c->stream, (const real*)rplus, (const double*)b.part, (int32_t)b.nparts, ld, r, fin);
}

extern "C" {

int jwas_hip_grm(jwas_hip_ctx* c, const void* divisor, void* K_host)
{
    if (int rc = need_dense(c, "relationship matrices")) return rc;
    NEED(c, divisor && K_host, JWAS_HIP_EINVAL, "NULL argument");
    const int64_t n = c->n, p = c->p;
    const bool f64 = IS_F64(c);
    for (int64_t j = 0; j < p; ++j) {
        const double d = f64 ? ((const double*)divisor)[j] : (double)((const float*)divisor)[j];
        NEED(c, std::isfinite(d) && d > 0.0, JWAS_HIP_EINVAL, "divisor[%lld] must be positive and finite (%g)", (long long)j, d);
    }
    const size_t el = f64 ? 8 : 4;
    const int64_t edge = f64 ? jwb::kGrmTile64 : jwb::kGrmTile32, nt = (n + edge - 1) / edge;
    NEED(c, nt * (nt + 1) / 2 < (1ll << 31), JWAS_HIP_EUNSUP, "n=%lld exceeds the tile grid of jwas_hip_grm", (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    DevOwner mem;
    void *d_div = nullptr, *d_K = nullptr;
    if (mem.alloc(&d_div, el * (size_t)p) != hipSuccess || mem.alloc(&d_K, el * (size_t)n * (size_t)n) != hipSuccess) {
        mem.release();
        return fail(c, JWAS_HIP_ENOMEM, "relationship matrix: device allocation of %zu bytes failed", el * ((size_t)n * (size_t)n + (size_t)p));
    }
    hipError_t e = hipMemcpyAsync(d_div, divisor, el * (size_t)p, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        with_real(c, [&](auto real) {
            using real_t = decltype(real);
            hipLaunchKernelGGL((jwb::k_grm<real_t>), dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, c->stream, (const real_t*)genotypes_ptr(c), c->ld, n, p,
                               (const real_t*)d_div, (real_t*)d_K);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(K_host, d_K, el * (size_t)n * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    mem.release();
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "jwas_hip_grm: %s", hipGetErrorString(e));
    return JWAS_HIP_OK;
}

int jwas_hip_grm_packed2bit(jwas_hip_ctx* c, const float* divisor, float* K_host)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, c->packed && c->Q && c->n > 0 && c->p > 0, JWAS_HIP_ESTATE, "the context holds no 2-bit packed genotypes (see jwas_hip_storage_info)");
    if (int rc = refuse_shards(c, "relationship matrices")) return rc;
    NEED(c, divisor && K_host, JWAS_HIP_EINVAL, "NULL argument");
    const int64_t n = c->n, p = c->p;
    for (int64_t j = 0; j < p; ++j) {
        const double d = (double)divisor[j];
        NEED(c, std::isfinite(d) && d > 0.0, JWAS_HIP_EINVAL, "divisor[%lld] must be positive and finite (%g)", (long long)j, d);
    }
    const int64_t nt = (n + jwb::kGrmTile32 - 1) / jwb::kGrmTile32;
    NEED(c, nt * (nt + 1) / 2 < (1ll << 31), JWAS_HIP_EUNSUP, "n=%lld exceeds the tile grid of jwas_hip_grm_packed2bit", (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    DevOwner mem;
    float *d_div = nullptr, *d_K = nullptr;
    if (mem.alloc(&d_div, sizeof(float) * (size_t)p) != hipSuccess || mem.alloc(&d_K, sizeof(float) * (size_t)n * (size_t)n) != hipSuccess) {
        mem.release();
        return fail(c, JWAS_HIP_ENOMEM, "relationship matrix: device allocation of %zu bytes failed", sizeof(float) * ((size_t)n * (size_t)n + (size_t)p));
    }
    hipError_t e = hipMemcpyAsync(d_div, divisor, sizeof(float) * (size_t)p, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(jwb::k_grm_packed, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, c->stream, (const uint8_t*)c->Q, c->ld, (const float*)c->qmean,
                           (int32_t)c->centered, n, p, (const float*)d_div, d_K);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(K_host, d_K, sizeof(float) * (size_t)n * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    mem.release();
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "jwas_hip_grm_packed2bit: %s", hipGetErrorString(e));
    return JWAS_HIP_OK;
}

int64_t jwas_hip_grm_estimate_bytes(int64_t n, int64_t p, int32_t precision_bits)
{
    return (precision_bits == 64 ? 8 : 4) * (std::max<int64_t>(n, 1) * std::max<int64_t>(n, 1) + std::max<int64_t>(p, 1));
}

int jwas_hip_gblup_begin(jwas_hip_ctx* c, const double* D)
{
    if (int rc = need_dense(c, "GBLUP steps")) return rc;
    if (int rc = begin_guard(c, "GBLUP steps")) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "GBLUP does not run with residual weights");
    NEED(c, D, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, c->p == c->n, JWAS_HIP_EINVAL, "GBLUP needs the n x n matrix of eigenvectors (the loaded matrix is %lld x %lld)", (long long)c->n, (long long)c->p);
    NEED(c, c->ntraits >= 1 && c->ntraits <= jwb::kMaxT, JWAS_HIP_EINVAL, "GBLUP runs 1 to %d traits (the state has %d)", jwb::kMaxT, c->ntraits);
    const int64_t n = c->n, ld = c->ld;
    for (int64_t i = 0; i < n; ++i) NEED(c, std::isfinite(D[i]) && D[i] > 0.0, JWAS_HIP_EINVAL, "D[%lld] must be positive and finite (%g)", (long long)i, D[i]);
    if (int rc = session_drop(c, gblup_free)) return rc;
    auto& b = c->gb;
    const int T = c->ntraits;
    const size_t el = IS_F64(c) ? 8 : 4;
    b.nt = T; b.nwg = (int)((n + 255) / 256); b.mat = genotypes_ptr(c);
    gblup_parts(n, c->nslices, b.nparts, b.len);
    auto alloc = [&](auto** ptr, size_t bytes) { return alloc_or_nomem(c, b.mem, ptr, bytes, "GBLUP session", gblup_free); };
    if (int rc = alloc(&b.D, sizeof(double) * (size_t)n)) return rc;
    if (int rc = alloc(&b.rplus, el * (size_t)T * (size_t)ld)) return rc;
    if (int rc = alloc(&b.s, sizeof(double) * (size_t)n * T)) return rc;
    if (int rc = alloc(&b.part, sizeof(double) * (size_t)b.nparts * T * (size_t)ld)) return rc;
    if (int rc = alloc(&b.par, sizeof(double) * jwb::kParSize)) return rc;
    if (int rc = alloc(&b.stat, sizeof(double) * ((size_t)b.nwg * T * T + (size_t)c->nslices * (T * T + T)))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.D, D, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.s, 0, sizeof(double) * (size_t)n * T, c->stream));
    HIPCHK(c, hipMemsetAsync(b.rplus, 0, el * (size_t)T * (size_t)ld, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_gblup_step(jwas_hip_ctx* c, const jwas_gblup_params* P, jwas_gblup_stats* S)
{
    if (int rc = need_gblup(c)) return rc;
    NEED(c, P && S, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_gblup_step: iteration must be >= 1");
    auto& b = c->gb;
    const int T = b.nt;
    NEED(c, (int64_t)P->first_trait + T <= jwb::kMaxT, JWAS_HIP_EINVAL, "first_trait + T must be <= %d (got %u + %d)", jwb::kMaxT, P->first_trait, T);
    const bool diagonal = P->diagonal != 0 || T == 1;
    double par[jwb::kParSize] = {};
    for (int k = 0; k < T; ++k) {
        const double ve = P->vare[k * T + k], g = P->G[k * T + k];
        NEED(c, std::isfinite(ve) && ve > 0.0, JWAS_HIP_EINVAL, "vare[%d,%d] must be positive and finite (%g)", k, k, ve);
        NEED(c, std::isfinite(g) && g > 0.0, JWAS_HIP_EINVAL, "G[%d,%d] must be positive and finite (%g)", k, k, g);
        par[jwb::kParVare + k] = ve;
        par[jwb::kParG + k] = g;
    }
    if (!diagonal) {
        for (int i = 0; i < T * T; ++i) NEED(c, std::isfinite(P->vare[i]) && std::isfinite(P->G[i]), JWAS_HIP_EINVAL, "vare and G must be finite");
        const bool spd = T == 2 ? spd_small<2>(P->vare) && spd_small<2>(P->G) : (T == 3 ? spd_small<3>(P->vare) && spd_small<3>(P->G)
                                                                                         : spd_small<4>(P->vare) && spd_small<4>(P->G));
        NEED(c, spd, JWAS_HIP_EINVAL, "vare and G must be positive definite");
        NEED(c, inv_small<double>(P->vare, T, par + jwb::kParRinv) == 0 && inv_small<double>(P->G, T, par + jwb::kParGinv) == 0, JWAS_HIP_EINVAL,
             "vare or G is singular");
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b.par, par, sizeof(par), hipMemcpyHostToDevice, c->stream));
    if (int rc = step_timer_begin(c)) return rc;
    jwb::SampleArgs A = {};
    A.s = b.s; A.D = b.D; A.par = b.par; A.alpha = alpha_ptr(c); A.beta = beta_ptr(c); A.stat = b.stat; A.n = c->n; A.iter = P->iteration; A.first = P->first_trait;
    A.diagonal = diagonal ? 1 : 0;
    split_seed(P->seed, A.seed_lo, A.seed_hi);
    with_real(c, [&](auto real) {
        using real_t = decltype(real);
        switch (T) {
            case 1: gblup_launch<real_t, 1>(c, A); break;
            case 2: gblup_launch<real_t, 2>(c, A); break;
            case 3: gblup_launch<real_t, 3>(c, A); break;
            default: gblup_launch<real_t, 4>(c, A); break;
        }
    });
    HIPCHK(c, hipGetLastError());
    const int nsl = c->nslices, nf = T * T + T;
    const size_t nstat = (size_t)b.nwg * T * T + (size_t)nsl * nf;
    std::vector<double> host(nstat);
    double ms = 0.0;
    if (int rc = step_timer_end(c, host.data(), b.stat, sizeof(double) * nstat, &ms)) return rc;
    *S = jwas_gblup_stats();
    S->step_ms = ms;
    for (int w = 0; w < b.nwg; ++w)                                                   // workgroups in order
        for (int i = 0; i < T * T; ++i) S->alpha_ss[i] += host[(size_t)w * T * T + i];
    const double* fin = host.data() + (size_t)b.nwg * T * T;
    for (int sl = 0; sl < nsl; ++sl) {                                                // slices in order
        for (int i = 0; i < T * T; ++i) S->resid_ss[i] += fin[(size_t)sl * nf + i];
        for (int k = 0; k < T; ++k) S->resid_sum[k] += fin[(size_t)sl * nf + T * T + k];
    }
    return JWAS_HIP_OK;
}

int jwas_hip_gblup_get_rhs(jwas_hip_ctx* c, int64_t nvalues, double* out)
{
    if (int rc = need_gblup(c)) return rc;
    return download(c, c->gb.s, c->n * c->gb.nt, nvalues, out);
}

int64_t jwas_hip_gblup_estimate_bytes(int64_t n, int32_t ntraits, int32_t precision_bits)
{
    // D, the right-hand sides, the column-part sums, the parameters, the statistics' partials and r+
    return gblup_bytes(std::max<int64_t>(n, 1), std::min(std::max(ntraits, 1), jwb::kMaxT), precision_bits);
}

int jwas_hip_gblup_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::gb, "jwas_hip_gblup_begin")) return rc;
    return session_drop(c, gblup_free);
}

}  // extern "C"
