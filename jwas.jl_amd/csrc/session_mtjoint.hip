// session_mtjoint.hip -- unconstrained multi-trait BayesC with 5 to 8 traits (mtjoint.hpp), jwas_hip_mtj_begin .. _end: Gibbs sampler I
// (_MTBayesABC_samplerI!, markers/BayesianAlphabet/MTBayesABC.jl:57-127) on the block form of the mega-trait session (mega.hpp).
#include "ctx.hpp"
#include "marker_state.hpp"
#include "mtjoint.hpp"

static_assert(jwj::kMinT == JWAS_HIP_MTJ_MIN_TRAITS && jwj::kMaxT == JWAS_HIP_MTJ_MAX_TRAITS, "the header's limits are mtjoint.hpp's");

static int need_mtj(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::mj, "jwas_hip_mtj_begin")) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "the joint multi-trait session does not run with residual weights");
    return refuse_shards(c, "joint multi-trait models");
}

static int need_trait(jwas_hip_ctx* c, int32_t trait)
{
    if (int rc = need_mtj(c)) return rc;
    NEED(c, trait >= 0 && trait < c->mj.nt, JWAS_HIP_EINVAL, "trait %d outside [0,%d)", trait, c->mj.nt);
    return JWAS_HIP_OK;
}

void mtj_free(jwas_hip_ctx* c) { DevOwner::reset(c->mj); }

// a T x T matrix of the caller -> dst (row stride kMaxT, the rest 0): finite, symmetric, positive definite (its Cholesky factor exists)
static int mtj_matrix(jwas_hip_ctx* c, const double* M, int T, const char* name, double* dst)
{
    NEED(c, M, JWAS_HIP_EINVAL, "jwas_hip_mtj_sweep: %s is NULL", name);
    double L[jwj::kMaxT][jwj::kMaxT] = {};
    for (int a = 0; a < T; ++a)
        for (int b = 0; b < T; ++b) {
            const double v = M[a * T + b], w = M[b * T + a];
            NEED(c, std::isfinite(v), JWAS_HIP_EINVAL, "%s[%d][%d] is not finite (%g)", name, a, b, v);
            // (an inverse formed by Gauss-Jordan is symmetric to rounding only: 1e-8 of the geometric mean of the two diagonal entries)
            NEED(c, std::fabs(v - w) <= 1e-8 * std::sqrt(std::fabs(M[a * T + a] * M[b * T + b])), JWAS_HIP_EINVAL, "%s is not symmetric at [%d][%d] (%g, %g)",
                 name, a, b, v, w);
            dst[a * jwj::kMaxT + b] = v;
        }
    for (int a = 0; a < T; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = M[a * T + b];
            for (int k = 0; k < b; ++k) s -= L[a][k] * L[b][k];
            if (a == b) {
                NEED(c, s > 0.0, JWAS_HIP_EINVAL, "%s is not positive definite (pivot %d: %g)", name, a, s);
                L[a][a] = std::sqrt(s);
            } else {
                L[a][b] = s / L[b][b];
            }
        }
    return JWAS_HIP_OK;
}

// checked, then par_host = Rinv | Ginv | log pi
static int mtj_params(jwas_hip_ctx* c, const jwas_mtj_params* P)
{
    auto& b = c->mj;
    NEED(c, P, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_mtj_sweep: iteration must be >= 1");
    const int T = b.nt;
    const int64_t ns = (int64_t)1 << T;
    b.par_host.assign((size_t)jwj::kParSize, 0.0);
    if (int rc = mtj_matrix(c, P->rinv, T, "rinv", b.par_host.data() + jwj::kParRinv)) return rc;
    if (int rc = mtj_matrix(c, P->ginv, T, "ginv", b.par_host.data() + jwj::kParGinv)) return rc;
    NEED(c, P->log_pi && P->npi == ns, JWAS_HIP_EINVAL, "the Pi table must hold 2^T = %lld values (got %lld)", (long long)ns, (long long)P->npi);
    bool some = false;
    for (int64_t q = 0; q < jwj::kMaxStates; ++q) {
        double v = -INFINITY;
        if (q < ns) {
            v = P->log_pi[q];
            NEED(c, !std::isnan(v) && v <= 0.0, JWAS_HIP_EINVAL, "log_pi[%lld] must be -Inf or a finite value <= 0 (%g)", (long long)q, v);
            some = some || std::isfinite(v);
        }
        b.par_host[(size_t)jwj::kParLogPi + (size_t)q] = v;
    }
    NEED(c, some, JWAS_HIP_EINVAL, "no joint state has a positive probability");
    return JWAS_HIP_OK;
}

extern "C" {

int jwas_hip_mtj_begin(jwas_hip_ctx* c, int32_t T, int32_t block_size)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, !c->packed, JWAS_HIP_EUNSUP, "joint multi-trait models need dense genotypes (2-bit packed storage is not supported)");
    NEED(c, genotypes_ptr(c) && c->n > 0 && c->p > 0, JWAS_HIP_ESTATE, "no genotype matrix loaded");
    if (int rc = refuse_shards(c, "joint multi-trait models")) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "the joint multi-trait session does not run with residual weights");
    NEED(c, T >= jwj::kMinT && T <= jwj::kMaxT, JWAS_HIP_EINVAL, "the number of traits must be in [%d,%d] (got %d)", jwj::kMinT, jwj::kMaxT, T);
    NEED(c, block_size >= 0 && block_size <= jwg::kMaxBlock, JWAS_HIP_EINVAL, "block size must be in [1,%d] (0: 64), got %d", jwg::kMaxBlock, block_size);
    if (int rc = session_drop(c, mtj_free)) return rc;
    auto& b = c->mj;
    const int bs = block_size ? block_size : 64;
    const int64_t p = c->p, ld = c->ld;
    b.nt = T; b.bs = bs; b.nblocks = (p + bs - 1) / bs; b.row_cap = ld;
    auto alloc = [&](auto** ptr, size_t bytes) { return alloc_or_nomem(c, b.mem, ptr, bytes, "joint multi-trait session", mtj_free); };
    const size_t gramb = sizeof(double) * (size_t)b.nblocks * bs * bs;
    const size_t statb = sizeof(double) * ((size_t)jwj::kStSize + (size_t)c->nslices * jwj::kRec);
    jwg::Events* ev = nullptr;
    if (int rc = alloc(&b.R, sizeof(double) * (size_t)T * ld)) return rc;
    if (int rc = alloc(&b.xpx, sizeof(double) * (size_t)p)) return rc;
    if (int rc = alloc(&b.gram, gramb)) return rc;
    if (int rc = marker_state_begin(c, b.ms, b.mem, T, "joint multi-trait session", mtj_free)) return rc;
    if (int rc = alloc(&b.partials, sizeof(double) * (size_t)c->nslices * T * bs)) return rc;
    if (int rc = alloc(&b.par, sizeof(double) * (size_t)jwj::kParSize)) return rc;
    if (int rc = alloc(&b.stat, statb)) return rc;
    if (int rc = alloc(&b.row, sizeof(double) * (size_t)ld)) return rc;
    if (int rc = alloc(&ev, sizeof(jwg::Events))) return rc;
    b.ev = ev;
    HIPCHK(c, hipMemsetAsync(b.R, 0, sizeof(double) * (size_t)T * ld, c->stream));
    HIPCHK(c, hipMemsetAsync(b.gram, 0, gramb, c->stream));
    HIPCHK(c, hipMemsetAsync(ev, 0, sizeof(jwg::Events), c->stream));
    with_real(c, [&](auto real) {
        using real_t = decltype(real);
        // (the grid's y extent is 65 535 blocks at most: the blocks go in trips)
        for (int64_t k0 = 0; k0 < b.nblocks; k0 += 32768) {
            const int64_t nb = std::min<int64_t>(32768, b.nblocks - k0);
            hipLaunchKernelGGL((jwg::k_mega_gram<real_t>), dim3((unsigned)bs, (unsigned)nb), dim3(256), 0, c->stream,
                               (const real_t*)genotypes_ptr(c) + k0 * bs * ld, ld, p - k0 * bs, (int32_t)bs, b.gram + k0 * bs * bs, b.xpx + k0 * bs);
        }
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_mtj_set_residual(jwas_hip_ctx* c, int32_t trait, const double* r)
{
    if (int rc = need_trait(c, trait)) return rc;
    NEED(c, r, JWAS_HIP_EINVAL, "NULL argument");
    for (int64_t i = 0; i < c->n; ++i) NEED(c, std::isfinite(r[i]), JWAS_HIP_EINVAL, "the residual of record %lld is not finite (%g)", (long long)i, r[i]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->mj.R + (size_t)trait * c->ld, r, sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_mtj_get_residual(jwas_hip_ctx* c, int32_t trait, double* out)
{
    if (int rc = need_trait(c, trait)) return rc;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, out, c->mj.R + (size_t)trait * c->ld, sizeof(double) * (size_t)c->n);
}

int jwas_hip_mtj_set_state(jwas_hip_ctx* c, int32_t trait, const double* alpha, const double* beta, const double* delta)
{
    if (int rc = need_trait(c, trait)) return rc;
    return marker_state_set(c, c->mj.ms, trait, 1, alpha, beta, delta);
}

int jwas_hip_mtj_get_state(jwas_hip_ctx* c, int32_t trait, double* alpha, double* beta, double* delta)
{
    if (int rc = need_trait(c, trait)) return rc;
    return marker_state_get(c, c->mj.ms, trait, 1, alpha, beta, delta);
}

int jwas_hip_mtj_gram(jwas_hip_ctx* c, int64_t block, int64_t nvalues, double* out, double* out_xpx)
{
    if (int rc = need_mtj(c)) return rc;
    auto& b = c->mj;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, block >= 0 && block < b.nblocks, JWAS_HIP_EINVAL, "block %lld outside [0,%lld)", (long long)block, (long long)b.nblocks);
    const int64_t nb = std::min<int64_t>(b.bs, c->p - block * b.bs);
    NEED(c, nvalues == nb * nb, JWAS_HIP_EINVAL, "nvalues (%lld) differs from b b (%lld)", (long long)nvalues, (long long)(nb * nb));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double) * (size_t)nb, b.gram + block * b.bs * b.bs, sizeof(double) * (size_t)b.bs, sizeof(double) * (size_t)nb, (size_t)nb,
                               hipMemcpyDeviceToHost, c->stream));
    if (out_xpx) HIPCHK(c, hipMemcpyAsync(out_xpx, b.xpx + block * b.bs, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_mtj_sweep(jwas_hip_ctx* c, const jwas_mtj_params* P, jwas_mtj_stats* S)
{
    if (int rc = need_mtj(c)) return rc;
    NEED(c, S, JWAS_HIP_EINVAL, "NULL argument");
    if (int rc = mtj_params(c, P)) return rc;
    auto& b = c->mj;
    const int T = b.nt, nsl = c->nslices;
    const size_t nstat = (size_t)jwj::kStSize + (size_t)nsl * jwj::kRec;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b.par, b.par_host.data(), sizeof(double) * b.par_host.size(), hipMemcpyHostToDevice, c->stream));
    if (int rc = step_timer_begin(c)) return rc;
    HIPCHK(c, hipMemsetAsync(b.stat, 0, sizeof(double) * nstat, c->stream));
    jwg::UpdateArgs U = {};
    U.X = genotypes_ptr(c); U.R = b.R; U.partials = b.partials; U.ld = c->ld; U.T = T; U.bs = b.bs;
    jwj::SampleArgs A = {};
    A.partials = b.partials; A.xpx = b.xpx; A.par = b.par; A.alpha = b.ms.alpha; A.beta = b.ms.beta; A.delta = b.ms.delta; A.ev = (jwg::Events*)b.ev;
    A.stat = b.stat; A.p = c->p; A.nslices = nsl; A.bs = b.bs; A.T = T; A.iter = P->iteration;
    split_seed(P->seed, A.seed_lo, A.seed_hi);
    jwj::FinishArgs F = {};
    F.X = genotypes_ptr(c); F.R = b.R; F.ev = (const jwg::Events*)b.ev; F.fin = b.stat + jwj::kStSize; F.ld = c->ld; F.T = T;
    with_real(c, [&](auto real) {
        using real_t = decltype(real);
        for (int64_t k = 0; k < b.nblocks; ++k) {
            const int64_t j0 = k * b.bs;
            U.ev = k ? (const jwg::Events*)b.ev : nullptr; U.j0 = j0; U.b = (int32_t)std::min<int64_t>(b.bs, c->p - j0);
            A.gram = b.gram + k * (int64_t)b.bs * b.bs; A.j0 = j0; A.b = U.b;
            hipLaunchKernelGGL((jwg::k_mega_update_partial<real_t>), dim3((unsigned)nsl, 1u), dim3(256), 0, c->stream, U);
            hipLaunchKernelGGL(jwj::k_mtj_sample, dim3(1), dim3(256), 0, c->stream, A);
        }
        hipLaunchKernelGGL((jwj::k_mtj_finish<real_t>), dim3((unsigned)nsl), dim3(256), 0, c->stream, F);
    });
    HIPCHK(c, hipGetLastError());
    std::vector<double> host(nstat);
    if (int rc = step_timer_end(c, host.data(), b.stat, sizeof(double) * nstat, &S->step_ms)) return rc;
    if (S->state_counts)
        for (int q = 0; q < (1 << T); ++q) S->state_counts[q] = host[(size_t)jwj::kStCounts + q];
    for (int k = 0; k < T; ++k) {
        if (S->beta_ss)
            for (int l = 0; l < T; ++l) S->beta_ss[k * T + l] = host[(size_t)jwj::kStBB + k * jwj::kMaxT + l];
        if (S->alpha_ss) S->alpha_ss[k] = host[(size_t)jwj::kStAA + k];
    }
    S->n_changed = host[jwj::kStChanged];
    // the residual sums: the slices in ascending order; pair q of a slice's record is (k, l), k <= l, row by row over kMaxT traits
    const double* fin = host.data() + jwj::kStSize;
    int q = 0;
    for (int k = 0; k < jwj::kMaxT; ++k)
        for (int l = k; l < jwj::kMaxT; ++l, ++q) {
            if (l >= T || !S->resid_cp) continue;
            double s = 0.0;
            for (int sl = 0; sl < nsl; ++sl) s += fin[(size_t)sl * jwj::kRec + q];
            S->resid_cp[k * T + l] = s;
            S->resid_cp[l * T + k] = s;
        }
    if (S->resid_sum)
        for (int k = 0; k < T; ++k) {
            double s = 0.0;
            for (int sl = 0; sl < nsl; ++sl) s += fin[(size_t)sl * jwj::kRec + jwj::kPairs + k];
            S->resid_sum[k] = s;
        }
    return JWAS_HIP_OK;
}

int jwas_hip_mtj_accumulate(jwas_hip_ctx* c, double nsamples)
{
    if (int rc = need_mtj(c)) return rc;
    return marker_state_accumulate<false>(c, c->mj.ms, c->mj.nt, nsamples);
}

int jwas_hip_mtj_posterior(jwas_hip_ctx* c, int32_t trait, double* mean, double* mean2, double* freq)
{
    if (int rc = need_trait(c, trait)) return rc;
    return marker_state_posterior(c, c->mj.ms, trait, mean, mean2, freq);
}

int jwas_hip_mtj_mul_alpha(jwas_hip_ctx* c, int32_t trait, int32_t use_output_rows, double* out)
{
    if (int rc = need_trait(c, trait)) return rc;
    auto& b = c->mj;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    const void* X = genotypes_ptr(c);
    int64_t n = c->n, ld = c->ld;
    if (use_output_rows) {
        X = output_rows_ptr(c, &n, &ld);
        NEED(c, X, JWAS_HIP_ESTATE, "no output rows loaded (jwas_hip_load_output_dense_f32 / _f64)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (ld > b.row_cap) {                                   // the output rows may outnumber the training rows
        HIPCHK(c, hipStreamSynchronize(c->stream));
        b.mem.free_one(b.row);
        b.row_cap = 0;
        if (int rc = alloc_or_nomem(c, b.mem, &b.row, sizeof(double) * (size_t)ld, "joint multi-trait session", mtj_free)) return rc;
        b.row_cap = ld;
    }
    return marker_state_mul_alpha(c, b.ms, trait, X, ld, n, b.row, out);
}

int jwas_hip_mtj_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::mj, "jwas_hip_mtj_begin")) return rc;
    return session_drop(c, mtj_free);
}

}  // extern "C"
