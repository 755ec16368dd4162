// session_rrm.hip -- random regression models (rrm.hpp), jwas_hip_rrm_begin .. _end: RRM/RRM.jl:43-57,101-158 and the marker part of
// RRM/MCMC_BayesianAlphabet_RRM.jl.
#include "ctx.hpp"
#include "marker_state.hpp"
#include "rrm.hpp"
#include <type_traits>

static int need_rrm(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::rr, "jwas_hip_rrm_begin")) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "random regression models do not run with residual weights");
    return refuse_shards(c, "random regression models");
}

void rrm_free(jwas_hip_ctx* c) { DevOwner::reset(c->rr); }

// f(real{}, integral_constant<C>{}) with the context's element type and the session's number of coefficients
template <class F>
static void with_real_c(jwas_hip_ctx* c, int C, F&& f)
{
    with_real(c, [&](auto real) {
        if (C == 2) f(real, std::integral_constant<int, 2>{});
        else if (C == 3) f(real, std::integral_constant<int, 3>{});
        else f(real, std::integral_constant<int, 4>{});
    });
}

static int64_t rrm_bytes(int64_t n, int64_t p, int T, int C, int bs)
{
    const int64_t ld = round_up(n, 256), cells = jwr::cells_of(C), nblocks = (p + bs - 1) / bs;
    return 8 * (ld + (int64_t)T * C + cells * ld + (int64_t)T * ld + p * cells + nblocks * bs * bs * cells + 6 * (int64_t)C * p +
                (ld / 256) * bs * C + jwr::kStSize + ld / 256 + ld) + (int64_t)sizeof(jwr::Events);
}

extern "C" {

int jwas_hip_rrm_begin(jwas_hip_ctx* c, int32_t T, int32_t C, int64_t n, const double* phi, const uint64_t* mask, int32_t block_size)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, !c->packed, JWAS_HIP_EUNSUP, "random regression models need dense genotypes (the reference refuses RRM on storage=:stream)");
    NEED(c, genotypes_ptr(c) && c->n > 0 && c->p > 0, JWAS_HIP_ESTATE, "no genotype matrix loaded");
    if (int rc = refuse_shards(c, "random regression models")) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "random regression models do not run with residual weights");
    NEED(c, C >= jwr::kMinC && C <= jwr::kMaxC, JWAS_HIP_EINVAL, "the number of regression coefficients must be in [%d,%d] (got %d)", jwr::kMinC, jwr::kMaxC, C);
    NEED(c, T >= 1 && T <= jwr::kMaxT, JWAS_HIP_EINVAL, "the number of time points must be in [1,%d] (got %d)", jwr::kMaxT, T);
    NEED(c, n == c->n, JWAS_HIP_EINVAL, "n (%lld) differs from the number of genotyped individuals (%lld)", (long long)n, (long long)c->n);
    NEED(c, block_size >= 0 && block_size <= jwr::kMaxBlock, JWAS_HIP_EINVAL, "block size must be in [1,%d] (0: 64), got %d", jwr::kMaxBlock, block_size);
    NEED(c, phi && mask, JWAS_HIP_EINVAL, "NULL argument");
    for (int i = 0; i < T * C; ++i) NEED(c, std::isfinite(phi[i]), JWAS_HIP_EINVAL, "Phi[%d][%d] is not finite (%g)", i / C, i % C, phi[i]);
    if (T < 64)
        for (int64_t i = 0; i < n; ++i)
            NEED(c, (mask[i] >> T) == 0, JWAS_HIP_EINVAL, "individual %lld has a record bit at or above T = %d", (long long)i, T);
    if (int rc = session_drop(c, rrm_free)) return rc;
    auto& b = c->rr;
    const int bs = block_size ? block_size : 64;
    const int64_t p = c->p, ld = c->ld, cells = jwr::cells_of(C);
    b.T = T; b.C = C; b.bs = bs; b.nblocks = (p + bs - 1) / bs;
    b.mask_host.assign(mask, mask + n);
    auto alloc = [&](auto** ptr, size_t bytes) { return alloc_or_nomem(c, b.mem, ptr, bytes, "RRM session", rrm_free); };
    const size_t gramb = sizeof(double) * (size_t)b.nblocks * bs * bs * cells;
    jwr::Events* ev = nullptr;
    if (int rc = alloc(&b.mask, sizeof(uint64_t) * (size_t)ld)) return rc;
    if (int rc = alloc(&b.phi, sizeof(double) * (size_t)T * C)) return rc;
    if (int rc = alloc(&b.O, sizeof(double) * (size_t)cells * ld)) return rc;
    if (int rc = alloc(&b.W, sizeof(double) * (size_t)T * ld)) return rc;
    if (int rc = alloc(&b.M, sizeof(double) * (size_t)p * cells)) return rc;
    if (int rc = alloc(&b.gram, gramb)) return rc;
    if (int rc = marker_state_begin(c, b.ms, b.mem, C, "RRM session", rrm_free)) return rc;      // (Mi.δ = 1, MCMC_BayesianAlphabet_RRM.jl:53)
    if (int rc = alloc(&b.partials, sizeof(double) * (size_t)c->nslices * bs * C)) return rc;
    if (int rc = alloc(&b.stat, sizeof(double) * (size_t)(jwr::kStSize + c->nslices))) return rc;
    if (int rc = alloc(&b.row, sizeof(double) * (size_t)ld)) return rc;
    if (int rc = alloc(&ev, sizeof(jwr::Events))) return rc;
    b.ev = ev;
    HIPCHK(c, hipMemsetAsync(b.mask, 0, sizeof(uint64_t) * (size_t)ld, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.mask, mask, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.phi, phi, sizeof(double) * (size_t)T * C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.W, 0, sizeof(double) * (size_t)T * ld, c->stream));
    HIPCHK(c, hipMemsetAsync(b.gram, 0, gramb, c->stream));
    HIPCHK(c, hipMemsetAsync(ev, 0, sizeof(jwr::Events), c->stream));
    hipLaunchKernelGGL(jwr::k_rrm_o, dim3((unsigned)c->nslices), dim3(256), 0, c->stream, (const uint64_t*)b.mask, (const double*)b.phi, T, C, ld, b.O);
    with_real_c(c, C, [&](auto real, auto cc) {
        using real_t = decltype(real);
        constexpr int CC = decltype(cc)::value;
        hipLaunchKernelGGL((jwr::k_rrm_m<real_t, CC>), dim3((unsigned)p), dim3(256), 0, c->stream, (const real_t*)genotypes_ptr(c), ld, (const double*)b.O, b.M);
        // (the grid's y extent is 65 535 blocks at most: the blocks go in trips)
        for (int64_t k0 = 0; k0 < b.nblocks; k0 += 32768) {
            const int64_t nb = std::min<int64_t>(32768, b.nblocks - k0);
            hipLaunchKernelGGL((jwr::k_rrm_gram<real_t, CC>), dim3((unsigned)bs, (unsigned)nb), dim3(256), 0, c->stream,
                               (const real_t*)genotypes_ptr(c) + k0 * bs * ld, ld, (const double*)b.O, p - k0 * bs, (int32_t)bs, b.gram + k0 * bs * bs * cells);
        }
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the caller's arrays may go away once this returns)
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_rrm_set_residual(jwas_hip_ctx* c, int64_t nvalues, const double* W)
{
    if (int rc = need_rrm(c)) return rc;
    auto& b = c->rr;
    NEED(c, W, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, nvalues == (int64_t)b.T * c->n, JWAS_HIP_EINVAL, "nvalues (%lld) differs from T n (%lld)", (long long)nvalues, (long long)((int64_t)b.T * c->n));
    std::vector<double> host((size_t)b.T * (size_t)c->ld, 0.0);
    for (int t = 0; t < b.T; ++t)
        for (int64_t i = 0; i < c->n; ++i) {
            const double v = W[(size_t)t * c->n + i];
            if ((b.mask_host[(size_t)i] >> t) & 1ull) {
                NEED(c, std::isfinite(v), JWAS_HIP_EINVAL, "the residual of individual %lld at time %d is not finite (%g)", (long long)i, t, v);
                host[(size_t)t * c->ld + i] = v;
            }
        }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b.W, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_rrm_get_residual(jwas_hip_ctx* c, int64_t nvalues, double* out)
{
    if (int rc = need_rrm(c)) return rc;
    auto& b = c->rr;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, nvalues == (int64_t)b.T * c->n, JWAS_HIP_EINVAL, "nvalues (%lld) differs from T n (%lld)", (long long)nvalues, (long long)((int64_t)b.T * c->n));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double) * (size_t)c->n, b.W, sizeof(double) * (size_t)c->ld, sizeof(double) * (size_t)c->n, (size_t)b.T,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_rrm_set_state(jwas_hip_ctx* c, const double* alpha, const double* beta, const double* delta)
{
    if (int rc = need_rrm(c)) return rc;
    return marker_state_set(c, c->rr.ms, 0, c->rr.C, alpha, beta, delta);
}

int jwas_hip_rrm_get_state(jwas_hip_ctx* c, double* alpha, double* beta, double* delta)
{
    if (int rc = need_rrm(c)) return rc;
    return marker_state_get(c, c->rr.ms, 0, c->rr.C, alpha, beta, delta);
}

int jwas_hip_rrm_sweep(jwas_hip_ctx* c, const jwas_rrm_params* P, jwas_rrm_stats* S)
{
    if (int rc = need_rrm(c)) return rc;
    NEED(c, P && S, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_rrm_sweep: iteration must be >= 1");
    NEED(c, std::isfinite(P->vare) && P->vare > 0.0, JWAS_HIP_EINVAL, "vare must be positive and finite (%g)", P->vare);
    auto& b = c->rr;
    const int C = b.C, NS = 1 << C, cells = jwr::cells_of(C);
    double G[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS], Gi[JWAS_HIP_MAX_TRAITS * JWAS_HIP_MAX_TRAITS], L[jwr::kMaxC][jwr::kMaxC] = {};
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
            G[i * C + j] = P->G[i * C + j];
            NEED(c, std::isfinite(G[i * C + j]), JWAS_HIP_EINVAL, "G[%d][%d] is not finite (%g)", i, j, G[i * C + j]);
            NEED(c, P->G[i * C + j] == P->G[j * C + i], JWAS_HIP_EINVAL, "G is not symmetric ([%d][%d] = %g, [%d][%d] = %g)", i, j, P->G[i * C + j], j, i, P->G[j * C + i]);
        }
    for (int i = 0; i < C; ++i)                        // positive definite: its Cholesky factor exists
        for (int j = 0; j <= i; ++j) {
            double s = G[i * C + j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                NEED(c, s > 0.0, JWAS_HIP_EINVAL, "G is not positive definite (pivot %d: %g)", i, s);
                L[i][i] = std::sqrt(s);
            } else L[i][j] = s / L[j][j];
        }
    NEED(c, inv_small<double>(G, C, Gi) == 0, JWAS_HIP_EINVAL, "G is singular");
    bool any = false;
    for (int s = 0; s < NS; ++s) {
        NEED(c, !std::isnan(P->log_pi[s]) && P->log_pi[s] < INFINITY, JWAS_HIP_EINVAL, "log_pi[%d] must be finite or -Inf (%g)", s, P->log_pi[s]);
        any = any || std::isfinite(P->log_pi[s]);
    }
    NEED(c, any, JWAS_HIP_EINVAL, "every state has prior probability 0");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = step_timer_begin(c)) return rc;
    HIPCHK(c, hipMemsetAsync(b.stat, 0, sizeof(double) * (size_t)(jwr::kStSize + c->nslices), c->stream));
    jwr::UpdateArgs U = {};
    U.X = genotypes_ptr(c); U.mask = b.mask; U.phi = b.phi; U.W = b.W; U.partials = b.partials; U.ld = c->ld; U.T = b.T; U.bs = b.bs;
    jwr::SampleArgs A = {};
    A.partials = b.partials; A.M = b.M; A.phi = b.phi; A.alpha = b.ms.alpha; A.beta = b.ms.beta; A.delta = b.ms.delta; A.ev = (jwr::Events*)b.ev;
    A.stat = b.stat; A.ie = 1.0 / P->vare; A.p = c->p; A.nslices = c->nslices; A.bs = b.bs; A.T = b.T; A.iter = P->iteration;
    split_seed(P->seed, A.seed_lo, A.seed_hi);
    for (int i = 0; i < C * C; ++i) A.Ginv[i] = Gi[i];
    for (int s = 0; s < NS; ++s) A.lpi[s] = P->log_pi[s];
    jwr::FinishArgs F = {};
    F.X = genotypes_ptr(c); F.mask = b.mask; F.W = b.W; F.ev = (const jwr::Events*)b.ev; F.wss = b.stat + jwr::kStSize; F.ld = c->ld; F.T = b.T;
    const dim3 slices((unsigned)c->nslices);
    with_real_c(c, C, [&](auto real, auto cc) {
        using real_t = decltype(real);
        constexpr int CC = decltype(cc)::value;
        for (int64_t k = 0; k < b.nblocks; ++k) {
            const int64_t j0 = k * b.bs;
            U.ev = k ? (const jwr::Events*)b.ev : nullptr; U.j0 = j0; U.b = (int32_t)std::min<int64_t>(b.bs, c->p - j0);
            A.gram = b.gram + k * (int64_t)b.bs * b.bs * cells; A.j0 = j0; A.b = U.b;
            hipLaunchKernelGGL((jwr::k_rrm_update_partial<real_t, CC>), slices, dim3(256), 0, c->stream, U);
            hipLaunchKernelGGL((jwr::k_rrm_sample<CC>), dim3(1), dim3(256), 0, c->stream, A);
        }
        hipLaunchKernelGGL((jwr::k_rrm_finish<real_t>), slices, dim3(256), 0, c->stream, F);
    });
    HIPCHK(c, hipGetLastError());
    std::vector<double> host((size_t)(jwr::kStSize + c->nslices));
    std::memset(S, 0, sizeof *S);
    if (int rc = step_timer_end(c, host.data(), b.stat, sizeof(double) * host.size(), &S->step_ms)) return rc;
    for (int s = 0; s < NS; ++s) S->state_counts[s] = host[jwr::kStCounts + s];
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) S->beta_ss[i * C + j] = host[jwr::kStBeta + jwr::cell(i, j)];
    S->alpha_ss = host[jwr::kStAlpha];
    S->n_changed = host[jwr::kStChanged];
    double wss = 0.0;
    for (int sl = 0; sl < c->nslices; ++sl) wss += host[(size_t)jwr::kStSize + sl];       // slices in order
    S->resid_ss = wss;
    return JWAS_HIP_OK;
}

int jwas_hip_rrm_accumulate(jwas_hip_ctx* c, double nsamples)
{
    if (int rc = need_rrm(c)) return rc;
    return marker_state_accumulate<false>(c, c->rr.ms, c->rr.C, nsamples);
}

int jwas_hip_rrm_get_posterior(jwas_hip_ctx* c, int32_t q, double* mean, double* mean2, double* freq)
{
    if (int rc = need_rrm(c)) return rc;
    NEED(c, q >= 0 && q < c->rr.C, JWAS_HIP_EINVAL, "coefficient %d outside [0,%d)", q, c->rr.C);
    return marker_state_posterior(c, c->rr.ms, q, mean, mean2, freq);
}

int jwas_hip_rrm_mul_alpha(jwas_hip_ctx* c, int32_t q, double* out)
{
    if (int rc = need_rrm(c)) return rc;
    auto& b = c->rr;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, q >= 0 && q < b.C, JWAS_HIP_EINVAL, "coefficient %d outside [0,%d)", q, b.C);
    HIPCHK(c, hipSetDevice(c->device));
    return marker_state_mul_alpha(c, b.ms, q, genotypes_ptr(c), c->ld, c->n, b.row, out);
}

int jwas_hip_rrm_get_m(jwas_hip_ctx* c, int64_t nvalues, double* out)
{
    if (int rc = need_rrm(c)) return rc;
    return download(c, c->rr.M, c->p * jwr::cells_of(c->rr.C), nvalues, out);
}

int jwas_hip_rrm_get_gram(jwas_hip_ctx* c, int64_t block, int64_t nvalues, double* out)
{
    if (int rc = need_rrm(c)) return rc;
    auto& b = c->rr;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, block >= 0 && block < b.nblocks, JWAS_HIP_EINVAL, "block %lld outside [0,%lld)", (long long)block, (long long)b.nblocks);
    const int64_t cells = jwr::cells_of(b.C), nb = std::min<int64_t>(b.bs, c->p - block * b.bs);
    NEED(c, nvalues == nb * nb * cells, JWAS_HIP_EINVAL, "nvalues (%lld) differs from b b cells (%lld)", (long long)nvalues, (long long)(nb * nb * cells));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double) * (size_t)(nb * cells), b.gram + block * b.bs * b.bs * cells, sizeof(double) * (size_t)(b.bs * cells),
                               sizeof(double) * (size_t)(nb * cells), (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int64_t jwas_hip_rrm_estimate_bytes(int64_t n, int64_t p, int32_t T, int32_t C, int32_t block_size)
{
    // the mask, Phi, O, the residual, M, the Gram tensor (8 p b c (c + 1) / 2 for whole blocks), the state and its running means,
    // the slice partials, the statistics, a row vector and the change list
    return rrm_bytes(std::max<int64_t>(n, 1), std::max<int64_t>(p, 1), std::max(T, 1), std::min(std::max(C, jwr::kMinC), jwr::kMaxC),
                     block_size > 0 ? std::min(block_size, jwr::kMaxBlock) : 64);
}

int jwas_hip_rrm_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::rr, "jwas_hip_rrm_begin")) return rc;
    return session_drop(c, rrm_free);
}

}  // extern "C"
