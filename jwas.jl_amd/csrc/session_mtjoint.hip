// session_mtjoint.hip -- unconstrained multi-trait BayesC with 5 to 8 traits (mtjoint.hpp), jwas_hip_mtj_begin .. _end: Gibbs sampler I
// (_MTBayesABC_samplerI!, markers/BayesianAlphabet/MTBayesABC.jl:57-127) on the block form of the mega-trait session (mega.hpp).
#include "mtjoint.hpp"      // (first: it takes the block form of mega.hpp alone, without the mega-trait samplers)
#include "block_session.hpp"

static_assert(jwj::kMinT == JWAS_HIP_MTJ_MIN_TRAITS && jwj::kMaxT == JWAS_HIP_MTJ_MAX_TRAITS, "the header's limits are mtjoint.hpp's");

void mtj_free(jwas_hip_ctx* c) { DevOwner::reset(c->mj); }

static const BlockWords kMtj = {"joint multi-trait session", "joint multi-trait models", "the joint multi-trait session does not run with residual weights",
                                "jwas_hip_mtj_begin", mtj_free};

static int need_mtj(jwas_hip_ctx* c) { return block_guard(c, &jwas_hip_ctx::mj, kMtj); }
static int need_trait(jwas_hip_ctx* c, int32_t trait) { return block_trait_guard(c, &jwas_hip_ctx::mj, kMtj, trait); }

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
    if (int rc = block_begin_guard(c, kMtj, T, jwj::kMinT, jwj::kMaxT, block_size)) return rc;
    return block_begin(c, c->mj, kMtj, T, block_size, (size_t)jwj::kParSize, (size_t)jwj::kStSize + (size_t)c->nslices * jwj::kRec,
                       [](auto) { return JWAS_HIP_OK; });
}

int jwas_hip_mtj_set_residual(jwas_hip_ctx* c, int32_t trait, const double* r)
{
    if (int rc = need_trait(c, trait)) return rc;
    return block_set_residual(c, c->mj, trait, r);
}

int jwas_hip_mtj_get_residual(jwas_hip_ctx* c, int32_t trait, double* out)
{
    if (int rc = need_trait(c, trait)) return rc;
    return block_get_residual(c, c->mj, trait, out);
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
    return block_get_gram(c, c->mj, block, nvalues, out, out_xpx);
}

int jwas_hip_mtj_sweep(jwas_hip_ctx* c, const jwas_mtj_params* P, jwas_mtj_stats* S)
{
    if (int rc = need_mtj(c)) return rc;
    NEED(c, S, JWAS_HIP_EINVAL, "NULL argument");
    if (int rc = mtj_params(c, P)) return rc;
    auto& b = c->mj;
    const int T = b.nt, nsl = c->nslices;
    jwj::SampleArgs A = {};
    A.partials = b.partials; A.xpx = b.xpx; A.par = b.par; A.alpha = b.ms.alpha; A.beta = b.ms.beta; A.delta = b.ms.delta; A.ev = (jwg::Events*)b.ev;
    A.stat = b.stat; A.p = c->p; A.nslices = nsl; A.bs = b.bs; A.T = T; A.iter = P->iteration;
    split_seed(P->seed, A.seed_lo, A.seed_hi);
    jwj::FinishArgs F = {};
    F.X = genotypes_ptr(c); F.R = b.R; F.ev = (const jwg::Events*)b.ev; F.fin = b.stat + jwj::kStSize; F.ld = c->ld; F.T = T;
    std::vector<double> host;
    auto sample = [&](double* gram, int64_t j0, int32_t nb) {
        A.gram = gram; A.j0 = j0; A.b = nb;
        hipLaunchKernelGGL(jwj::k_mtj_sample, dim3(1), dim3(256), 0, c->stream, A);
    };
    auto finish = [&](auto real) { hipLaunchKernelGGL((jwj::k_mtj_finish<decltype(real)>), dim3((unsigned)nsl), dim3(256), 0, c->stream, F); };
    if (int rc = block_walk(c, b, b.par, b.stat, (size_t)jwj::kStSize + (size_t)nsl * jwj::kRec, 1u, sample, finish, host, &S->step_ms)) return rc;
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
    return block_mul_alpha(c, c->mj, kMtj, trait, use_output_rows, out);
}

int jwas_hip_mtj_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::mj, kMtj.begin)) return rc;
    return session_drop(c, mtj_free);
}

}  // extern "C"
