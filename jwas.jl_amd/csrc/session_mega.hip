// session_mega.hip -- mega-trait models (mega.hpp), jwas_hip_mega_begin .. _end: megaBayesABC! / megaBayesC0!
// (markers/BayesianAlphabet/BayesABC.jl:1-58) for up to 64 traits and sampleMissingResiduals under a diagonal R (residual.jl:51-73).
// Several chains of one model are traits of the same session: jwas_hip_mega_sweep_r (the 4-class BayesR law, BayesR.jl:56-96),
// jwas_hip_mega_accumulate_r and jwas_hip_mega_psrf (the potential scale reduction factor over the chains).
#include "block_session.hpp"

static_assert(jwg::kMaxT == JWAS_HIP_MEGA_MAX_TRAITS && jwg::kMaxBlock == JWAS_HIP_MEGA_MAX_BLOCK, "the header's limits are mega.hpp's");

void mega_free(jwas_hip_ctx* c) { DevOwner::reset(c->mg); }

static const BlockWords kMega = {"mega-trait session", "mega-trait models", "mega-trait models do not run with residual weights", "jwas_hip_mega_begin", mega_free};

static int need_mega(jwas_hip_ctx* c) { return block_guard(c, &jwas_hip_ctx::mg, kMega); }
static int need_trait(jwas_hip_ctx* c, int32_t trait) { return block_trait_guard(c, &jwas_hip_ctx::mg, kMega, trait); }

static int64_t mega_bytes(int64_t n, int64_t p, int T, int bs)
{
    const int64_t ld = round_up(n, jwg::kRows), nsl = ld / jwg::kRows, nblocks = (p + bs - 1) / bs;
    return 8 * ((int64_t)T * ld + p + nblocks * bs * bs + 6 * (int64_t)T * p + nsl * T * bs + (int64_t)jwg::kParSize * T +
                (int64_t)T * (jwg::kStSize + 2 * nsl) + ld) + 4 * (int64_t)T * (ld / 32) + (int64_t)sizeof(jwg::Events);
}

// the per-trait parameters of a sweep or an imputation: checked, then par_host = vare | var_effect | log pi | log(1 - pi)
static int mega_params(jwas_hip_ctx* c, const jwas_mega_params* P, bool sweep, const char* who)
{
    auto& b = c->mg;
    NEED(c, P, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "%s: iteration must be >= 1", who);
    NEED(c, P->vare && (!sweep || (P->var_effect && P->pi)), JWAS_HIP_EINVAL, "%s: NULL parameter array", who);
    const int T = b.nt;
    b.par_host.assign((size_t)jwg::kParSize * T, 1.0);
    for (int k = 0; k < T; ++k) {
        NEED(c, std::isfinite(P->vare[k]) && P->vare[k] > 0.0, JWAS_HIP_EINVAL, "vare[%d] must be positive and finite (%g)", k, P->vare[k]);
        b.par_host[(size_t)jwg::kParVare * T + k] = P->vare[k];
        if (!sweep) continue;
        NEED(c, std::isfinite(P->var_effect[k]) && P->var_effect[k] > 0.0, JWAS_HIP_EINVAL, "var_effect[%d] must be positive and finite (%g)", k, P->var_effect[k]);
        NEED(c, P->pi[k] >= 0.0 && P->pi[k] <= 1.0, JWAS_HIP_EINVAL, "pi[%d] must be in [0,1] (%g)", k, P->pi[k]);
        b.par_host[(size_t)jwg::kParVar * T + k] = P->var_effect[k];
        b.par_host[(size_t)jwg::kParLogPi * T + k] = std::log(P->pi[k]);                    // pi = 0: -Inf, every marker is included
        b.par_host[(size_t)jwg::kParLogPiComp * T + k] = std::log(1.0 - P->pi[k]);
    }
    return JWAS_HIP_OK;
}

// One sweep over the blocks under the law of `sample` (jwg::k_mega_sample, _r) on block_session.hpp's walk.  host: the device record
// [T][rec] | [T][nslices][2]; resid_ss, resid_sum (NULL: not wanted): sum r^2 and sum r of every trait, the slices added in ascending order.
static int mega_run_sweep(jwas_hip_ctx* c, uint32_t iteration, uint64_t seed, double* par, double* stat, int rec, void (*sample)(const jwg::SampleArgs),
                          std::vector<double>& host, double* step_ms, double* resid_ss, double* resid_sum)
{
    auto& b = c->mg;
    const int T = b.nt, nsl = c->nslices;
    jwg::SampleArgs A = {};
    A.partials = b.partials; A.xpx = b.xpx; A.par = par; A.alpha = b.ms.alpha; A.beta = b.ms.beta; A.delta = b.ms.delta; A.ev = (jwg::Events*)b.ev;
    A.stat = stat; A.p = c->p; A.nslices = nsl; A.bs = b.bs; A.T = T; A.iter = iteration; A.first_trait = b.first_trait;
    split_seed(seed, A.seed_lo, A.seed_hi);
    jwg::FinishArgs F = {};
    F.X = genotypes_ptr(c); F.R = b.R; F.ev = (const jwg::Events*)b.ev; F.fin = stat + (size_t)T * rec; F.ld = c->ld; F.T = T;
    auto launch = [&](double* gram, int64_t j0, int32_t nb) {
        A.gram = gram; A.j0 = j0; A.b = nb;
        hipLaunchKernelGGL(sample, dim3((unsigned)T), dim3(256), 0, c->stream, A);
    };
    auto finish = [&](auto real) { hipLaunchKernelGGL((jwg::k_mega_finish<decltype(real)>), dim3((unsigned)nsl, (unsigned)T), dim3(256), 0, c->stream, F); };
    if (int rc = block_walk(c, b, par, stat, (size_t)T * (size_t)(rec + 2 * nsl), (unsigned)((T + jwg::kTT - 1) / jwg::kTT), launch, finish, host, step_ms)) return rc;
    for (int k = 0; k < T; ++k) {
        const double* fin = host.data() + (size_t)T * rec + (size_t)k * nsl * 2;
        double ss = 0.0, sm = 0.0;
        for (int sl = 0; sl < nsl; ++sl) { ss += fin[2 * sl]; sm += fin[2 * sl + 1]; }       // slices in order
        if (resid_ss) resid_ss[k] = ss;
        if (resid_sum) resid_sum[k] = sm;
    }
    return JWAS_HIP_OK;
}

extern "C" {

int jwas_hip_mega_begin(jwas_hip_ctx* c, int32_t T, int32_t block_size, int32_t first_trait)
{
    if (int rc = block_begin_guard(c, kMega, T, 1, jwg::kMaxT, block_size)) return rc;
    NEED(c, first_trait >= 0 && (int64_t)first_trait + T <= (int64_t)jwg::kMaxTraitId, JWAS_HIP_EINVAL,
         "first_trait must be >= 0 and first_trait + T <= %u (got %d)", jwg::kMaxTraitId, first_trait);
    auto& b = c->mg;
    return block_begin(c, b, kMega, T, block_size, (size_t)jwg::kParSize * T, (size_t)T * (size_t)(jwg::kStSize + 2 * c->nslices), [&](auto alloc) {
        b.first_trait = (uint32_t)first_trait; b.mask_words = c->ld / 32;
        const size_t maskb = sizeof(uint32_t) * (size_t)T * (size_t)b.mask_words;
        if (int rc = alloc(&b.mask, maskb)) return rc;
        HIPCHK(c, hipMemsetAsync(b.mask, 0, maskb, c->stream));
        return (int)JWAS_HIP_OK;
    });
}

int jwas_hip_mega_set_missing(jwas_hip_ctx* c, int64_t nvalues, const uint8_t* missing)
{
    if (int rc = need_mega(c)) return rc;
    auto& b = c->mg;
    const int64_t n = c->n;
    std::vector<uint32_t> words((size_t)b.nt * (size_t)b.mask_words, 0u);
    if (missing) {
        NEED(c, nvalues == (int64_t)b.nt * n, JWAS_HIP_EINVAL, "nvalues (%lld) differs from T n (%lld)", (long long)nvalues, (long long)((int64_t)b.nt * n));
        for (int k = 0; k < b.nt; ++k)
            for (int64_t i = 0; i < n; ++i)
                if (missing[(size_t)k * n + i]) words[(size_t)k * b.mask_words + (size_t)(i >> 5)] |= 1u << (i & 31);
        b.miss_host.assign(missing, missing + (size_t)b.nt * n);
    } else {
        b.miss_host.clear();
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b.mask, words.data(), sizeof(uint32_t) * words.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_mega_set_residual(jwas_hip_ctx* c, int32_t trait, const double* r)
{
    if (int rc = need_trait(c, trait)) return rc;
    return block_set_residual(c, c->mg, trait, r);
}

int jwas_hip_mega_get_residual(jwas_hip_ctx* c, int32_t trait, double* out)
{
    if (int rc = need_trait(c, trait)) return rc;
    return block_get_residual(c, c->mg, trait, out);
}

int jwas_hip_mega_set_state(jwas_hip_ctx* c, int32_t trait, const double* alpha, const double* beta, const double* delta)
{
    if (int rc = need_trait(c, trait)) return rc;
    return marker_state_set(c, c->mg.ms, trait, 1, alpha, beta, delta);
}

int jwas_hip_mega_get_state(jwas_hip_ctx* c, int32_t trait, double* alpha, double* beta, double* delta)
{
    if (int rc = need_trait(c, trait)) return rc;
    return marker_state_get(c, c->mg.ms, trait, 1, alpha, beta, delta);
}

int jwas_hip_mega_impute(jwas_hip_ctx* c, const jwas_mega_params* P)
{
    if (int rc = need_mega(c)) return rc;
    if (int rc = mega_params(c, P, false, "jwas_hip_mega_impute")) return rc;
    auto& b = c->mg;
    if (int rc = block_upload_params(c, b, b.par)) return rc;
    if (!b.miss_host.empty()) {
        uint32_t lo, hi;
        split_seed(P->seed, lo, hi);
        hipLaunchKernelGGL(jwg::k_mega_impute, dim3((unsigned)((c->n + 255) / 256), (unsigned)b.nt), dim3(256), 0, c->stream, (const uint32_t*)b.mask, b.mask_words,
                           c->n, c->ld, (const double*)b.par, P->iteration, lo, hi, b.first_trait, b.R);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// the per-chain parameters of a BayesR sweep: checked, then par_host = vare | sigma2 | gamma[4] | log pi[4]
static int mega_params_r(jwas_hip_ctx* c, const jwas_mega_r_params* P)
{
    auto& b = c->mg;
    NEED(c, P, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_mega_sweep_r: iteration must be >= 1");
    NEED(c, P->vare && P->var_effect && P->gamma && P->pi, JWAS_HIP_EINVAL, "jwas_hip_mega_sweep_r: NULL parameter array");
    const int T = b.nt;
    b.par_host.assign((size_t)jwg::kParRSize * T, 1.0);
    for (int k = 0; k < T; ++k) {
        NEED(c, std::isfinite(P->vare[k]) && P->vare[k] > 0.0, JWAS_HIP_EINVAL, "vare[%d] must be positive and finite (%g)", k, P->vare[k]);
        NEED(c, std::isfinite(P->var_effect[k]) && P->var_effect[k] > 0.0, JWAS_HIP_EINVAL, "var_effect[%d] must be positive and finite (%g)", k, P->var_effect[k]);
        b.par_host[(size_t)jwg::kParRVare * T + k] = P->vare[k];
        b.par_host[(size_t)jwg::kParRVar * T + k] = P->var_effect[k];
        double sum = 0.0;
        for (int q = 0; q < jwg::kClasses; ++q) {
            const double g = P->gamma[(size_t)q * T + k], pq = P->pi[(size_t)q * T + k];
            if (q == 0) NEED(c, g == 0.0, JWAS_HIP_EINVAL, "gamma[0][%d] must be 0: class 1 is the null class (%g)", k, g);
            else NEED(c, std::isfinite(g) && g > 0.0, JWAS_HIP_EINVAL, "gamma[%d][%d] must be positive and finite (%g)", q, k, g);
            NEED(c, pq >= 0.0 && pq <= 1.0, JWAS_HIP_EINVAL, "pi[%d][%d] must be in [0,1] (%g)", q, k, pq);
            sum += pq;
            b.par_host[(size_t)(jwg::kParRGamma + q) * T + k] = g;
            b.par_host[(size_t)(jwg::kParRLogPi + q) * T + k] = std::log(pq);              // pi = 0: -Inf, the class is never drawn
        }
        NEED(c, std::fabs(sum - 1.0) <= 1e-8, JWAS_HIP_EINVAL, "the class probabilities of chain %d sum to %.17g, not 1", k, sum);
    }
    return JWAS_HIP_OK;
}

int jwas_hip_mega_sweep(jwas_hip_ctx* c, const jwas_mega_params* P, jwas_mega_stats* S)
{
    if (int rc = need_mega(c)) return rc;
    NEED(c, S, JWAS_HIP_EINVAL, "NULL argument");
    if (int rc = mega_params(c, P, true, "jwas_hip_mega_sweep")) return rc;
    auto& b = c->mg;
    std::vector<double> host;
    if (int rc = mega_run_sweep(c, P->iteration, P->seed, b.par, b.stat, jwg::kStSize, jwg::k_mega_sample, host, &S->step_ms, S->resid_ss, S->resid_sum)) return rc;
    for (int k = 0; k < b.nt; ++k) {
        const double* st = host.data() + (size_t)k * jwg::kStSize;
        if (S->sum_delta) S->sum_delta[k] = st[jwg::kStDelta];
        if (S->beta_ss) S->beta_ss[k] = st[jwg::kStBeta];
        if (S->alpha_ss) S->alpha_ss[k] = st[jwg::kStAlpha];
        if (S->n_changed) S->n_changed[k] = st[jwg::kStChanged];
    }
    return JWAS_HIP_OK;
}

int jwas_hip_mega_accumulate(jwas_hip_ctx* c, double nsamples)
{
    if (int rc = need_mega(c)) return rc;
    return marker_state_accumulate<false>(c, c->mg.ms, c->mg.nt, nsamples);
}

int jwas_hip_mega_sweep_r(jwas_hip_ctx* c, const jwas_mega_r_params* P, jwas_mega_r_stats* S)
{
    if (int rc = need_mega(c)) return rc;
    NEED(c, S, JWAS_HIP_EINVAL, "NULL argument");
    if (int rc = mega_params_r(c, P)) return rc;
    auto& b = c->mg;
    const int T = b.nt;
    HIPCHK(c, hipSetDevice(c->device));
    if (!b.par_r) {
        if (int rc = alloc_or_nomem(c, b.mem, &b.par_r, sizeof(double) * (size_t)jwg::kParRSize * T, "mega-trait session", mega_free)) return rc;
        if (int rc = alloc_or_nomem(c, b.mem, &b.stat_r, sizeof(double) * (size_t)T * (size_t)(jwg::kStRSize + 2 * c->nslices), "mega-trait session", mega_free))
            return rc;
    }
    std::vector<double> host;
    if (int rc = mega_run_sweep(c, P->iteration, P->seed, b.par_r, b.stat_r, jwg::kStRSize, jwg::k_mega_sample_r, host, &S->step_ms, S->resid_ss, S->resid_sum))
        return rc;
    for (int k = 0; k < T; ++k) {
        const double* st = host.data() + (size_t)k * jwg::kStRSize;
        if (S->class_counts)
            for (int q = 0; q < jwg::kClasses; ++q) S->class_counts[(size_t)q * T + k] = st[jwg::kStRCount + q];
        if (S->ssq) S->ssq[k] = st[jwg::kStRSsq];
        if (S->nnz) S->nnz[k] = st[jwg::kStRNnz];
        if (S->alpha_ss) S->alpha_ss[k] = st[jwg::kStRAlpha];
        if (S->n_changed) S->n_changed[k] = st[jwg::kStRChanged];
    }
    return JWAS_HIP_OK;
}

int jwas_hip_mega_accumulate_r(jwas_hip_ctx* c, double nsamples)
{
    if (int rc = need_mega(c)) return rc;
    return marker_state_accumulate<true>(c, c->mg.ms, c->mg.nt, nsamples);
}

int jwas_hip_mega_psrf(jwas_hip_ctx* c, double nsamples, double* out)
{
    if (int rc = need_mega(c)) return rc;
    auto& b = c->mg;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, b.nt >= 2, JWAS_HIP_EINVAL, "the potential scale reduction factor needs at least 2 chains (the session has %d)", b.nt);
    NEED(c, std::isfinite(nsamples) && nsamples >= 2.0, JWAS_HIP_EINVAL, "nsamples must be >= 2 (got %g)", nsamples);
    HIPCHK(c, hipSetDevice(c->device));
    if (!b.psrf)
        if (int rc = alloc_or_nomem(c, b.mem, &b.psrf, sizeof(double) * (size_t)c->p, "mega-trait session", mega_free)) return rc;
    const unsigned blocks = (unsigned)std::min<int64_t>(jwg::kPsrfBlocks, (c->p + 255) / 256);
    hipLaunchKernelGGL(jwg::k_mega_psrf, dim3(blocks), dim3(256), 0, c->stream, (const double*)b.ms.mean_a, (const double*)b.ms.mean_a2, c->p, (int32_t)b.nt, nsamples,
                       b.psrf);
    HIPCHK(c, hipGetLastError());
    return to_host(c, out, b.psrf, sizeof(double) * (size_t)c->p);
}

int jwas_hip_mega_get_posterior(jwas_hip_ctx* c, int32_t trait, double* mean, double* mean2, double* freq)
{
    if (int rc = need_trait(c, trait)) return rc;
    return marker_state_posterior(c, c->mg.ms, trait, mean, mean2, freq);
}

int jwas_hip_mega_mul_alpha(jwas_hip_ctx* c, int32_t trait, int32_t use_output_rows, double* out)
{
    if (int rc = need_trait(c, trait)) return rc;
    return block_mul_alpha(c, c->mg, kMega, trait, use_output_rows, out);
}

int jwas_hip_mega_get_gram(jwas_hip_ctx* c, int64_t block, int64_t nvalues, double* out, double* out_xpx)
{
    if (int rc = need_mega(c)) return rc;
    return block_get_gram(c, c->mg, block, nvalues, out, out_xpx);
}

int64_t jwas_hip_mega_estimate_bytes(int64_t n, int64_t p, int32_t T, int32_t block_size)
{
    // the residuals, x'x, the Grams (8 p b for whole blocks), the state and its running means, the slice partials, the per-trait
    // parameters and statistics, a row vector, the missing-cell bit mask and the change lists
    return mega_bytes(std::max<int64_t>(n, 1), std::max<int64_t>(p, 1), std::min(std::max(T, 1), jwg::kMaxT),
                      block_size > 0 ? std::min(block_size, jwg::kMaxBlock) : 64);
}

int jwas_hip_mega_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::mg, kMega.begin)) return rc;
    return session_drop(c, mega_free);
}

}  // extern "C"
