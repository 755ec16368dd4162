// block_session.hpp -- the host side that the mega-trait session (session_mega.hip) and the joint multi-trait session
// (session_mtjoint.hip) share: both hold a BlockSession (ctx.hpp) -- residuals, x'x, the block Grams, a MarkerState, the slice partials
// and a change list -- and walk the blocks with mega.hpp's k_mega_update_partial.  One body for the guards, _begin, the residual, Gram
// and X alpha transfers and the block walk of a sweep; a session adds its parameters, its sampler and its finish kernel.
// Host-only: no kernel is defined here.
#pragma once
#include "ctx.hpp"
#include "marker_state.hpp"
#include "mega.hpp"

// a session's words in the messages, the entry point that opens it and its free function
struct BlockWords {
    const char* session;                                    // "mega-trait session": the name in allocation failures
    const char* models;                                     // "mega-trait models": what needs dense genotypes and refuses shards
    const char* weighted;                                   // the refusal of residual weights
    const char* begin;                                      // "jwas_hip_mega_begin"
    void (*free_session)(jwas_hip_ctx*);
};

// what every entry point of an open session checks first
template <class S>
static int block_guard(jwas_hip_ctx* c, S jwas_hip_ctx::*session, const BlockWords& w)
{
    if (int rc = session_guard(c, session, w.begin)) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "%s", w.weighted);
    return refuse_shards(c, w.models);
}

template <class S>
static int block_trait_guard(jwas_hip_ctx* c, S jwas_hip_ctx::*session, const BlockWords& w, int32_t trait)
{
    if (int rc = block_guard(c, session, w)) return rc;
    NEED(c, trait >= 0 && trait < (c->*session).nt, JWAS_HIP_EINVAL, "trait %d outside [0,%d)", trait, (c->*session).nt);
    return JWAS_HIP_OK;
}

// what a _begin checks before it drops the earlier session
static inline int block_begin_guard(jwas_hip_ctx* c, const BlockWords& w, int32_t T, int min_t, int max_t, int32_t block_size)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, !c->packed, JWAS_HIP_EUNSUP, "%s need dense genotypes (2-bit packed storage is not supported)", w.models);
    NEED(c, genotypes_ptr(c) && c->n > 0 && c->p > 0, JWAS_HIP_ESTATE, "no genotype matrix loaded");
    if (int rc = refuse_shards(c, w.models)) return rc;
    NEED(c, !is_weighted(c), JWAS_HIP_EUNSUP, "%s", w.weighted);
    NEED(c, T >= min_t && T <= max_t, JWAS_HIP_EINVAL, "the number of traits must be in [%d,%d] (got %d)", min_t, max_t, T);
    NEED(c, block_size >= 0 && block_size <= jwg::kMaxBlock, JWAS_HIP_EINVAL, "block size must be in [1,%d] (0: 64), got %d", jwg::kMaxBlock, block_size);
    return JWAS_HIP_OK;
}

// The earlier session dropped, the shared buffers allocated (par, stat: their doubles) and zeroed, x'x and the block Grams formed.
// own(alloc): the session's own members and buffers, before the shared ones.
template <class Own>
static int block_begin(jwas_hip_ctx* c, BlockSession& b, const BlockWords& w, int32_t T, int32_t block_size, size_t par_doubles, size_t stat_doubles, Own&& own)
{
    if (int rc = session_drop(c, w.free_session)) return rc;
    const int bs = block_size ? block_size : 64;
    const int64_t p = c->p, ld = c->ld;
    b.nt = T; b.bs = bs; b.nblocks = (p + bs - 1) / bs; b.row_cap = ld;
    auto alloc = [&](auto** ptr, size_t bytes) { return alloc_or_nomem(c, b.mem, ptr, bytes, w.session, w.free_session); };
    const size_t gramb = sizeof(double) * (size_t)b.nblocks * bs * bs;
    jwg::Events* ev = nullptr;
    if (int rc = own(alloc)) return rc;
    if (int rc = alloc(&b.R, sizeof(double) * (size_t)T * ld)) return rc;
    if (int rc = alloc(&b.xpx, sizeof(double) * (size_t)p)) return rc;
    if (int rc = alloc(&b.gram, gramb)) return rc;
    if (int rc = marker_state_begin(c, b.ms, b.mem, T, w.session, w.free_session)) return rc;
    if (int rc = alloc(&b.partials, sizeof(double) * (size_t)c->nslices * T * bs)) return rc;
    if (int rc = alloc(&b.par, sizeof(double) * par_doubles)) return rc;
    if (int rc = alloc(&b.stat, sizeof(double) * stat_doubles)) return rc;
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

// (the callers have passed block_trait_guard)
static inline int block_set_residual(jwas_hip_ctx* c, BlockSession& b, int32_t trait, const double* r)
{
    NEED(c, r, JWAS_HIP_EINVAL, "NULL argument");
    for (int64_t i = 0; i < c->n; ++i) NEED(c, std::isfinite(r[i]), JWAS_HIP_EINVAL, "the residual of record %lld is not finite (%g)", (long long)i, r[i]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b.R + (size_t)trait * c->ld, r, sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

static inline int block_get_residual(jwas_hip_ctx* c, BlockSession& b, int32_t trait, double* out)
{
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, out, b.R + (size_t)trait * c->ld, sizeof(double) * (size_t)c->n);
}

// the Gram of one block (b x b of its bs x bs) and, if wanted, its x'x
static inline int block_get_gram(jwas_hip_ctx* c, BlockSession& b, int64_t block, int64_t nvalues, double* out, double* out_xpx)
{
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

// X alpha_trait over the training rows or the output rows
static inline int block_mul_alpha(jwas_hip_ctx* c, BlockSession& b, const BlockWords& w, int32_t trait, int32_t use_output_rows, double* out)
{
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
        if (int rc = alloc_or_nomem(c, b.mem, &b.row, sizeof(double) * (size_t)ld, w.session, w.free_session)) return rc;
        b.row_cap = ld;
    }
    return marker_state_mul_alpha(c, b.ms, trait, X, ld, n, b.row, out);
}

// par_host -> the device table `par` (par_host stays until the sweep has finished)
static inline int block_upload_params(jwas_hip_ctx* c, BlockSession& b, double* par)
{
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(par, b.par_host.data(), sizeof(double) * b.par_host.size(), hipMemcpyHostToDevice, c->stream));
    return JWAS_HIP_OK;
}

// One sweep over the blocks: par_host goes to `par`, the nstat doubles of `stat` are zeroed; per block the right-hand sides
// (k_mega_update_partial on a grid of nslices x tiles_y) and sample(gram, j0, b): the launch of the sampler on the block's Gram, first
// marker and width; after the last block finish(real): the launch of the kernel that applies its change list and sums the residuals
// (real: a value of the context's element type).  host: `stat` as the device left it; step_ms: the device time of the launches.
template <class Sample, class Finish>
static int block_walk(jwas_hip_ctx* c, BlockSession& b, double* par, double* stat, size_t nstat, unsigned tiles_y, Sample&& sample, Finish&& finish,
                      std::vector<double>& host, double* step_ms)
{
    if (int rc = block_upload_params(c, b, par)) return rc;
    if (int rc = step_timer_begin(c)) return rc;
    HIPCHK(c, hipMemsetAsync(stat, 0, sizeof(double) * nstat, c->stream));
    jwg::UpdateArgs U = {};
    U.X = genotypes_ptr(c); U.R = b.R; U.partials = b.partials; U.ld = c->ld; U.T = b.nt; U.bs = b.bs;
    with_real(c, [&](auto real) {
        using real_t = decltype(real);
        for (int64_t k = 0; k < b.nblocks; ++k) {
            const int64_t j0 = k * b.bs;
            U.ev = k ? (const jwg::Events*)b.ev : nullptr; U.j0 = j0; U.b = (int32_t)std::min<int64_t>(b.bs, c->p - j0);
            hipLaunchKernelGGL((jwg::k_mega_update_partial<real_t>), dim3((unsigned)c->nslices, tiles_y), dim3(256), 0, c->stream, U);
            sample(b.gram + k * (int64_t)b.bs * b.bs, j0, U.b);
        }
        finish(real);
    });
    HIPCHK(c, hipGetLastError());
    host.resize(nstat);
    return step_timer_end(c, host.data(), stat, sizeof(double) * nstat, step_ms);
}
