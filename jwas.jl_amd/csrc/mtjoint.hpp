// mtjoint.hpp -- unconstrained multi-trait BayesC with 5 to 8 traits on the device: Gibbs sampler I (_MTBayesABC_samplerI!,
// markers/BayesianAlphabet/MTBayesABC.jl:57-127) with a full t x t marker-effect covariance G (common to all markers), a full residual
// covariance R and Pi over the 2^t joint inclusion states, on the block form of the mega-trait session (mega.hpp: its Grams, its
// pass over the genotypes k_mega_update_partial and its change lists are used as they are).
//
// THE LAW (MTBayesABC.jl:75-126).  Rinv = inv(vare), Ginv = inv(G), both t x t, and log pi[2^t] (-Inf: the state has probability 0)
// come from the host once per sweep.  Marker j, with s_k = x_j'r_k at the marker's entry, xx = x_j'x_j and the marker's current
// (alpha, beta, delta):   w_k = s_k + xx alpha_k(old)   for every k (NOT refreshed inside the loop below), then for k = 0 .. t-1 in order,
// with beta and delta of the other traits as they stand (those of l < k are this marker's new ones):
//   Ginv11 = Ginv[k][k],  C11 = Ginv11 + Rinv[k][k] xx,  invLhs0 = 1 / Ginv11,  invLhs1 = 1 / C11
//   q0  = sum_{l != k} Ginv[k][l] beta_l                                       gHat0 = (-q0) invLhs0
//   wr  = sum_l w_l Rinv[l][k]
//   q1  = sum_{l != k} (delta_l ? Ginv[k][l] + xx Rinv[k][l] : Ginv[k][l]) beta_l      gHat1 = (wr - q1) invLhs1      (every sum: l ascending)
//   logDelta0 = -0.5 (log Ginv11 - gHat0^2 Ginv11) + log pi[d0],  logDelta1 = -0.5 (log C11 - gHat1^2 C11) + log pi[d1]
//          d0 / d1: the marker's joint state (bit l: delta_l) with bit k cleared / set
//   probDelta1 = 1 / (1 + exp(logDelta0 - logDelta1));   log pi[d1] = -Inf: probDelta1 = 0 (no NaN when both are -Inf); log pi[d0] = -Inf:
//          exp(-Inf) = 0, probDelta1 = 1.  A state of probability 0 is never entered from a state of positive probability.
//   u_k < probDelta1:  delta_k = 1, beta_k = alpha_k = gHat1 + z_k sqrt(invLhs1);   else  delta_k = 0, alpha_k = 0, beta_k = gHat0 + z_k sqrt(invLhs0)
//          (beta of an excluded trait is a real draw and enters the right-hand sides of the later traits)
// After the marker  r_k += x_j (alpha_k,old - alpha_k,new)  for every k.
//
// EXACT BLOCK FORM (mega.hpp): s[k][i] = x_i'r_k for the markers i of a block from the residuals at block entry; when marker j moves by
// d_k = alpha_old - alpha_new in trait k, s[k][i] += G_ij d_k for every i of the block; the residuals follow at the next block's entry
// (k_mega_update_partial applies the per-trait change lists) or in k_mtj_finish.  Per block two stream-ordered launches:
//   k_mega_update_partial  grid (row slices, 1): t <= kTT = 8, one trait tile holds all traits
//   k_mtj_sample           ONE workgroup: all threads add the slice partials (ascending) into s[t][b] in LDS; wave 0 walks the block 64
//                          markers at a time by speculative evaluation: every pending lane evaluates its marker's WHOLE t-step chain from
//                          the current s[:, marker] and its own (alpha, beta, delta) against the fixed draws; the first lane in which
//                          any alpha_k moved commits, its Gram row corrects s[k][.] of every trait that moved; the lanes before it are
//                          final with what they just evaluated (beta and delta of excluded traits included).  Rinv, Ginv, the
//                          constants of Ginv11 and log pi are in LDS (uniform reads).  Then all threads form the block's statistics.
//   k_mtj_finish           grid (row slices): the last change lists, then the slice's t (t + 1) / 2 residual cross-products and t sums.
// ORDER OF EVERY SUM (no floating-point atomics; the same seed gives the same bits).  Slice partials and s: mega.hpp's.  The
// statistics of a block (sum beta beta' by pairs k <= l, written to both (k, l) and (l, k): symmetric bit for bit; sum alpha^2 per
// trait): thread i holds marker i of the block, a shuffle tree (32 .. 1) per wave, the four waves in order, the blocks in stream
// order.  The joint-state counts and the changed count are integers (LDS integer atomics are exact).  Residual cross-products: per
// slice one row per thread, the same tree; the host adds the slices ascending.
// DRAWS: philox4x32_10(marker, iteration, 0x05000000 | trait, slot): slot 14 the decision uniform (u52 of words (1, 0)), slot 15 the
// normal (Box-Muller, jwu::normal_from).  They do not depend on the block size.
#pragma once
#define JWG_BLOCK_FORM_ONLY
#include "mega.hpp"

namespace jwj {

constexpr int kMinT = 5, kMaxT = 8, kMaxStates = 1 << kMaxT;
constexpr int kPairs = kMaxT * (kMaxT + 1) / 2;             // 36 pairs k <= l
constexpr int kRec = kPairs + kMaxT;                        // what a block (its statistics) and a slice (its residual sums) reduce
constexpr uint32_t kTag = 0x05000000u, kSlotU = 14u, kSlotZ = 15u;
// the parameters of a sweep (matrices with row stride kMaxT, unused entries 0; log pi beyond 2^t: -Inf)
constexpr int kParRinv = 0, kParGinv = kMaxT * kMaxT, kParLogPi = 2 * kMaxT * kMaxT, kParSize = kParLogPi + kMaxStates;
// the device record of a sweep's statistics; behind it [nslices][kRec] residual cross-products (pairs k <= l) | sums
constexpr int kStCounts = 0, kStBB = kMaxStates, kStAA = kStBB + kMaxT * kMaxT, kStChanged = kStAA + kMaxT, kStSize = kStChanged + 8;
static_assert(kMaxT == jwg::kTT, "one trait tile of k_mega_update_partial holds all traits");

struct SampleArgs {
    const double* partials;             // [nslices][T][bs]
    const double* gram;                 // this block's [bs][bs]
    const double* xpx;                  // [p]
    const double* par;                  // [kParSize]
    double *alpha, *beta, *delta;       // [T][p]
    jwg::Events* ev;                    // out
    double* stat;                       // [kStSize], accumulated over the blocks of a sweep
    int64_t j0, p;
    int32_t nslices, b, bs, T;
    uint32_t iter, seed_lo, seed_hi;
};

// the pairs k <= l of v v' (row by row) and, behind them, f(v_k): what a block or a slice reduces
template <class F>
__device__ __forceinline__ void pairs_of(const double (&v)[kMaxT], double (&acc)[kRec], F&& f)
{
    int q = 0;
#pragma unroll
    for (int k = 0; k < kMaxT; ++k)
#pragma unroll
        for (int l = k; l < kMaxT; ++l) acc[q++] = v[k] * v[l];
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) acc[kPairs + k] = f(k, v[k]);
}

// grid = 1 workgroup of 256 threads
__global__ __launch_bounds__(256) void k_mtj_sample(const SampleArgs A)
{
    __shared__ double s_s[kMaxT][jwg::kMaxBlock];           // x_i'r_k, corrected by every commit
    __shared__ double s_a0[kMaxT][jwg::kMaxBlock];          // alpha at block entry; after a sub-block is final: its beta
    __shared__ double c_R[kMaxT * kMaxT], c_G[kMaxT * kMaxT], c_lp[kMaxStates];
    __shared__ double c_lg[kMaxT], c_ig[kMaxT], c_sg[kMaxT];            // log Ginv11, 1 / Ginv11, sqrt(1 / Ginv11)
    __shared__ int s_dm[jwg::kMaxBlock], s_hist[kMaxStates];
    __shared__ double sh[4 * kRec], outv[kRec];
    const int tid = threadIdx.x, lane = tid & 63;
    const int T = A.T, b = A.b, bs = A.bs;
    const int64_t p = A.p;
    for (int i = tid; i < b; i += 256) {
        const int64_t stride = (int64_t)T * bs;
        for (int k = 0; k < T; ++k) {
            const double* __restrict__ part = A.partials + (int64_t)k * bs + i;
            double s = 0.0;
#pragma unroll 8
            for (int sl = 0; sl < A.nslices; ++sl) s = s + part[sl * stride];      // (ascending)
            s_s[k][i] = s;
            s_a0[k][i] = A.alpha[(int64_t)k * p + A.j0 + i];
        }
    }
    if (tid < kMaxT * kMaxT) { c_R[tid] = A.par[kParRinv + tid]; c_G[tid] = A.par[kParGinv + tid]; }
    c_lp[tid] = A.par[kParLogPi + tid];
    s_hist[tid] = 0;
    s_dm[tid] = 0;
    if (tid < T) {
        const double g11 = A.par[kParGinv + tid * kMaxT + tid], inv = 1.0 / g11;
        c_lg[tid] = log(g11); c_ig[tid] = inv; c_sg[tid] = sqrt(inv);
    }
    __syncthreads();
    int nchanged = 0;
    if (tid < 64) {
        int base[kMaxT];
#pragma unroll
        for (int k = 0; k < kMaxT; ++k) base[k] = 0;
        const int nsub = (b + 63) / 64;
#pragma unroll 1
        for (int s = 0; s < nsub; ++s) {
            const int kq = 64 * s + lane;
            const bool valid = kq < b;
            const int kl = valid ? kq : 0;
            const int64_t j = A.j0 + kl;
            const double xx = A.xpx[j];
            double u[kMaxT], z[kMaxT], a_cur[kMaxT], b_cur[kMaxT], invC[kMaxT], logC[kMaxT], sdC[kMaxT];
            int dm = 0;
#pragma unroll
            for (int k = 0; k < kMaxT; ++k) {
                u[k] = 1.0; z[k] = 0.0; a_cur[k] = 0.0; b_cur[k] = 0.0; invC[k] = 1.0; logC[k] = 0.0; sdC[k] = 1.0;
                if (k < T) {
                    const uint32_t tag = kTag | (uint32_t)k;
                    z[k] = jwu::normal_from(jw::philox4x32_10((uint32_t)j, A.iter, tag, kSlotZ, A.seed_lo, A.seed_hi));
                    const jw::u32x4 wu = jw::philox4x32_10((uint32_t)j, A.iter, tag, kSlotU, A.seed_lo, A.seed_hi);
                    u[k] = jw::u52(wu.x, wu.y);
                    a_cur[k] = s_a0[k][kl];
                    b_cur[k] = A.beta[(int64_t)k * p + j];
                    if (A.delta[(int64_t)k * p + j] != 0.0) dm |= 1 << k;
                    const double C11 = c_G[k * kMaxT + k] + c_R[k * kMaxT + k] * xx;
                    invC[k] = 1.0 / C11; logC[k] = log(C11); sdC[k] = sqrt(invC[k]);
                }
            }
            unsigned long long pending = __ballot(valid);
            while (pending) {
                // the marker's whole chain from the current s and the lane's own state
                double an[kMaxT], bn[kMaxT], w[kMaxT];
                int dn = dm;
#pragma unroll
                for (int k = 0; k < kMaxT; ++k) { an[k] = 0.0; bn[k] = b_cur[k]; w[k] = k < T ? s_s[k][kl] + xx * a_cur[k] : 0.0; }
#pragma unroll
                for (int k = 0; k < kMaxT; ++k) {
                    if (k < T) {
                        const double G11 = c_G[k * kMaxT + k];
                        const double C11 = G11 + c_R[k * kMaxT + k] * xx;
                        double q0 = 0.0, q1 = 0.0, wr = 0.0;
#pragma unroll
                        for (int l = 0; l < kMaxT; ++l) {
                            if (l < T) {
                                wr = wr + w[l] * c_R[l * kMaxT + k];
                                if (l != k) {
                                    const double g = c_G[k * kMaxT + l];
                                    q0 = q0 + g * bn[l];
                                    q1 = q1 + (((dn >> l) & 1) ? g + xx * c_R[k * kMaxT + l] : g) * bn[l];
                                }
                            }
                        }
                        const double gHat0 = (-q0) * c_ig[k];
                        const double gHat1 = (wr - q1) * invC[k];
                        const int d0 = dn & ~(1 << k), d1 = dn | (1 << k);
                        const double lp1 = c_lp[d1];
                        const double ld0 = -0.5 * (c_lg[k] - gHat0 * gHat0 * G11) + c_lp[d0];
                        const double ld1 = -0.5 * (logC[k] - gHat1 * gHat1 * C11) + lp1;
                        const double prob = lp1 == -__builtin_inf() ? 0.0 : 1.0 / (1.0 + exp(ld0 - ld1));
                        const bool inc = u[k] < prob;
                        bn[k] = inc ? gHat1 + z[k] * sdC[k] : gHat0 + z[k] * c_sg[k];
                        an[k] = inc ? bn[k] : 0.0;
                        dn = inc ? d1 : d0;
                    }
                }
                bool moved = false;
#pragma unroll
                for (int k = 0; k < kMaxT; ++k) moved = moved || (an[k] != a_cur[k]);
                const int kw = jwu::first_changed(moved && valid, pending);
                // lanes up to the winner are final with what they just evaluated
                const unsigned long long done = jwu::final_lanes(pending, kw);
                if ((done >> lane) & 1ull) {
                    dm = dn;
#pragma unroll
                    for (int k = 0; k < kMaxT; ++k) b_cur[k] = bn[k];
                }
                if (kw >= 64) break;
                // the winner commits; its Gram row corrects s of every trait that moved: s[k][i] += G_i,ce d_k
                const int ce = 64 * s + kw;
                const double* __restrict__ grow = A.gram + (int64_t)ce * bs;
                __builtin_amdgcn_wave_barrier();            // (one wave: its LDS accesses execute in program order)
#pragma unroll
                for (int k = 0; k < kMaxT; ++k) {
                    const double D = __shfl(a_cur[k] - an[k], kw, 64);
                    if (k < T && D != 0.0)
                        for (int k2 = lane; k2 < b; k2 += 64) s_s[k][k2] = s_s[k][k2] + grow[k2] * D;
                    if (lane == kw) a_cur[k] = an[k];
                }
                __builtin_amdgcn_wave_barrier();
                pending &= ~done;
            }
            // the sub-block is final: change lists, state, what the statistics read
            bool any = false;
#pragma unroll
            for (int k = 0; k < kMaxT; ++k) {
                if (k < T) {
                    const double a0 = s_a0[k][kl];
                    const bool changed = valid && (a_cur[k] != a0);
                    any = any || changed;
                    const int e = jwu::list_entry(changed, lane, base[k]);
                    if (changed) {
                        A.ev->idx[k][e] = (int32_t)j;
                        A.ev->d[k][e] = a0 - a_cur[k];
                    }
                    if (valid) {
                        A.alpha[(int64_t)k * p + j] = a_cur[k];
                        A.beta[(int64_t)k * p + j] = b_cur[k];
                        A.delta[(int64_t)k * p + j] = (double)((dm >> k) & 1);
                    }
                }
            }
            nchanged += __popcll(__ballot(any));
            __builtin_amdgcn_wave_barrier();
            if (valid) {
#pragma unroll
                for (int k = 0; k < kMaxT; ++k)
                    if (k < T) s_a0[k][kl] = b_cur[k];
                s_dm[kl] = dm;
                atomicAdd(&s_hist[dm], 1);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kMaxT; ++k)
                if (k < T) A.ev->count[k] = base[k];
        }
    }
    __syncthreads();
    // the block's statistics join the sweep's (the blocks of a sweep run in stream order)
    double bv[kMaxT], acc[kRec];
    const int dmf = s_dm[tid];
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) bv[k] = (tid < b && k < T) ? s_a0[k][tid] : 0.0;
    pairs_of(bv, acc, [&](int k, double v) { return ((dmf >> k) & 1) ? v * v : 0.0; });
    jwu::block_reduce<kRec>(acc, sh, outv);
    __syncthreads();
    if (tid < kPairs) {
        int k = 0, q = tid;
        while (q >= kMaxT - k) { q -= kMaxT - k; ++k; }
        const int l = k + q;
        const double v = A.stat[kStBB + k * kMaxT + l] + outv[tid];
        A.stat[kStBB + k * kMaxT + l] = v;
        A.stat[kStBB + l * kMaxT + k] = v;
    } else if (tid < kRec) {
        A.stat[kStAA + tid - kPairs] = A.stat[kStAA + tid - kPairs] + outv[tid];
    }
    A.stat[kStCounts + tid] = A.stat[kStCounts + tid] + (double)s_hist[tid];
    if (tid == 0) A.stat[kStChanged] = A.stat[kStChanged] + (double)nchanged;
}

struct FinishArgs {
    const void* X;
    double* R;                          // [T][ld]
    const jwg::Events* ev;
    double* fin;                        // [nslices][kRec]: the pairs k <= l of sum r_k r_l, then sum r_k
    int64_t ld;
    int32_t T;
};

// grid = nslices: after the last block its change lists, then the slice's sums
template <class real>
__global__ __launch_bounds__(256) void k_mtj_finish(const FinishArgs A)
{
    __shared__ double sh[4 * kRec];
    const real* __restrict__ X = (const real*)A.X;
    const int64_t row = (int64_t)blockIdx.x * jwg::kRows + threadIdx.x;
    double r[kMaxT], acc[kRec];
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) {
        r[k] = 0.0;
        if (k < A.T) {
            double v = A.R[(int64_t)k * A.ld + row];
            const int nev = A.ev->count[k];
            for (int e = 0; e < nev; ++e) v = v + (double)X[(int64_t)A.ev->idx[k][e] * A.ld + row] * A.ev->d[k][e];
            if (nev > 0) A.R[(int64_t)k * A.ld + row] = v;
            r[k] = v;
        }
    }
    pairs_of(r, acc, [](int, double v) { return v; });
    jwu::block_reduce<kRec>(acc, sh, A.fin + (int64_t)blockIdx.x * kRec);
}

}  // namespace jwj
