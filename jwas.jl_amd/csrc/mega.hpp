// mega.hpp -- mega-trait models on the device: constraint=true with up to 64 traits, the sweep of megaBayesABC! / megaBayesC0!
// (markers/BayesianAlphabet/BayesABC.jl:1-8): T independent single-trait chains over ONE genotype matrix.
//
// n individuals (genotype rows, the context's dense Float32 or Float64 matrix X, [p][ld], pad rows 0), T traits.  Per trait k:
// the residual r_k [ld] (pad rows 0), alpha_k, beta_k, delta_k [p] and their running means; vare_k = vare[k,k], v_k the trait's
// marker-effect variance, pi_k the trait's exclusion probability.  Shared by all traits, fixed at set-up (double):
//   xpx_j = x_j'x_j                       G_ij = x_i'x_j for the marker pairs WITHIN a block (G_jj and xpx_j are the same sum)
// One marker of one trait, markers in order (bayesabc_update_marker!, BayesABC.jl:24-58):
//   rhs = (x_j'r + xpx_j alpha_j) / vare,   lhs = xpx_j / vare + 1 / v,   gHat = rhs / lhs
//   logDelta1 = -0.5 (log lhs + log v - gHat rhs) + log(1 - pi),   logDelta0 = log pi,   probDelta1 = 1 / (1 + exp(logDelta0 - logDelta1))
//   u < probDelta1:  delta = 1, beta = gHat + z sqrt(1 / lhs), alpha = beta;   else  delta = 0, beta = z sqrt(v), alpha = 0
//   r += x_j (alpha_old - alpha_new).   pi = 0 (RR-BLUP, megaBayesC0!): logDelta0 = -Inf, exp(-Inf) = 0, probDelta1 = 1 -- no NaN.
//
// EXACT BLOCK FORM (as rrm.hpp).  For a block B: s_j[k] = x_j'r_k for all j in B and all k from the residual at block entry; when
// marker j of trait k changes by d = alpha_old - alpha_new, s_i[k] += G_ij d for every i in B; at block exit r_k += sum_j x_j d_jk.
// Per block two stream-ordered launches, no lookahead:
//   k_mega_update_partial  grid (row slices, trait tiles): one 256-row slice and kTT = 8 traits per workgroup.  Phase 1, one row per
//                          thread: the previous block's change list of every trait of the tile is applied to the row in list order
//                          (r = r + x * d), the row's values go to LDS [trait][row].  Phase 2, a split-K GEMM over the rows: the
//                          slice's b x kTT tile of X_b'R.  The 256 threads are `parts` = 256 / bp row parts x bp markers (bp = 64,
//                          128 or 256, the smallest that holds the block); a thread adds its part's rows in ascending order into
//                          one accumulator per trait (x read four rows at a time, the residual broadcast from LDS), the parts meet
//                          in LDS in ascending order.
//   k_mega_sample          one workgroup per trait: s = the slice partials in ascending slice order (one marker per thread); wave 0
//                          walks the block 64 markers at a time by speculative evaluation (every pending lane tests its marker
//                          against the current s, the first changed marker commits, its Gram row -- b doubles, read from L2 --
//                          corrects s); the trait's change list and statistics.
//   k_mega_sample_r        the same walk (mega_walk) under the 4-class law of BayesR (LawR, below): K chains of one model are K
//                          traits with the same record.
//   k_mega_finish          grid (row slices, traits): the last change list, then sum r^2 and sum r of the slice.
//   k_mega_impute          grid (row chunks, traits): a missing cell (bit mask [T][ld / 32]) is redrawn from N(0, vare_k) -- with a
//                          diagonal R the conditional law of a missing residual whatever the record's other traits
//                          (sampleMissingResiduals, residual.jl:51-73, with Rc = 0).  Observed cells and pad rows are never written.
//
// ORDER OF EVERY SUM (no floating-point atomics: the same seed gives the same bits; NO sum of trait k depends on T or on the
// position of the trait inside its tile).  A slice partial: a thread adds the rows of its part ascending, the parts are added
// ascending ((p0 + p1) + p2) + p3.  s: the slices ascending.  xpx_j and G_ij: a thread adds rows tid, tid + 256, ... ascending, a
// wave meets in a shuffle tree (32 .. 1), the four waves in wave order.  Statistics of a trait: per lane in marker order, a shuffle
// tree, the blocks in stream order.  sum r^2 and sum r: per slice the shuffle tree and the four waves in order, then (on the host)
// the slices ascending.
//
// DRAWS: philox4x32_10(marker, iteration, 0x01000000 | trait_id, slot): slot 10 the decision uniform (u52 of words (1, 0)), slot 11
// the effect normal (Box-Muller, jwu::normal_from); philox4x32_10(record, iteration, 0x01000000 | trait_id, 12) the normal of a
// missing cell.  trait_id = first_trait + k: trait k of a T-trait session draws what trait 0 of a one-trait session with
// first_trait = k draws.  They do not depend on the block size.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwg {

constexpr int kMaxT = 64;                       // traits of a session
constexpr int kMaxBlock = 256;                  // markers of a block
constexpr int kTT = 8;                          // traits per workgroup of k_mega_update_partial
constexpr int kRows = 256;                      // rows per slice (= the context's)
constexpr uint32_t kTag = 0x01000000u;
constexpr uint32_t kMaxTraitId = 0x01000000u;   // first_trait + T <= this: the tag's low 24 bits
constexpr uint32_t kSlotU = 10u, kSlotZ = 11u, kSlotMiss = 12u;
// the device record of a trait's statistics
constexpr int kStDelta = 0, kStBeta = 1, kStAlpha = 2, kStChanged = 3, kStSize = 4;
// the per-trait parameters of a sweep: par[q * T + k]
constexpr int kParVare = 0, kParVar = 1, kParLogPi = 2, kParLogPiComp = 3, kParSize = 4;

// The change lists of a block: per trait the markers whose effect moved and d = alpha_old - alpha_new.
struct Events {
    int32_t count[kMaxT];
    int32_t idx[kMaxT][kMaxBlock];
    double d[kMaxT][kMaxBlock];
};

// ---- set-up ------------------------------------------------------------------------------------------------------------------------
// The Grams of the blocks: gram[(blk bs + a) bs + k] = sum_i x_ia x_ik for the markers a, k of block blk.  grid = (bs, nblocks):
// workgroup (a, blk) forms the pairs k >= a and writes both (a, k) and (k, a): symmetric bit for bit; the pair (a, a) is also xpx.
template <class real>
__global__ __launch_bounds__(256) void k_mega_gram(const real* __restrict__ X, int64_t ld, int64_t p, int32_t bs, double* __restrict__ gram,
                                                   double* __restrict__ xpx)
{
    __shared__ double sh[4];
    __shared__ double outv[1];
    const int a = blockIdx.x;
    const int64_t j0 = (int64_t)blockIdx.y * bs;
    const int b = (int)((p - j0) < bs ? (p - j0) : bs);
    if (a >= b) return;
    const real* __restrict__ xa = X + (j0 + a) * ld;
    double* __restrict__ G = gram + (int64_t)blockIdx.y * bs * bs;
    for (int k = a; k < b; ++k) {
        const real* __restrict__ xk = X + (j0 + k) * ld;
        double acc[1] = {0.0};
        for (int64_t i = threadIdx.x; i < ld; i += 256) acc[0] = acc[0] + (double)xa[i] * (double)xk[i];
        jwu::block_reduce<1>(acc, sh, outv);
        __syncthreads();
        if (threadIdx.x == 0) {
            const double v = outv[0];
            G[(int64_t)a * bs + k] = v;
            G[(int64_t)k * bs + a] = v;
            if (k == a) xpx[j0 + a] = v;
        }
        __syncthreads();
    }
}

// ---- the block right-hand sides -----------------------------------------------------------------------------------------------------
struct UpdateArgs {
    const void* X;                      // [p][ld] genotypes (real)
    double* R;                          // [T][ld]
    const Events* ev;                   // the previous block's change lists (NULL: none)
    double* partials;                   // [nslices][T][bs]
    int64_t ld, j0;
    int32_t T, b, bs;
};

// grid = (nslices, ceil(T / kTT)) workgroups of 256 threads
template <class real>
__global__ __launch_bounds__(256) void k_mega_update_partial(const UpdateArgs A)
{
    __shared__ double Rs[kTT][kRows];   // the tile's residual, [trait][row]
    __shared__ double red[kTT][kRows];  // the parts' sums, [trait][part * bp + marker]
    const real* __restrict__ X = (const real*)A.X;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRows, row = row0 + tid;
    const int k0 = (int)blockIdx.y * kTT;
    // phase 1: the previous block's change lists, one row per thread
#pragma unroll
    for (int kk = 0; kk < kTT; ++kk) {
        const int k = k0 + kk;
        double r = 0.0;
        if (k < A.T) {
            r = A.R[(int64_t)k * A.ld + row];
            const int nev = A.ev ? A.ev->count[k] : 0;
            for (int e = 0; e < nev; ++e) r = r + (double)X[(int64_t)A.ev->idx[k][e] * A.ld + row] * A.ev->d[k][e];
            if (nev > 0) A.R[(int64_t)k * A.ld + row] = r;
        }
        Rs[kk][tid] = r;
    }
    __syncthreads();
    // phase 2: the slice's tile of X_b'R
    const int bp = A.b <= 64 ? 64 : (A.b <= 128 ? 128 : 256), parts = kRows / bp, len = kRows / parts;
    const int m = tid & (bp - 1), part = tid / bp;
    double acc[kTT];
#pragma unroll
    for (int kk = 0; kk < kTT; ++kk) acc[kk] = 0.0;
    if (m < A.b) {
        const int i0 = part * len;
        const real* __restrict__ x = X + (A.j0 + m) * A.ld + row0 + i0;
        for (int i = 0; i < len; i += 4) {
            double xv[4];
            jwu::load4(x + i, xv);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int kk = 0; kk < kTT; ++kk) acc[kk] = acc[kk] + xv[u] * Rs[kk][i0 + i + u];
        }
    }
    if (parts > 1) {
#pragma unroll
        for (int kk = 0; kk < kTT; ++kk) red[kk][tid] = acc[kk];
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int kk = 0; kk < kTT; ++kk) {
                double s = red[kk][m];
                for (int q = 1; q < parts; ++q) s = s + red[kk][q * bp + m];
                acc[kk] = s;
            }
        }
    }
    if (part == 0 && m < A.b) {
#pragma unroll
        for (int kk = 0; kk < kTT; ++kk)
            if (k0 + kk < A.T) A.partials[((int64_t)blockIdx.x * A.T + k0 + kk) * A.bs + m] = acc[kk];
    }
}

// What follows is the mega-trait session's own.  A unit that shares only the block form above (mtjoint.hpp) defines
// JWG_BLOCK_FORM_ONLY: a non-template __global__ in two units would be a duplicate host symbol at link time.
#ifndef JWG_BLOCK_FORM_ONLY
struct FinishArgs {
    const void* X;
    double* R;
    const Events* ev;
    double* fin;                        // [T][nslices][2]: sum r^2, sum r of the slice
    int64_t ld;
    int32_t T;
};

// grid = (nslices, T): after the last block its change list, then the slice's sums
template <class real>
__global__ __launch_bounds__(256) void k_mega_finish(const FinishArgs A)
{
    __shared__ double sh[8];
    const real* __restrict__ X = (const real*)A.X;
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x;
    const int k = blockIdx.y;
    double r = A.R[(int64_t)k * A.ld + row];
    const int nev = A.ev ? A.ev->count[k] : 0;
    for (int e = 0; e < nev; ++e) r = r + (double)X[(int64_t)A.ev->idx[k][e] * A.ld + row] * A.ev->d[k][e];
    if (nev > 0) A.R[(int64_t)k * A.ld + row] = r;
    const double acc[2] = {r * r, r};
    jwu::block_reduce<2>(acc, sh, A.fin + ((int64_t)k * gridDim.x + blockIdx.x) * 2);
}

// ---- one block of one trait ----------------------------------------------------------------------------------------------------------
struct SampleArgs {
    const double* partials;             // [nslices][T][bs]
    const double* gram;                 // this block's [bs][bs]
    const double* xpx;                  // [p]
    const double* par;                  // [kParSize][T]
    double *alpha, *beta, *delta;       // [T][p]
    Events* ev;                         // out
    double* stat;                       // [T][kStSize], accumulated over the blocks of a sweep
    int64_t j0, p;
    int32_t nslices, b, bs, T;
    uint32_t iter, seed_lo, seed_hi, first_trait;
};

// The law of one marker under megaBayesABC! (this file's header): what k_mega_sample gives the walk.
struct LawC {
    static constexpr int kStats = kStSize;
    static constexpr bool kBetaIsAlpha = false;
    double ie, iv, logv, sdv, lp0, lpc;         // of the trait
    double invLhs, loglhs, sdl;                 // of the marker
    __device__ __forceinline__ LawC(const double* __restrict__ par, int T, int k)
    {
        const double vare = par[kParVare * T + k], v = par[kParVar * T + k];
        lp0 = par[kParLogPi * T + k]; lpc = par[kParLogPiComp * T + k];
        ie = 1.0 / vare; iv = 1.0 / v; logv = log(v); sdv = sqrt(v);
    }
    __device__ __forceinline__ void marker(double xx)
    {
        const double lhs = xx * ie + iv;
        invLhs = 1.0 / lhs; loglhs = log(lhs); sdl = sqrt(invLhs);
    }
    // s = x_j'r, the marker's current effect a -> the candidate (alpha, beta, delta)
    __device__ __forceinline__ void draw(double s, double xx, double a, double u, double z, double& an, double& bn, double& dn) const
    {
        const double rhs = (s + xx * a) * ie;
        const double gHat = rhs * invLhs;
        const double ld1 = -0.5 * (loglhs + logv - gHat * rhs) + lpc;
        const double prob = 1.0 / (1.0 + exp(lp0 - ld1));
        const bool inc = u < prob;
        bn = inc ? gHat + z * sdl : z * sdv;
        an = inc ? bn : 0.0;
        dn = inc ? 1.0 : 0.0;
    }
    __device__ __forceinline__ void record(double (&st)[kStats], double a, double b, double d, bool changed) const
    {
        st[kStDelta] = st[kStDelta] + d;
        st[kStBeta] = st[kStBeta] + b * b;
        st[kStAlpha] = st[kStAlpha] + a * a;
        if (changed) st[kStChanged] = st[kStChanged] + 1.0;
    }
};

// The 4-class law of BayesR (markers/BayesianAlphabet/BayesR.jl:56-96), all in double: what k_mega_sample_r gives the walk.  Per chain
// vare, sigma2, gamma[4] (gamma_1 = 0) and log pi[4]; one marker:
//   rhs = (s + xpx alpha) / vare;  class c = 2..4: v_c = gamma_c sigma2, lhs_c = xpx / vare + 1 / v_c, bHat_c = rhs / lhs_c,
//   lp_c = 0.5 (log(1 / lhs_c) - log v_c + bHat_c rhs) + log pi_c;  lp_1 = log pi_1
//   probs_c = exp(lp_c - (mx + log sum_c exp(lp_c - mx))), mx = max lp (the sum over c ascending)
//   the class: cp = probs_1, while cp <= u the next class is added (rand(Categorical), the CDF walk)
//   class 1: alpha = 0;  class c: alpha = bHat_c + z sqrt(1 / lhs_c);  delta = the class, 1..4;  beta = alpha
// Draws: slot 10 the uniform, slot 11 the normal, trait_id = first_trait + k, as under LawC.
constexpr int kClasses = 4;
// the device record of a BayesR chain's statistics
constexpr int kStRCount = 0, kStRSsq = 4, kStRNnz = 5, kStRAlpha = 6, kStRChanged = 7, kStRSize = 8;
// the per-chain parameters of a BayesR sweep: par[q * T + k]
constexpr int kParRVare = 0, kParRVar = 1, kParRGamma = 2, kParRLogPi = 6, kParRSize = 10;

struct LawR {
    static constexpr int kStats = kStRSize;
    static constexpr bool kBetaIsAlpha = true;
    double ie, lp1, gam[3], iv[3], logv[3], lpi[3];         // of the chain (the arrays: the classes 2..4)
    double invLhs[3], lconst[3], sdl[3];                    // of the marker
    __device__ __forceinline__ LawR(const double* __restrict__ par, int T, int k)
    {
        const double vare = par[kParRVare * T + k], sig = par[kParRVar * T + k];
        ie = 1.0 / vare;
        lp1 = par[kParRLogPi * T + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double g = par[(kParRGamma + 1 + c) * T + k], vc = g * sig;
            gam[c] = g; iv[c] = 1.0 / vc; logv[c] = log(vc);
            lpi[c] = par[(kParRLogPi + 1 + c) * T + k];
        }
    }
    __device__ __forceinline__ void marker(double xx)
    {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double lhs = xx * ie + iv[c];
            invLhs[c] = 1.0 / lhs;
            lconst[c] = log(invLhs[c]) - logv[c];
            sdl[c] = sqrt(invLhs[c]);
        }
    }
    __device__ __forceinline__ void draw(double s, double xx, double a, double u, double z, double& an, double& bn, double& dn) const
    {
        const double rhs = (s + xx * a) * ie;
        double bh[3], lp[3], mx = lp1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bh[c] = rhs * invLhs[c];
            lp[c] = 0.5 * (lconst[c] + bh[c] * rhs) + lpi[c];
            mx = lp[c] > mx ? lp[c] : mx;
        }
        const double se = ((exp(lp1 - mx) + exp(lp[0] - mx)) + exp(lp[1] - mx)) + exp(lp[2] - mx);
        const double ln = mx + log(se);
        // the CDF walk: the class is the first whose cumulated probability exceeds u (the last class takes the rest)
        double cp = exp(lp1 - ln);
        int cls = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (cls == c && cp <= u) { cls = c + 1; cp = cp + exp(lp[c] - ln); }
        }
        const double bsel = cls == 1 ? bh[0] : (cls == 2 ? bh[1] : bh[2]);
        const double sd2 = sdl[0], sd3 = sdl[1], sd4 = sdl[2];      // (values, not members: a choice among members stays in memory)
        const double ssel = cls == 1 ? sd2 : (cls == 2 ? sd3 : sd4);
        an = cls == 0 ? 0.0 : bsel + z * ssel;
        bn = an;
        dn = (double)(cls + 1);
    }
    __device__ __forceinline__ void record(double (&st)[kStats], double a, double, double d, bool changed) const
    {
        const double a2 = a * a;
#pragma unroll
        for (int c = 0; c < kClasses; ++c)
            if (d == (double)(c + 1)) st[kStRCount + c] = st[kStRCount + c] + 1.0;
        if (d > 1.0) {
            const double g2 = gam[0], g3 = gam[1], g4 = gam[2];
            const double gs = d == 2.0 ? g2 : (d == 3.0 ? g3 : g4);
            st[kStRSsq] = st[kStRSsq] + a2 / gs;
            st[kStRNnz] = st[kStRNnz] + 1.0;
        }
        st[kStRAlpha] = st[kStRAlpha] + a2;
        if (changed) st[kStRChanged] = st[kStRChanged] + 1.0;
    }
};

// One block of one trait under `Law`: every thread adds the slice partials of one marker, then wave 0 runs the trait's chain.
// A.par is the law's [.][T] table, A.stat its [T][Law::kStats] record.
template <class Law>
__device__ __forceinline__ void mega_walk(const SampleArgs& A)
{
    __shared__ double s_s[kMaxBlock], s_a0[kMaxBlock];
    const int lane = threadIdx.x & 63, k = blockIdx.x;
    const int b = A.b, bs = A.bs;
    double* __restrict__ alpha = A.alpha + (int64_t)k * A.p;
    double* __restrict__ beta = A.beta + (int64_t)k * A.p;
    double* __restrict__ delta = A.delta + (int64_t)k * A.p;
    for (int i = threadIdx.x; i < b; i += 256) {
        const double* __restrict__ part = A.partials + (int64_t)k * bs + i;
        const int64_t stride = (int64_t)A.T * bs;
        double s = 0.0;
#pragma unroll 8
        for (int sl = 0; sl < A.nslices; ++sl) s = s + part[sl * stride];      // (ascending; the loads of a batch are in flight together)
        s_s[i] = s;
        s_a0[i] = alpha[A.j0 + i];
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    Law law(A.par, A.T, k);
    const uint32_t tag = kTag | (A.first_trait + (uint32_t)k);
    double st_acc[Law::kStats];
#pragma unroll
    for (int i = 0; i < Law::kStats; ++i) st_acc[i] = 0.0;
    const int nsub = (b + 63) / 64;
    int base = 0;
#pragma unroll 1
    for (int s = 0; s < nsub; ++s) {
        const int kq = 64 * s + lane;
        const bool valid = kq < b;
        const int kl = valid ? kq : 0;
        const int64_t j = A.j0 + kl;
        const double xx = A.xpx[j];
        const double z = jwu::normal_from(jw::philox4x32_10((uint32_t)j, A.iter, tag, kSlotZ, A.seed_lo, A.seed_hi));
        const jw::u32x4 wu = jw::philox4x32_10((uint32_t)j, A.iter, tag, kSlotU, A.seed_lo, A.seed_hi);
        const double u = jw::u52(wu.x, wu.y);
        law.marker(xx);
        double a_cur = s_a0[kl], b_cur = Law::kBetaIsAlpha ? 0.0 : beta[j], d_cur = delta[j];
        unsigned long long pending = __ballot(valid);
        while (pending) {
            double an, bn, dn;
            law.draw(s_s[kl], xx, a_cur, u, z, an, bn, dn);
            const int kw = jwu::first_changed(an != a_cur && valid, pending);
            // lanes before the winner are final with what they just evaluated (their effects do not move)
            const unsigned long long done = jwu::final_lanes(pending, kw);
            if ((done >> lane) & 1ull) { b_cur = bn; d_cur = dn; }
            if (kw >= 64) break;
            // the winner commits; its Gram row corrects s of the whole block: s_i += G_i,ce d
            const int ce = 64 * s + kw;
            const double Dl = a_cur - an;
            const double D = __shfl(Dl, kw, 64);
            if (lane == kw) a_cur = an;
            const double* __restrict__ grow = A.gram + (int64_t)ce * bs;
            __builtin_amdgcn_wave_barrier();                // (one wave: its LDS accesses execute in program order)
            for (int k2 = lane; k2 < b; k2 += 64) s_s[k2] = s_s[k2] + grow[k2] * D;
            __builtin_amdgcn_wave_barrier();
            pending &= ~done;
        }
        // the sub-block is final: state, change list, statistics
        const bool changed = valid && (a_cur != s_a0[kl]);
        const int e = jwu::list_entry(changed, lane, base);
        if (changed) {
            A.ev->idx[k][e] = (int32_t)j;
            A.ev->d[k][e] = s_a0[kl] - a_cur;
        }
        if (valid) {
            alpha[j] = a_cur; beta[j] = Law::kBetaIsAlpha ? a_cur : b_cur; delta[j] = d_cur;
            law.record(st_acc, a_cur, b_cur, d_cur, changed);
        }
    }
    // the block's statistics join the sweep's: shuffle tree, lane 0 adds (the blocks of a sweep run in stream order)
#pragma unroll
    for (int i = 0; i < Law::kStats; ++i) st_acc[i] = jwu::wave_sum(st_acc[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < Law::kStats; ++i) A.stat[k * Law::kStats + i] = A.stat[k * Law::kStats + i] + st_acc[i];
        A.ev->count[k] = base;
    }
}

// grid = T workgroups of 256 threads; par [kParSize][T], stat [T][kStSize]
__global__ __launch_bounds__(256) void k_mega_sample(const SampleArgs A) { mega_walk<LawC>(A); }

// ... of T BayesR chains: par [kParRSize][T], stat [T][kStRSize]
__global__ __launch_bounds__(256) void k_mega_sample_r(const SampleArgs A) { mega_walk<LawR>(A); }

// ---- missing cells ---------------------------------------------------------------------------------------------------------------------
// grid = (ceil(n / 256), T): r_k[i] = z sqrt(vare_k) where bit i of the trait's mask is set; nothing else is written
__global__ __launch_bounds__(256) void k_mega_impute(const uint32_t* __restrict__ mask, int64_t words, int64_t n, int64_t ld, const double* __restrict__ vare,
                                                     uint32_t iter, uint32_t seed_lo, uint32_t seed_hi, uint32_t first_trait, double* __restrict__ R)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    if (!((mask[(int64_t)k * words + (i >> 5)] >> (i & 31)) & 1u)) return;
    const double z = jwu::normal_from(jw::philox4x32_10((uint32_t)i, iter, kTag | (first_trait + (uint32_t)k), kSlotMiss, seed_lo, seed_hi));
    R[(int64_t)k * ld + i] = z * sqrt(vare[k]);
}

// ---- outputs (the running means and X alpha: marker_state.hpp) -----------------------------------------------------------------------------
// The potential scale reduction factor of every marker effect (Gelman and Rubin) from the running means m_k and means of squares q_k
// of K chains after N saved samples: s_k^2 = N / (N - 1) (q_k - m_k^2), W = mean_k s_k^2, B / N = sum_k (m_k - mean m)^2 / (K - 1),
// V = (N - 1) / N W + B / N, out = sqrt(V / W); W == 0 (the marker never entered the model in any chain): NaN.  One thread per marker,
// the chains added in ascending order; at most kPsrfBlocks workgroups, the markers beyond them in further trips of the same threads.
constexpr int kPsrfBlocks = 64;
__global__ __launch_bounds__(256) void k_mega_psrf(const double* __restrict__ mean_a, const double* __restrict__ mean_a2, int64_t p, int32_t K, double N,
                                                   double* __restrict__ out)
{
    const double f = N / (N - 1.0), g = (N - 1.0) / N;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p; j += (int64_t)gridDim.x * 256) {
        double sm = 0.0, sw = 0.0;
        for (int k = 0; k < K; ++k) {
            const double m = mean_a[(int64_t)k * p + j];
            sm = sm + m;
            sw = sw + f * (mean_a2[(int64_t)k * p + j] - m * m);
        }
        const double mbar = sm / (double)K, W = sw / (double)K;
        double sb = 0.0;
        for (int k = 0; k < K; ++k) {
            const double e = mean_a[(int64_t)k * p + j] - mbar;
            sb = sb + e * e;
        }
        const double V = g * W + sb / (double)(K - 1);
        out[j] = W == 0.0 ? __builtin_nan("") : sqrt(V / W);
    }
}
#endif  // JWG_BLOCK_FORM_ONLY

}  // namespace jwg
