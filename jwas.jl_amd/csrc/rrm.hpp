// rrm.hpp -- random regression models on the device: the marker sweep of runMCMC(...; RRM = Phi).
//
// The reference (RRM/RRM.jl:101-158 BayesABCRRM!, RRM/MCMC_BayesianAlphabet_RRM.jl) gives every marker C regression coefficients and
// every individual up to T records, one per time point.  n individuals (genotype rows x_i.), Phi the T x C matrix with rows phi_t,
// m_it = 1 when individual i has a record at time t (bit t of the individual's 64-bit mask word; pad rows have mask 0), W the T x n
// residual (the reference's yfull: EXACTLY 0 wherever m_it = 0, RRM.jl:12-20,151), vare a scalar, G C x C, pi a table over 2^C states.
//
// Fixed at set-up (all double):
//   O_i  = sum_t m_it phi_t phi_t'            C x C symmetric, cells = C (C + 1) / 2 lower cells: cell(a, b) = a (a + 1) / 2 + b, b <= a
//   M_j  = sum_i x_ij^2 O_i                   get_mPhiPhiarray, RRM.jl:43-57
//   G_jk = sum_i x_ij x_ik O_i                for the marker pairs WITHIN a block (the block Gram tensor; G_jj = M_j, G_jk = G_kj)
// One marker, markers in order:
//   s_j  = sum_i x_ij sum_t m_it phi_t W_it                         (Phi' of the reference's T dots, RRM.jl:108-112)
//   xw   = s_j + M_j alpha_j
//   every state D = diag(delta), bit q of the state index = coefficient q:
//       lhs = D M_j D / vare + G^-1,  rhs = D xw / vare,  lhs = L L',  inv = L^-T L^-1,  mu = inv rhs
//       logDelta = -0.5 (log prod L_ii^2 - rhs'mu) + log pi(state)                                          (RRM.jl:115-122)
//   state ~ Categorical(softmax(logDelta)): ONE uniform, CDF walk in state-index order, the last state when rounding leaves u above
//   the total;  beta = mu + chol(inv) z with ONE shared z in R^C (the convention of the multi-trait sampler II: only the chosen
//   state's candidate is formed);  alpha_new = D beta;  W_it += m_it x_ij phi_t'(alpha_j - alpha_new).
// The reference draws one MvNormal per candidate state and indexes three dictionaries by one position (RRM.jl:138-141); this file
// implements the law above, not the dictionary order.
//
// EXACT BLOCK FORM.  For a block B: s_k for all k in B from the residual at block entry; whenever marker j in B changes by
// d = alpha_old - alpha_new, s_k += G_kj d for every k in B; at block exit W_it += m_it sum_{j in B} x_ij (phi_t'd_j).  Per block two
// stream-ordered launches, no lookahead:
//   k_rrm_update_partial   one 256-row slice per workgroup, one row per thread: the previous block's change list is applied to the
//                          row's T residual values under its mask word (eight time points in registers at a time, the changed
//                          columns in list order: w = w + x * g_et with g_et = phi_t'd_e formed once by the sampler), v_i = sum_t
//                          m_it phi_t W_it (t ascending) in registers, then the slice's partial s_k for the block's markers.
//   k_rrm_sample           one workgroup: s = the slice partials in slice order; wave 0 walks the block, 64 markers at a time by
//                          speculative evaluation (every pending lane tests its marker against the current s, the first changed
//                          marker commits, its Gram row -- b x cells doubles, read from L2 -- corrects s); the change list, the
//                          g_et table and the sweep's statistics.
//   k_rrm_finish           after the last block: the last change list, and sum W^2 per slice.
//
// ORDER OF EVERY SUM (no floating-point atomics: the same seed gives the same bits).  A slice partial: the 64 lanes of a wave meet
// in a transposed butterfly (32, 16, 8 exchange halves, then 4, 2, 1), the four waves are added as (w0 + w1) + (w2 + w3); the
// sampler adds the slices in ascending order.  M_j and G_jk: a thread adds rows tid, tid + 256, ... ascending, a wave meets in a
// shuffle tree (32 .. 1), the four waves in wave order.  Statistics: per lane in marker order, a shuffle tree, blocks in order.
//
// DRAWS: philox4x32_10(marker, iteration, 0x02000000, slot): slot 8 the uniform (u52 of words (1, 0)), slot 9 + 16 q the normal of
// coefficient q (Box-Muller, jwu::normal_from).  They do not depend on the block size.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwr {

constexpr int kMaxC = 4, kMinC = 2;
constexpr int kMaxT = 64;
constexpr int kMaxBlock = 256;
constexpr int kMaxCells = kMaxC * (kMaxC + 1) / 2;
constexpr int kMaxStates = 1 << kMaxC;
constexpr int kTC = 8;                          // time points held in registers at a time
constexpr uint32_t kTag = 0x02000000u;
constexpr uint32_t kSlotU = 8u, kSlotZ = 9u;
// the device record of a sweep's statistics
constexpr int kStCounts = 0, kStBeta = 16, kStAlpha = 32, kStChanged = 33, kStSize = 34;

__host__ __device__ constexpr int cells_of(int c) { return c * (c + 1) / 2; }
__host__ __device__ constexpr int cell(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// The change list of a block: the markers whose coefficients moved, d = alpha_old - alpha_new, and g[e][t] = phi_t'd_e.
struct Events {
    int32_t count;
    int32_t idx[kMaxBlock];
    double d[kMaxC][kMaxBlock];
    double g[kMaxBlock * kMaxT];                // [e * T + t]
};

// Eight per-lane values (one per column) -> lane l holds the wave's sum of column (l >> 3) & 7 in every lane of its 8-lane group.
__device__ __forceinline__ double transposed_sum8(const double (&v)[8], int lane)
{
    double a[4], b[2], c;
    const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0, h3 = (lane & 8) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double send = h5 ? v[i] : v[4 + i], keep = h5 ? v[4 + i] : v[i];
        a[i] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double send = h4 ? a[i] : a[2 + i], keep = h4 ? a[2 + i] : a[i];
        b[i] = keep + __shfl_xor(send, 16, 64);
    }
    {
        const double send = h3 ? b[0] : b[1], keep = h3 ? b[1] : b[0];
        c = keep + __shfl_xor(send, 8, 64);
    }
    c = c + __shfl_xor(c, 4, 64);
    c = c + __shfl_xor(c, 2, 64);
    c = c + __shfl_xor(c, 1, 64);
    return c;
}

// ---- set-up ------------------------------------------------------------------------------------------------------------------------
// O[cell][row] = sum_t m_it phi_ta phi_tb (t ascending), one thread per row of the padded matrix (pad rows: mask 0, O = 0)
__global__ __launch_bounds__(256) void k_rrm_o(const uint64_t* __restrict__ mask, const double* __restrict__ phi, int32_t T, int32_t C,
                                               int64_t ld, double* __restrict__ O)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= ld) return;
    const uint64_t m = mask[row];
    for (int a = 0; a < C; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int t = 0; t < T; ++t)
                if ((m >> t) & 1ull) s = s + phi[t * C + a] * phi[t * C + b];
            O[(int64_t)cell(a, b) * ld + row] = s;
        }
}

// M[j][cell] = sum_i x_ij^2 O_i[cell]: one workgroup per marker
template <class real, int C>
__global__ __launch_bounds__(256) void k_rrm_m(const real* __restrict__ X, int64_t ld, const double* __restrict__ O, double* __restrict__ M)
{
    constexpr int NC = cells_of(C);
    __shared__ double sh[4 * NC];
    const real* __restrict__ x = X + (int64_t)blockIdx.x * ld;
    double acc[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = 0.0;
    for (int64_t i = threadIdx.x; i < ld; i += 256) {
        const double xv = (double)x[i], xx = xv * xv;
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = acc[q] + xx * O[(int64_t)q * ld + i];
    }
    jwu::block_reduce<NC>(acc, sh, M + (int64_t)blockIdx.x * NC);
}

// The Gram tensor of the blocks: gram[(blk bs + a) bs + k][cell] = sum_i x_ia x_ik O_i[cell] for the markers a, k of block blk.
// grid = (bs, nblocks): workgroup (a, blk) forms the pairs k >= a and writes both (a, k) and (k, a): symmetric bit for bit.
template <class real, int C>
__global__ __launch_bounds__(256) void k_rrm_gram(const real* __restrict__ X, int64_t ld, const double* __restrict__ O, int64_t p, int32_t bs,
                                                  double* __restrict__ gram)
{
    constexpr int NC = cells_of(C);
    __shared__ double sh[4 * NC];
    __shared__ double outv[NC];
    const int a = blockIdx.x;
    const int64_t j0 = (int64_t)blockIdx.y * bs;
    const int b = (int)((p - j0) < bs ? (p - j0) : bs);
    if (a >= b) return;
    const real* __restrict__ xa = X + (j0 + a) * ld;
    double* __restrict__ G = gram + (int64_t)blockIdx.y * bs * bs * NC;
    for (int k = a; k < b; ++k) {
        const real* __restrict__ xk = X + (j0 + k) * ld;
        double acc[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = 0.0;
        for (int64_t i = threadIdx.x; i < ld; i += 256) {
            const double xx = (double)xa[i] * (double)xk[i];
#pragma unroll
            for (int q = 0; q < NC; ++q) acc[q] = acc[q] + xx * O[(int64_t)q * ld + i];
        }
        jwu::block_reduce<NC>(acc, sh, outv);
        __syncthreads();
        if ((int)threadIdx.x < NC) {
            const double v = outv[threadIdx.x];
            G[((int64_t)a * bs + k) * NC + threadIdx.x] = v;
            G[((int64_t)k * bs + a) * NC + threadIdx.x] = v;
        }
        __syncthreads();
    }
}

// ---- the residual of a row under a change list ---------------------------------------------------------------------------------------
// The time points t0 .. t0 + kTC - 1 of one row: w_u = W[t0 + u][row], then for every entry e of the list in order
// w_u = w_u + x_e * g[e][t0 + u] where the row has a record.  An unobserved cell keeps its exact 0.
template <class real>
__device__ __forceinline__ void apply_chunk(const real* __restrict__ X, int64_t ld, int64_t row, const Events* __restrict__ ev, int nev,
                                            int T, int t0, uint64_t m, const double* __restrict__ W, double (&w)[kTC])
{
#pragma unroll
    for (int u = 0; u < kTC; ++u) w[u] = (t0 + u < T) ? W[(int64_t)(t0 + u) * ld + row] : 0.0;
    for (int e = 0; e < nev; ++e) {
        const double x = (double)X[(int64_t)ev->idx[e] * ld + row];
        const double* __restrict__ g = ev->g + (int64_t)e * T + t0;
#pragma unroll
        for (int u = 0; u < kTC; ++u)
            if (t0 + u < T && ((m >> (t0 + u)) & 1ull)) w[u] = w[u] + x * g[u];
    }
}

struct UpdateArgs {
    const void* X;                      // [p][ld] genotypes (real)
    const uint64_t* mask;               // [ld]
    const double* phi;                  // [T][C]
    double* W;                          // [T][ld]
    const Events* ev;                   // the previous block's change list (NULL: none)
    double* partials;                   // [nslices][bs * C]: (k * C + q)
    int64_t ld, j0;
    int32_t T, b, bs;
};

// grid = nslices workgroups of 256 threads
template <class real, int C>
__global__ __launch_bounds__(256) void k_rrm_update_partial(const UpdateArgs A)
{
    __shared__ double sphi[kMaxT * C];
    __shared__ double red[2][4][8 * C];
    const real* __restrict__ X = (const real*)A.X;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * 256 + tid;
    const int T = A.T;
    for (int i = tid; i < T * C; i += 256) sphi[i] = A.phi[i];
    __syncthreads();
    const uint64_t m = A.mask[row];
    const int nev = A.ev ? A.ev->count : 0;
    double v[C];
#pragma unroll
    for (int q = 0; q < C; ++q) v[q] = 0.0;
    for (int t0 = 0; t0 < T; t0 += kTC) {
        double w[kTC];
        apply_chunk<real>(X, A.ld, row, A.ev, nev, T, t0, m, A.W, w);
#pragma unroll
        for (int u = 0; u < kTC; ++u) {
            if (t0 + u < T) {
                if (nev > 0) A.W[(int64_t)(t0 + u) * A.ld + row] = w[u];
                if ((m >> (t0 + u)) & 1ull) {
#pragma unroll
                    for (int q = 0; q < C; ++q) v[q] = v[q] + sphi[(t0 + u) * C + q] * w[u];
                }
            }
        }
    }
    // the slice's partial s_k, eight markers at a time; the cross-wave scratch is double-buffered (one barrier per batch)
    int ph = 0;
    for (int c0 = 0; c0 < A.b; c0 += 8, ph ^= 1) {
        double xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = (c0 + u < A.b) ? (double)X[(A.j0 + c0 + u) * A.ld + row] : 0.0;
#pragma unroll
        for (int q = 0; q < C; ++q) {
            double pr[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) pr[u] = xv[u] * v[q];
            const double s = transposed_sum8(pr, lane);
            if ((lane & 7) == 0) red[ph][wave][(lane >> 3) * C + q] = s;
        }
        __syncthreads();
        if (tid < 8 * C) {
            const int u = tid / C;
            if (c0 + u < A.b)
                A.partials[(int64_t)blockIdx.x * A.bs * C + (int64_t)c0 * C + tid] = (red[ph][0][tid] + red[ph][1][tid]) + (red[ph][2][tid] + red[ph][3][tid]);
        }
    }
}

struct FinishArgs {
    const void* X;
    const uint64_t* mask;
    double* W;
    const Events* ev;
    double* wss;                        // [nslices] sum W^2 of the slice
    int64_t ld;
    int32_t T;
};

// after the last block: its change list, and sum_t sum_i W_it^2 per slice (t ascending per row, then the block tree)
template <class real>
__global__ __launch_bounds__(256) void k_rrm_finish(const FinishArgs A)
{
    __shared__ double sh[4];
    const real* __restrict__ X = (const real*)A.X;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t m = A.mask[row];
    const int nev = A.ev ? A.ev->count : 0;
    double acc[1] = {0.0};
    for (int t0 = 0; t0 < A.T; t0 += kTC) {
        double w[kTC];
        apply_chunk<real>(X, A.ld, row, A.ev, nev, A.T, t0, m, A.W, w);
#pragma unroll
        for (int u = 0; u < kTC; ++u) {
            if (t0 + u < A.T) {
                if (nev > 0) A.W[(int64_t)(t0 + u) * A.ld + row] = w[u];
                acc[0] = acc[0] + w[u] * w[u];
            }
        }
    }
    jwu::block_reduce<1>(acc, sh, A.wss + blockIdx.x);
}

// ---- one marker -----------------------------------------------------------------------------------------------------------------------
// One candidate state: q = -0.5 (log det lhs - rhs'mu); with want_cand the candidate mu + chol(inv(lhs)) z.
template <int C>
__device__ __forceinline__ void rrm_state(const double (&Mj)[C][C], const double (&Gi)[C][C], unsigned st, double ie, const double (&xw)[C],
                                          const double (&z)[C], bool want_cand, double& q, double (&cand)[C])
{
    double lhs[C][C], L[C][C], Li[C][C], inv[C][C], rhs[C];
#pragma unroll
    for (int a = 0; a < C; ++a) {
        const double Da = ((st >> a) & 1u) ? 1.0 : 0.0;
#pragma unroll
        for (int b = 0; b < C; ++b) {
            const double Db = ((st >> b) & 1u) ? 1.0 : 0.0;
            lhs[a][b] = ((Da * Mj[a][b]) * Db) * ie + Gi[a][b];
        }
        rhs[a] = (Da * xw[a]) * ie;
    }
    jwu::chol_lower<C>(lhs, L);
#pragma unroll
    for (int a = 0; a < C; ++a)
#pragma unroll
        for (int b = 0; b < C; ++b) Li[a][b] = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) {                                                   // Li = L^-1
        Li[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < C; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) s = s + L[i][k] * Li[k][j];
            Li[i][j] = -s / L[i][i];
        }
    }
#pragma unroll
    for (int a = 0; a < C; ++a)                                                     // inv(lhs) = Li'Li
#pragma unroll
        for (int b = 0; b < C; ++b) {
            double s = 0.0;
#pragma unroll
            for (int k = (a > b ? a : b); k < C; ++k) s = s + Li[k][a] * Li[k][b];
            inv[a][b] = s;
        }
    double det = 1.0;
#pragma unroll
    for (int j = 0; j < C; ++j) det = det * (L[j][j] * L[j][j]);
    double quad = 0.0, mu[C];
#pragma unroll
    for (int a = 0; a < C; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < C; ++b) s = s + inv[a][b] * rhs[b];
        mu[a] = s;
        quad = quad + rhs[a] * s;
    }
    q = -0.5 * (log(det) - quad);
    if (!want_cand) return;
    double K[C][C];
    jwu::chol_lower<C>(inv, K);
#pragma unroll
    for (int a = 0; a < C; ++a) {
        double s = mu[a];
#pragma unroll
        for (int b = 0; b <= a; ++b) s = s + K[a][b] * z[b];
        cand[a] = s;
    }
}

// Every state's log density, the categorical draw, the chosen state's candidate.  ldst: the lane's LDS column (stride 64).
template <int C>
__device__ __forceinline__ int rrm_eval(const double (&Mj)[C][C], const double (&Gi)[C][C], const double* __restrict__ lpi, double ie,
                                        const double (&xw)[C], double u, const double (&z)[C], double* ldst, double (&cand)[C])
{
    constexpr int NS = 1 << C;
    double q, mx = -INFINITY;
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
        rrm_state<C>(Mj, Gi, (unsigned)s, ie, xw, z, false, q, cand);
        const double v = q + lpi[s];
        ldst[s * 64] = v;
        mx = v > mx ? v : mx;
    }
    double den = 0.0;
#pragma unroll 1
    for (int s = 0; s < NS; ++s) { const double e = exp(ldst[s * 64] - mx); ldst[s * 64] = e; den = den + e; }
    int which = NS - 1;
    double cp = 0.0;
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
        cp = cp + ldst[s * 64] / den;
        if (u < cp) { which = s; break; }
    }
    rrm_state<C>(Mj, Gi, (unsigned)which, ie, xw, z, true, q, cand);
    return which;
}

struct SampleArgs {
    const double* partials;             // [nslices][bs * C]
    const double* gram;                 // this block's [bs][bs][cells]
    const double* M;                    // [p][cells]
    const double* phi;                  // [T][C]
    double *alpha, *beta, *delta;       // [C][p]
    Events* ev;                         // out
    double* stat;                       // [kStSize], accumulated over the blocks of a sweep
    double Ginv[kMaxC * kMaxC];         // row-major, stride C
    double lpi[kMaxStates];
    double ie;                          // 1 / vare
    int64_t j0, p;
    int32_t nslices, b, bs, T;
    uint32_t iter, seed_lo, seed_hi;
};

// one workgroup of 256 threads; wave 0 runs the chain
template <int C>
__global__ __launch_bounds__(256) void k_rrm_sample(const SampleArgs A)
{
    constexpr int NC = cells_of(C), NS = 1 << C;
    __shared__ double s_s[kMaxBlock * C], s_a[kMaxBlock * C], s_a0[kMaxBlock * C], s_b[kMaxBlock * C], s_d[kMaxBlock * C];
    __shared__ double s_ld[NS * 64];
    __shared__ double s_dl[kMaxBlock * C];        // the change list's d, [e * C + q]
    __shared__ double s_phi[kMaxT * C];
    __shared__ int s_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = A.b, bs = A.bs;
    for (int i = tid; i < A.T * C; i += 256) s_phi[i] = A.phi[i];
    for (int i = tid; i < b * C; i += 256) {
        const int k = i / C, q = i - k * C;
        double s = 0.0;
        for (int sl = 0; sl < A.nslices; ++sl) s = s + A.partials[(int64_t)sl * bs * C + i];
        s_s[i] = s;
        const double a0 = A.alpha[(int64_t)q * A.p + A.j0 + k];
        s_a[i] = a0; s_a0[i] = a0;
        s_b[i] = A.beta[(int64_t)q * A.p + A.j0 + k];
        s_d[i] = A.delta[(int64_t)q * A.p + A.j0 + k];
    }
    __syncthreads();
    if (wave == 0) {
        const int nsub = (b + 63) / 64;
        double Gi[C][C];
#pragma unroll
        for (int a = 0; a < C; ++a)
#pragma unroll
            for (int c2 = 0; c2 < C; ++c2) Gi[a][c2] = A.Ginv[a * C + c2];
        double st_acc[NC + 2];                    // beta'beta cells | sum alpha^2 | changed markers
#pragma unroll
        for (int i = 0; i < NC + 2; ++i) st_acc[i] = 0.0;
        double cnt[NS];                           // markers of the lane per state
#pragma unroll
        for (int i = 0; i < NS; ++i) cnt[i] = 0.0;
        int base = 0;
#pragma unroll 1
        for (int s = 0; s < nsub; ++s) {
            const int k = 64 * s + lane;
            const bool valid = k < b;
            const int kl = valid ? k : 0;
            const int64_t j = A.j0 + kl;
            double Mj[C][C];
#pragma unroll
            for (int a = 0; a < C; ++a)
#pragma unroll
                for (int c2 = 0; c2 < C; ++c2) Mj[a][c2] = A.M[j * NC + cell(a, c2)];
            double z[C];
#pragma unroll
            for (int q = 0; q < C; ++q)
                z[q] = jwu::normal_from(jw::philox4x32_10((uint32_t)j, A.iter, kTag, kSlotZ + 16u * (uint32_t)q, A.seed_lo, A.seed_hi));
            const jw::u32x4 wu = jw::philox4x32_10((uint32_t)j, A.iter, kTag, kSlotU, A.seed_lo, A.seed_hi);
            const double u = jw::u52(wu.x, wu.y);
            double a_cur[C], b_cur[C], d_cur[C];
#pragma unroll
            for (int q = 0; q < C; ++q) { a_cur[q] = s_a[kl * C + q]; b_cur[q] = s_b[kl * C + q]; d_cur[q] = s_d[kl * C + q]; }
            unsigned long long pending = __ballot(valid);
            while (pending) {
                double xw[C], cand[C], an[C], dn[C];
#pragma unroll
                for (int a = 0; a < C; ++a) {
                    double t = s_s[kl * C + a];
#pragma unroll
                    for (int c2 = 0; c2 < C; ++c2) t = t + Mj[a][c2] * a_cur[c2];
                    xw[a] = t;
                }
                const int which = rrm_eval<C>(Mj, Gi, A.lpi, A.ie, xw, u, z, s_ld + lane, cand);
                bool ch = false;
#pragma unroll
                for (int q = 0; q < C; ++q) {
                    dn[q] = ((which >> q) & 1) ? 1.0 : 0.0;
                    an[q] = dn[q] * cand[q];
                    ch = ch || (an[q] != a_cur[q]);
                }
                const int kw = jwu::first_changed(ch && valid, pending);
                // lanes before the winner are final with what they just evaluated (their coefficients do not move)
                const unsigned long long done = jwu::final_lanes(pending, kw);
                if ((done >> lane) & 1ull) {
#pragma unroll
                    for (int q = 0; q < C; ++q) { b_cur[q] = cand[q]; d_cur[q] = dn[q]; }
                }
                if (kw >= 64) break;
                // the winner commits; its Gram row corrects s of the whole block: s_k += G_k,ce d
                const int ce = 64 * s + kw;
                double D[C];
#pragma unroll
                for (int q = 0; q < C; ++q) {
                    const double Dl = a_cur[q] - an[q];
                    D[q] = __shfl(Dl, kw, 64);
                    if (lane == kw) a_cur[q] = an[q];
                }
                const double* __restrict__ grow = A.gram + (int64_t)ce * bs * NC;
                for (int k2 = lane; k2 < b; k2 += 64) {
                    double g[NC];
#pragma unroll
                    for (int i = 0; i < NC; ++i) g[i] = grow[(int64_t)k2 * NC + i];
#pragma unroll
                    for (int a = 0; a < C; ++a) {
                        double t = s_s[k2 * C + a];
#pragma unroll
                        for (int c2 = 0; c2 < C; ++c2) t = t + g[cell(a, c2)] * D[c2];
                        s_s[k2 * C + a] = t;
                    }
                }
                pending &= ~done;
            }
            // the sub-block is final: state, change list, statistics
            bool changed = false;
            unsigned stv = 0u;
#pragma unroll
            for (int q = 0; q < C; ++q) {
                changed = changed || (a_cur[q] != s_a0[kl * C + q]);
                if (d_cur[q] != 0.0) stv |= 1u << q;
            }
            changed = changed && valid;
            const int e = jwu::list_entry(changed, lane, base);
            if (changed) {
                A.ev->idx[e] = (int32_t)(A.j0 + k);
#pragma unroll
                for (int q = 0; q < C; ++q) {
                    const double dd = s_a0[k * C + q] - a_cur[q];
                    A.ev->d[q][e] = dd;
                    s_dl[e * C + q] = dd;
                }
            }
            if (valid) {
#pragma unroll
                for (int q = 0; q < C; ++q) {
                    A.alpha[(int64_t)q * A.p + A.j0 + k] = a_cur[q];
                    A.beta[(int64_t)q * A.p + A.j0 + k] = b_cur[q];
                    A.delta[(int64_t)q * A.p + A.j0 + k] = d_cur[q];
                    st_acc[NC] = st_acc[NC] + a_cur[q] * a_cur[q];
#pragma unroll
                    for (int q2 = 0; q2 <= q; ++q2) st_acc[q * (q + 1) / 2 + q2] = st_acc[q * (q + 1) / 2 + q2] + b_cur[q] * b_cur[q2];
                }
#pragma unroll
                for (int i = 0; i < NS; ++i) cnt[i] = cnt[i] + ((unsigned)i == stv ? 1.0 : 0.0);
                if (changed) st_acc[NC + 1] = st_acc[NC + 1] + 1.0;
            }
        }
        // the block's statistics join the sweep's: shuffle tree, lane 0 adds (the blocks of a sweep run in stream order)
#pragma unroll
        for (int i = 0; i < NC + 2; ++i) st_acc[i] = jwu::wave_sum(st_acc[i]);
#pragma unroll
        for (int i = 0; i < NS; ++i) cnt[i] = jwu::wave_sum(cnt[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) A.stat[kStCounts + i] = A.stat[kStCounts + i] + cnt[i];
#pragma unroll
            for (int i = 0; i < NC; ++i) A.stat[kStBeta + i] = A.stat[kStBeta + i] + st_acc[i];
            A.stat[kStAlpha] = A.stat[kStAlpha] + st_acc[NC];
            A.stat[kStChanged] = A.stat[kStChanged] + st_acc[NC + 1];
            A.ev->count = base;
            s_count = base;
        }
    }
    __syncthreads();
    // g[e][t] = phi_t'd_e (q ascending from the first product): what the next launch applies
    const int total = s_count * A.T;
    for (int f = tid; f < total; f += 256) {
        const int e = f / A.T, t = f - e * A.T;
        double g = s_phi[t * C] * s_dl[e * C];
#pragma unroll
        for (int q = 1; q < C; ++q) g = g + s_phi[t * C + q] * s_dl[e * C + q];
        A.ev->g[f] = g;
    }
}

}  // namespace jwr
