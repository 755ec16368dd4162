// annot.hpp -- marker-annotation priors on the device: the probit update of the annotation coefficients from the resident delta.
//
// The reference regresses the inclusion indicators on marker annotations with a probit model between sweeps
// (MCMC/annotation_updates.jl:21-137,181-361) and feeds the per-marker prior back into the sweep.  A model has S steps; step s has
// an active set A_s and a binary response z (delta: the context's indicator, float | double, or the int32 class of BayesR):
//   BayesC         S = 1   all markers, z = delta != 0
//   BayesR         S = 3   delta > 1 on all;  delta > 2 on {delta > 1};  delta > 3 on {delta > 2}
//   2-trait tree   S = 3   d1 | d2 on all;    d1 & d2 on {d1 | d2};      d1 & ~d2 on {d1 ^ d2}      (d_k = delta_k != 0)
// The design matrix is p x K with an intercept column of ones; the device keeps the K - 1 other columns column-major ([K - 1][p]),
// so a lane reads consecutive markers.  All arithmetic is double, -ffp-contract=off.  Step s, with its coefficients c_0 .. c_K-1:
//   (a) mu_i = c_0 + sum_{k >= 1} D_ik c_k                        k ascending, multiply then add
//   (b) i in A_s:  u = u52(philox4x32_10(i, iteration, 0x08000000 | s, 5)),
//                  e_i = truncated_std_normal(lo, hi, u)  (device_util.hpp),  (lo, hi) = (-mu_i, +Inf) if z_i, (-Inf, -mu_i) otherwise,
//                  liability_i = mu_i + e_i, forced onto its side of 0 (max(., 0) if z_i, min(., 0) otherwise)
//       i not in A_s:  e_i = 0, the stored liability is kept
//   (c) the coefficient scan in residual-update form, k = 0 .. K - 1 in order.  n_A = |A_s|, S_k = sum_A D_ik e_i,
//       d_k = sum_A D_ik^2 (D_i0 = 1, d_0 = n_A):
//         inv_k = 1 / (d_k + 1 / var_s),  inv_0 = 1 / n_A          (a flat prior on the intercept)
//         c_k'  = inv_k (S_k + d_k c_k) + z_k sqrt(inv_k)          z_k: Box-Muller as rng.hpp slot 1 on philox4x32_10(k, iteration, 0x08000000 | s, 6)
//         e_i  += D_ik (c_k - c_k')  on A_s
//   (d) n_A = 0: (b) and (c) do nothing, the coefficients of the step stay
//   (e) mu again from the new coefficients, P_s,i = clip(Phi(mu_i), eps, 1 - eps), Phi(x) = erfc(-x / sqrt 2) / 2, eps = 2^-52
// and after the last step the table the sweep reads (annotation_updates.jl:181-194,337-361):
//   BayesC   pi_vec[i]  = clip(1 - Phi(mu_i), eps, 1 - eps)
//   BayesR   pi_mat[i]  = {1 - P1, P1 (1 - P2), (P1 P2) (1 - P3), (P1 P2) P3}
//   tree     lpr_mat[i] = log {1 - P1, (P1 (1 - P2)) P3, (P1 (1 - P2)) (1 - P3), P1 P2}        (states 00, 10, 01, 11)
//
// ORDER OF EVERY SUM.  The markers are cut into pieces of kPiece = 1024 consecutive markers, one workgroup of 256 threads each:
// thread j adds markers j, j + 256, j + 512, j + 768 of its piece in that order, the 256 partial sums meet in a fixed tree
// (128 .. 1).  The piece sums are added by ONE workgroup: thread j adds pieces j, j + 256, ... in that order, then the same tree.
// No floating-point atomics; the order is a function of p only, two runs give identical bits.
//
// LAUNCHES.  Launch order is the only synchronisation between workgroups.  The axpy of coefficient k rides in the reduction pass
// of coefficient k + 1 (the one of the last coefficient is never read and is not made), so a coefficient costs one streaming
// launch and one one-workgroup launch:
//   k_annot_liab<DT, KIND>    (a), (b) and the piece sums of coefficient 0 (S_0, n_A)
//   k_annot_sums<DT, KIND>    e += D_k-1 (c_k-1 - c_k-1'), then the piece sums of S_k (and of d_k unless A_s is all markers: then
//                             d_k comes from set-up, k_annot_colsq)
//   k_annot_draw              one workgroup: the piece sums in piece order, the draw, c_k - c_k' left for the next pass
//   k_annot_table<KIND>       (e) for every step, the table, the piece sums of its columns
//   k_annot_colmeans          one workgroup: the column means
//   k_annot_accumulate        running mean and mean of squares of the per-marker prior (output.jl:597-601's form)
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwa {

constexpr int kPiece = 1024;
constexpr int kMaxCols = 64;            // columns of the design matrix, the intercept included
constexpr int kMaxSteps = 3;
constexpr uint32_t kTag = 0x08000000u;
constexpr double kEps = 0x1.0p-52;

// (the kinds kBayesC, kBayesR, kTree: device_util.hpp)

__host__ __device__ inline int annot_nsteps(int kind) { return kind == kBayesC ? 1 : 3; }

template <class DT, int KIND>
__device__ __forceinline__ void annot_response(const DT* __restrict__ d1, const DT* __restrict__ d2, int64_t i, int s, bool& act, bool& z)
{
    if constexpr (KIND == kBayesC) {
        act = true; z = d1[i] != (DT)0;
    } else if constexpr (KIND == kBayesR) {
        const int cl = (int)d1[i];
        act = s == 0 || cl > s; z = cl > s + 1;
    } else {
        const bool a = d1[i] != (DT)0, b = d2[i] != (DT)0;
        if (s == 0) { act = true; z = a || b; }
        else if (s == 1) { act = a || b; z = a && b; }
        else { act = a != b; z = a && !b; }
    }
}

struct StepArgs {
    const void *d1, *d2;                // [p] the indicators (d2: the tree's second trait)
    const double* D;                    // [K - 1][p]
    const double* coef;                 // [K] of this step
    double* liab;                       // [p] of this step
    double* e;                          // [p]
    double* part;                       // [npieces][3]: S, d, n_A
    const double* dc;                   // c_k-1 - c_k-1' of the previous draw (k_annot_sums)
    int64_t p;
    int32_t K, s, k, all_active;
    uint32_t iter, seed_lo, seed_hi;
};

__device__ __forceinline__ double annot_mu(const double* __restrict__ D, const double* __restrict__ coef, int K, int64_t p, int64_t i)
{
    double mu = coef[0];
    for (int k = 1; k < K; ++k) mu = mu + D[(size_t)(k - 1) * p + i] * coef[k];
    return mu;
}

// grid: npieces workgroups of 256 threads
template <class DT, int KIND>
__global__ __launch_bounds__(256) void k_annot_liab(const StepArgs A)
{
    __shared__ double sh[256];
    const int64_t base = (int64_t)blockIdx.x * kPiece;
    double S = 0.0, cnt = 0.0;
    for (int q = 0; q < kPiece / 256; ++q) {
        const int64_t i = base + q * 256 + threadIdx.x;
        if (i >= A.p) break;
        bool act, z;
        annot_response<DT, KIND>((const DT*)A.d1, (const DT*)A.d2, i, A.s, act, z);
        double e = 0.0;
        if (act) {
            const double mu = annot_mu(A.D, A.coef, A.K, A.p, i);
            const jw::u32x4 w = jw::philox4x32_10((uint32_t)i, A.iter, kTag | (uint32_t)A.s, 5u, A.seed_lo, A.seed_hi);
            const double u = jw::u52(w.x, w.y);
            e = jwu::truncated_std_normal(z ? -mu : -INFINITY, z ? INFINITY : -mu, u);
            const double l = mu + e;
            A.liab[i] = z ? fmax(l, 0.0) : fmin(l, 0.0);
            S = S + e;
            cnt = cnt + 1.0;
        }
        A.e[i] = e;
    }
    const double St = jwu::tree256(sh, S), ct = jwu::tree256(sh, cnt);
    if (threadIdx.x == 0) { A.part[(size_t)blockIdx.x * 3] = St; A.part[(size_t)blockIdx.x * 3 + 2] = ct; }
}

// coefficient k >= 1: the axpy of coefficient k - 1, then the piece sums of S_k and d_k
template <class DT, int KIND>
__global__ __launch_bounds__(256) void k_annot_sums(const StepArgs A)
{
    __shared__ double sh[256];
    const int64_t base = (int64_t)blockIdx.x * kPiece;
    const double dc = *A.dc;
    const double* __restrict__ Dprev = A.k >= 2 ? A.D + (size_t)(A.k - 2) * A.p : nullptr;      // (column 0 is the ones)
    const double* __restrict__ Dk = A.D + (size_t)(A.k - 1) * A.p;
    double S = 0.0, d = 0.0;
    for (int q = 0; q < kPiece / 256; ++q) {
        const int64_t i = base + q * 256 + threadIdx.x;
        if (i >= A.p) break;
        bool act, z;
        annot_response<DT, KIND>((const DT*)A.d1, (const DT*)A.d2, i, A.s, act, z);
        if (!act) continue;
        const double e = A.e[i] + (Dprev ? Dprev[i] : 1.0) * dc;
        A.e[i] = e;
        const double x = Dk[i];
        S = S + x * e;
        d = d + x * x;
    }
    const double St = jwu::tree256(sh, S);
    if (threadIdx.x == 0) A.part[(size_t)blockIdx.x * 3] = St;
    if (!A.all_active) {                                                    // (uniform)
        const double dt = jwu::tree256(sh, d);
        if (threadIdx.x == 0) A.part[(size_t)blockIdx.x * 3 + 1] = dt;
    }
}

struct DrawArgs {
    const double* part;                 // [npieces][3]
    const double* dsq;                  // [K] d_k over all markers (set-up)
    double* coef;                       // [K] of this step
    double* nA;                         // this step's n_A (written at k == 0)
    double* dc;                         // out: c_k - c_k'
    double var;
    int32_t npieces, k, s, all_active;
    uint32_t iter, seed_lo, seed_hi;
};

// one workgroup of 256 threads
__global__ __launch_bounds__(256) void k_annot_draw(const DrawArgs A)
{
    __shared__ double sh[256];
    const double S = jwu::ordered_sum256(sh, A.part, 3, A.npieces);
    double d, cnt;
    if (A.k == 0) {
        cnt = jwu::ordered_sum256(sh, A.part + 2, 3, A.npieces);
        d = cnt;
    } else {
        cnt = *A.nA;
        d = A.all_active ? A.dsq[A.k] : jwu::ordered_sum256(sh, A.part + 1, 3, A.npieces);       // (uniform)
    }
    if (threadIdx.x != 0) return;
    if (A.k == 0) *A.nA = cnt;
    if (cnt == 0.0) { *A.dc = 0.0; return; }                                // (d): the coefficients stay
    const double inv = A.k == 0 ? 1.0 / cnt : 1.0 / (d + 1.0 / A.var);
    const double old = A.coef[A.k];
    const jw::u32x4 w = jw::philox4x32_10((uint32_t)A.k, A.iter, kTag | (uint32_t)A.s, 6u, A.seed_lo, A.seed_hi);
    const double u1 = jw::u52(w.x, w.y), u2 = jw::u52(w.z, w.w);
    const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
    const double now = inv * (S + d * old) + z * sqrt(inv);
    A.coef[A.k] = now;
    *A.dc = old - now;
}

// set-up: piece sums of D_ik^2 over all markers; grid (npieces, K - 1), out[(k - 1) npieces + piece]
__global__ __launch_bounds__(256) void k_annot_colsq(const double* __restrict__ D, int64_t p, int32_t npieces, double* __restrict__ out)
{
    __shared__ double sh[256];
    const double* __restrict__ Dk = D + (size_t)blockIdx.y * p;
    const int64_t base = (int64_t)blockIdx.x * kPiece;
    double d = 0.0;
    for (int q = 0; q < kPiece / 256; ++q) {
        const int64_t i = base + q * 256 + threadIdx.x;
        if (i >= p) break;
        d = d + Dk[i] * Dk[i];
    }
    const double dt = jwu::tree256(sh, d);
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * npieces + blockIdx.x] = dt;
}

// grid: K - 1 workgroups; dsq[k] for k = blockIdx.x + 1
__global__ __launch_bounds__(256) void k_annot_colsq_reduce(const double* __restrict__ part, int32_t npieces, double* __restrict__ dsq)
{
    __shared__ double sh[256];
    const double tot = jwu::ordered_sum256(sh, part + (size_t)blockIdx.x * npieces, 1, npieces);
    if (threadIdx.x == 0) dsq[blockIdx.x + 1] = tot;
}

struct TableArgs {
    const double* D;                    // [K - 1][p]
    const double* coef;                 // [nsteps][K]
    double* mu;                         // [nsteps][p]
    double* table;                      // pi_vec [p] | pi_mat [p][4] | lpr_mat [p][4]
    double* part;                       // [npieces][4] piece sums of the columns (the probabilities, not their logs)
    int64_t p;
    int32_t K;
};

__device__ __forceinline__ double annot_clip(double v) { return fmin(fmax(v, kEps), 1.0 - kEps); }

// grid: npieces workgroups of 256 threads
template <int KIND>
__global__ __launch_bounds__(256) void k_annot_table(const TableArgs A)
{
    __shared__ double sh[256];
    constexpr int NS = KIND == kBayesC ? 1 : 3;
    constexpr int NC = KIND == kBayesC ? 1 : 4;
    const int64_t base = (int64_t)blockIdx.x * kPiece;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    for (int q = 0; q < kPiece / 256; ++q) {
        const int64_t i = base + q * 256 + threadIdx.x;
        if (i >= A.p) break;
        double P[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double mu = annot_mu(A.D, A.coef + (size_t)s * A.K, A.K, A.p, i);
            A.mu[(size_t)s * A.p + i] = mu;
            P[s] = jwu::upper_tail(-mu);                                    // Phi(mu)
        }
        if constexpr (KIND == kBayesC) {
            const double pi = annot_clip(1.0 - P[0]);
            A.table[i] = pi;
            acc[0] = acc[0] + pi;
        } else {
            const double p1 = annot_clip(P[0]), p2 = annot_clip(P[1]), p3 = annot_clip(P[2]);
            double row[4];
            if constexpr (KIND == kBayesR) {
                row[0] = 1.0 - p1; row[1] = p1 * (1.0 - p2); row[2] = (p1 * p2) * (1.0 - p3); row[3] = (p1 * p2) * p3;
            } else {
                row[0] = 1.0 - p1; row[1] = (p1 * (1.0 - p2)) * p3; row[2] = (p1 * (1.0 - p2)) * (1.0 - p3); row[3] = p1 * p2;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                A.table[(size_t)i * 4 + c] = KIND == kTree ? log(row[c]) : row[c];
                acc[c] = acc[c] + row[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double tot = jwu::tree256(sh, acc[c]);
        if (threadIdx.x == 0) A.part[(size_t)blockIdx.x * 4 + c] = tot;
    }
}

// one workgroup: means[c] = (the piece sums of column c in piece order) / p
__global__ __launch_bounds__(256) void k_annot_colmeans(const double* __restrict__ part, int32_t npieces, int32_t ncols, double p, double* __restrict__ means)
{
    __shared__ double sh[256];
    for (int c = 0; c < ncols; ++c) {
        const double tot = jwu::ordered_sum256(sh, part + c, 4, npieces);
        if (threadIdx.x == 0) means[c] = tot / p;
    }
}

// running mean and mean of squares of the per-marker prior; is_log: the table holds logs (the tree), the probabilities are exp(.)
__global__ __launch_bounds__(256) void k_annot_accumulate(const double* __restrict__ table, double* __restrict__ mean, double* __restrict__ mean2,
                                                          int64_t q, double nsamples, int32_t is_log)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= q) return;
    const double v = is_log ? exp(table[i]) : table[i];
    mean[i] = jwu::running_mean(mean[i], v, nsamples);
    mean2[i] = jwu::running_mean(mean2[i], v * v, nsamples);
}

}  // namespace jwa
