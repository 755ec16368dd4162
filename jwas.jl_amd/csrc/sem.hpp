// sem.hpp -- structural equation models on the device: the recursive causal structure among the traits.
//
// The reference samples the structural coefficients between the residual-variance draw and the saved sample
// (MCMC/MCMC_BayesianAlphabet.jl:372-377, structure_equation_model/SEM.jl:124-165; Wang et al. 2020, G3).  t traits, n records,
// y (t x n, double, constant) the phenotypes, cs the strictly lower 0/1 causal structure (cs[i][j] = 1: trait j acts on trait i),
// P_i the parents of trait i ascending, lambda_i their coefficients.  The resident residual is the reference's "Lambda ycorr",
//   r_i = y_i - sum_{j in P_i} lambda_ij y_j - fitted_i,
// so the sweep, the location parameters and the variance draws run on it unchanged.  One step, for every trait i with parents
// (all arithmetic double, -ffp-contract=off):
//   S_jk  = y_j'y_k                                     formed once (k_sem_gram)
//   C_ji  = y_j'r_i               j in P_i              (k_sem_dots: the only O(n) reduction of a step)
//   rhs_q = (C_{P_q,i} + sum_m S_{P_q,P_m} lambda_old_m) / R_ii      m ascending, the sum starts from C
//   F_qm  = S_{P_q,P_m} / R_ii + (q == m)               the prior lambda ~ N(0, 1) (SEM.jl:134-138); only diag(R) (SEM.jl:129)
//   F = L L' (Cholesky, lower),  L w = rhs,  L' mu = w,  L' x = z,  lambda_new = mu + x
//   z_q = sqrt(-2 ln u1) cos(2 pi u2) on philox4x32_10(q, iteration, 0x04000000 | i, 7): u1 from words (1, 0), u2 from (3, 2)
//   r_i,n = T(((double(r_i,n) + d_1 y_j1,n) + d_2 y_j2,n) + ...)     d = lambda_old - lambda_new, parents ascending (k_sem_apply)
// The coefficient estimated from the column (i, j) of the design IS lambda_ij: the reference maps the drawn vector back in column
// order (tranform_lambda: findnz), which differs from the row order of its design from t = 4 on.
//
// ORDER OF EVERY SUM.  The records are cut into pieces of kPiece = 1024; the grid is G = min(ceil(n / 1024), 512) workgroups of 256
// threads, workgroup b takes pieces b, b + G, ...; a thread adds its records in ascending order, the 64 lanes of a wave meet in a
// shuffle tree (32 .. 1), the four waves are added in wave order through LDS, and ONE workgroup adds the G partials in ascending
// order.  No floating-point atomics: the order is a function of n alone, two runs give identical bits.
//
// Indirect and overall marker effects (compute_indirect_effect, SEM.jl:245-252): with K = sum_{m=1}^{t-1} Lambda^m from the host,
//   indirect_k = sum_j K[k][j] alpha_j (j ascending, from 0),  overall_k = alpha_k + indirect_k,
// and per marker and trait a running mean, mean of squares and frequency of non-zero of both (k_sem_accumulate).
//
// Matrices on the device are 4 x 4 row-major (stride kMaxT) whatever t.  Launch order is the only synchronisation between workgroups.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jws {

constexpr int kMaxT = 4;
constexpr int kMaxPairs = 6;            // strictly lower cells of a 4 x 4 matrix: cell(i, j) = i (i - 1) / 2 + j
constexpr int kGramCells = 10;          // lower cells with the diagonal: gcell(j, k) = j (j + 1) / 2 + k
constexpr int kPiece = 1024;
constexpr int kMaxGrid = 512;
constexpr uint32_t kTag = 0x04000000u;
constexpr uint32_t kSlot = 7u;
// the device record of a session: lambda | d | mu | C, 16 doubles each
constexpr int kRecLambda = 0, kRecD = 16, kRecMu = 32, kRecC = 48, kRecSize = 64;

__host__ __device__ constexpr int cell(int i, int j) { return i * (i - 1) / 2 + j; }
__host__ __device__ constexpr int gcell(int j, int k) { return j * (j + 1) / 2 + k; }

inline int sem_grid(int64_t n)
{
    const int64_t g = (n + kPiece - 1) / kPiece;
    return (int)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

struct DotArgs {
    const void* r;                      // [nt][ld] residuals (T)
    const double* y;                    // [nt][n]
    double* part;                       // [G][kMaxPairs]
    int64_t n, ld;
    uint32_t mask, ymask, rmask;        // bit cell(i, j): cs[i][j]; bit k: trait k is a parent / has parents
    int32_t nt;
};

// grid: sem_grid(n) workgroups of 256 threads
template <class T>
__global__ __launch_bounds__(256) void k_sem_dots(const DotArgs A)
{
    __shared__ double sh[4 * kMaxPairs];
    const T* __restrict__ r = (const T*)A.r;
    double acc[kMaxPairs];
#pragma unroll
    for (int q = 0; q < kMaxPairs; ++q) acc[q] = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * kPiece; base < A.n; base += (int64_t)gridDim.x * kPiece) {
#pragma unroll
        for (int q = 0; q < kPiece / 256; ++q) {
            const int64_t rec = base + q * 256 + threadIdx.x;
            if (rec >= A.n) continue;
            double yv[kMaxT], rv[kMaxT];
#pragma unroll
            for (int k = 0; k < kMaxT; ++k) {
                yv[k] = (k < A.nt && ((A.ymask >> k) & 1u)) ? A.y[(size_t)k * A.n + rec] : 0.0;
                rv[k] = (k < A.nt && ((A.rmask >> k) & 1u)) ? (double)r[(size_t)k * A.ld + rec] : 0.0;
            }
#pragma unroll
            for (int i = 1; i < kMaxT; ++i)
#pragma unroll
                for (int j = 0; j < i; ++j)
                    if ((A.mask >> cell(i, j)) & 1u) acc[cell(i, j)] = acc[cell(i, j)] + yv[j] * rv[i];
        }
    }
    jwu::block_reduce<kMaxPairs>(acc, sh, A.part + (size_t)blockIdx.x * kMaxPairs);
}

// S = y y' at begin: the same reduction over the cells (j, k), k <= j < nt; part: [G][kGramCells]
__global__ __launch_bounds__(256) void k_sem_gram(const double* __restrict__ y, int64_t n, int32_t nt, double* __restrict__ part)
{
    __shared__ double sh[4 * kGramCells];
    double acc[kGramCells];
#pragma unroll
    for (int q = 0; q < kGramCells; ++q) acc[q] = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * kPiece; base < n; base += (int64_t)gridDim.x * kPiece) {
#pragma unroll
        for (int q = 0; q < kPiece / 256; ++q) {
            const int64_t rec = base + q * 256 + threadIdx.x;
            if (rec >= n) continue;
            double yv[kMaxT];
#pragma unroll
            for (int k = 0; k < kMaxT; ++k) yv[k] = k < nt ? y[(size_t)k * n + rec] : 0.0;
#pragma unroll
            for (int j = 0; j < kMaxT; ++j)
#pragma unroll
                for (int k = 0; k <= j; ++k) acc[gcell(j, k)] = acc[gcell(j, k)] + yv[j] * yv[k];
        }
    }
    jwu::block_reduce<kGramCells>(acc, sh, part + (size_t)blockIdx.x * kGramCells);
}

// one workgroup of 64 threads: the G partials of every cell in ascending workgroup order, S symmetric 4 x 4
__global__ __launch_bounds__(64) void k_sem_gram_sum(const double* __restrict__ part, int32_t G, double* __restrict__ S)
{
    const int tid = threadIdx.x;
    if (tid >= 16) return;
    const int a = tid >> 2, b = tid & 3;
    const int cl = a >= b ? gcell(a, b) : gcell(b, a);
    double s = 0.0;
    for (int g = 0; g < G; ++g) s = s + part[(size_t)g * kGramCells + cl];
    S[tid] = s;
}

struct DrawArgs {
    const double* part;                 // [G][kMaxPairs]
    const double* S;                    // [16]
    double* rec;                        // [kRecSize]
    double Rdiag[kMaxT];
    int32_t G, nt;
    uint32_t mask, iter, seed_lo, seed_hi;
};

// one workgroup of 64 threads: lanes 0 .. 15 add the partials of their cell, then lane i < nt draws the coefficients of trait i
__global__ __launch_bounds__(64) void k_sem_draw(const DrawArgs A)
{
    __shared__ double C[16];
    const int tid = threadIdx.x;
    if (tid < 16) {
        const int i = tid >> 2, j = tid & 3;
        double s = 0.0;
        if (i > j && i < A.nt && ((A.mask >> cell(i, j)) & 1u)) {
            const int cl = cell(i, j);
            for (int g = 0; g < A.G; ++g) s = s + A.part[(size_t)g * kMaxPairs + cl];
        }
        C[tid] = s;
        A.rec[kRecC + tid] = s;
    }
    __syncthreads();
    if (tid >= A.nt) return;
    const int i = tid;
    // The at most M = 3 parents are compacted with selects and the system is padded to M x M with rows of the identity (rhs = z = 0
    // there): the factor and the solves of the leading k x k block are unchanged bit for bit (every padded product is an exact
    // zero), every loop has constant bounds and everything stays in registers.
    constexpr int M = kMaxT - 1;
    int P[M] = {0, 0, 0};
    int k = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        if (j < i && ((A.mask >> cell(i, j)) & 1u)) {
#pragma unroll
            for (int q = 0; q < M; ++q) P[q] = q == k ? j : P[q];
            ++k;
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxT; ++j) { A.rec[kRecD + i * kMaxT + j] = 0.0; A.rec[kRecMu + i * kMaxT + j] = 0.0; }
    if (k == 0) return;
    const double Rii = A.Rdiag[i];
    double F[M][M], L[M][M], rhs[M], old[M], w[M], mu[M], x[M], z[M];
#pragma unroll
    for (int q = 0; q < M; ++q) old[q] = q < k ? A.rec[kRecLambda + i * kMaxT + P[q]] : 0.0;
#pragma unroll
    for (int q = 0; q < M; ++q) {
        rhs[q] = 0.0; z[q] = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) { F[q][m] = q == m ? 1.0 : 0.0; L[q][m] = 0.0; }
        if (q < k) {
            double s = C[i * kMaxT + P[q]];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                if (m < k) {
                    const double Sqm = A.S[P[q] * kMaxT + P[m]];
                    s = s + Sqm * old[m];
                    F[q][m] = Sqm / Rii + (q == m ? 1.0 : 0.0);
                }
            }
            rhs[q] = s / Rii;
            const jw::u32x4 v = jw::philox4x32_10((uint32_t)q, A.iter, kTag | (uint32_t)i, kSlot, A.seed_lo, A.seed_hi);
            const double u1 = jw::u52(v.x, v.y), u2 = jw::u52(v.z, v.w);
            z[q] = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
        }
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            double s = F[a][b];
#pragma unroll
            for (int c = 0; c < b; ++c) s = s - L[a][c] * L[b][c];
            L[a][b] = a == b ? sqrt(s) : s / L[b][b];
        }
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
        double s = rhs[a];
#pragma unroll
        for (int c = 0; c < a; ++c) s = s - L[a][c] * w[c];
        w[a] = s / L[a][a];
    }
#pragma unroll
    for (int a = M - 1; a >= 0; --a) {
        double s = w[a], sz = z[a];
#pragma unroll
        for (int c = a + 1; c < M; ++c) { s = s - L[c][a] * mu[c]; sz = sz - L[c][a] * x[c]; }
        mu[a] = s / L[a][a];
        x[a] = sz / L[a][a];
    }
#pragma unroll
    for (int q = 0; q < M; ++q) {
        if (q < k) {
            const double now = mu[q] + x[q];
            A.rec[kRecLambda + i * kMaxT + P[q]] = now;
            A.rec[kRecD + i * kMaxT + P[q]] = old[q] - now;
            A.rec[kRecMu + i * kMaxT + P[q]] = mu[q];
        }
    }
}

struct ApplyArgs {
    void* r;                            // [nt][ld] residuals (T)
    const double* y;                    // [nt][n]
    const double* d;                    // [16] lambda_old - lambda_new
    int64_t n, ld;
    uint32_t mask, ymask, rmask;
    int32_t nt;
};

// one thread per record
template <class T>
__global__ __launch_bounds__(256) void k_sem_apply(const ApplyArgs A)
{
    const int64_t rec = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (rec >= A.n) return;
    T* __restrict__ r = (T*)A.r;
    double yv[kMaxT];
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) yv[k] = (k < A.nt && ((A.ymask >> k) & 1u)) ? A.y[(size_t)k * A.n + rec] : 0.0;
#pragma unroll
    for (int i = 1; i < kMaxT; ++i) {
        if (i >= A.nt || !((A.rmask >> i) & 1u)) continue;
        double v = (double)r[(size_t)i * A.ld + rec];
#pragma unroll
        for (int j = 0; j < i; ++j)
            if ((A.mask >> cell(i, j)) & 1u) v = v + A.d[i * kMaxT + j] * yv[j];
        r[(size_t)i * A.ld + rec] = (T)v;
    }
}

struct AccArgs {
    const void* alpha;                  // [nt][p] marker effects (T)
    double* acc;                        // [2 kinds][3: mean, mean of squares, frequency][nt][p]
    double K[kMaxT * kMaxT];
    double nsamples;
    int64_t p;
    int32_t nt;
};

__device__ __forceinline__ void sem_running(double* __restrict__ acc, size_t stat_stride, size_t at, double v, double ns)
{
    const double m = acc[at], m2 = acc[stat_stride + at], f = acc[2 * stat_stride + at];
    acc[at] = jwu::running_mean(m, v, ns);
    acc[stat_stride + at] = jwu::running_mean(m2, v * v, ns);
    acc[2 * stat_stride + at] = jwu::running_mean(f, v != 0.0 ? 1.0 : 0.0, ns);
}

// one thread per marker
template <class T>
__global__ __launch_bounds__(256) void k_sem_accumulate(const AccArgs A)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= A.p) return;
    const T* __restrict__ alpha = (const T*)A.alpha;
    double a[kMaxT];
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) a[k] = k < A.nt ? (double)alpha[(size_t)k * A.p + m] : 0.0;
    const size_t stat = (size_t)A.nt * A.p;
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) {
        if (k >= A.nt) continue;
        double ind = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxT; ++j)
            if (j < A.nt) ind = ind + A.K[k * kMaxT + j] * a[j];
        const size_t at = (size_t)k * A.p + m;
        sem_running(A.acc, stat, at, ind, A.nsamples);
        sem_running(A.acc + 3 * stat, stat, at, a[k] + ind, A.nsamples);
    }
}

}  // namespace jws
