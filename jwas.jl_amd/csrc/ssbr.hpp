// ssbr.hpp -- single-step analysis on the device: the imputation of the non-genotyped individuals' genotypes,
//
//     A^nn M_n = -A^ng M_g                       (impute_genotypes, single_step/SSBR.jl:83-142; make_JVecs, :146-159)
//
// as a sparse solve with many right-hand sides.  A^nn (n_n x n_n, sparse, symmetric positive definite) is factorised ONCE on the host
// (SuperLU: Pr A^nn Pc = L U); the device holds L and U as CSR with ascending columns (L with its unit diagonal as the last entry of
// every row, U with its diagonal as the first), A^ng as CSR, and two permutation vectors: rsrc[r] = the row of A^nn whose right-hand
// side sits at position r of the permuted system (the inverse of perm_r) and perm_c (x[i] = z[perm_c[i]]).  Nothing in the kernels
// assumes symmetric-mode pivoting: they solve with whatever L, U and permutations they are handed.
//
// LAYOUT (markers of the running chunk along the fast axis, all double):
//   Gt[g][ldc]     the genotyped block M_g of the chunk, transposed: row k = genotyped individual k (pedigree order), column = marker
//   W [n_n][ldc]   the solve's work matrix, row = position in the permuted system; after the solve row perm_c[i] is M_n[i, chunk]
// so the entries of one row for neighbouring markers are contiguous: the 64 lanes of a wave, one marker each, read and write 512
// contiguous bytes per row.
//
// k_ss_stage    the uploaded g x count block (column-major, the context's element type or double) -> Gt, through a 32 x 33 LDS tile.
// k_ss_solve    ONE THREAD PER MARKER COLUMN.  The thread walks the rows of L top-down -- the right-hand side element
//               -sum_k A^ng[rsrc[r], k] Gt[k][col] is formed on the fly at the row's forward step -- and then the rows of U bottom-up,
//               in place in its own column of W.  Row entries are taken in ascending column order with explicit fma, so the result
//               of a column depends on nothing but that column: not on the chunk size, the grid or the workgroup size.  The sparse
//               indices and values are the same for every lane (plain loads from wave-uniform addresses); the W / Gt accesses are
//               coalesced across lanes.
// k_ss_scatter  rows [M_n; M_g][prow[r]] of the chunk -> columns [j0, j0 + count) of a marker-major matrix [p][ld] in the target's
//               element type, through a 32 x 33 LDS tile (read along markers, written along rows).  A non-genotyped row is row
//               perm_c[prow[r]] of W, a genotyped row is row prow[r] - n_n of Gt.  The cast to Float32 is the reference's
//               data_type.(Mpheno) (SSBR.jl:137-138).  Rows [nrows, ld) of those columns are written as zero.
//
// WHY THE SOLVE CANNOT HANG.  A thread of k_ss_solve reads from W only what it wrote itself (its own column), and from Gt and the
// factors only what earlier launches on the same stream wrote.  There are no barriers between workgroups, no barriers at all in the
// solve, no atomics, no flags, no waits and no spin loops; every loop runs over a range fixed by the (validated) CSR row pointers.
// The two tile kernels use __syncthreads() outside any divergent branch.  No kernel uses scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jws {

constexpr int kTile = 32;                       // the LDS tile of the two transposes
constexpr int kTileRows = 8;                    // ... walked by 32 x 8 threads
constexpr int kSolveThreads = 64;               // one wave per workgroup: the chunk's columns spread over the CUs
constexpr int kChunkGranule = 64;               // ldc is a multiple of this
constexpr int64_t kMaxChunk = 65536;            // ... and at most this

struct SolveArgs {
    const int64_t *Lp, *Up, *Ap;                // [n_n + 1] row pointers
    const int32_t *Lc, *Uc, *Ac;                // columns, ascending within a row
    const double *Lv, *Uv, *Av;
    const int32_t* rsrc;                        // [n_n] inverse of perm_r
    const double* Gt;                           // [g][ldc]
    double* W;                                  // [n_n][ldc]
    int64_t nn, ldc;
    int32_t count;
};

// in: [count][ldin] (individual k fastest) -> Gt[k ldc + j]
template <class T>
__global__ __launch_bounds__(kTile * kTileRows) void k_ss_stage(const T* __restrict__ in, int64_t ldin, int64_t g, int32_t count, double* __restrict__ Gt, int64_t ldc)
{
    __shared__ double tile[kTile][kTile + 1];
    const int64_t k0 = (int64_t)blockIdx.x * kTile, j0 = (int64_t)blockIdx.y * kTile;
    for (int i = threadIdx.y; i < kTile; i += kTileRows) {
        const int64_t k = k0 + threadIdx.x, j = j0 + i;
        tile[i][threadIdx.x] = (k < g && j < count) ? (double)in[j * ldin + k] : 0.0;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < kTile; i += kTileRows) {
        const int64_t k = k0 + i, j = j0 + threadIdx.x;
        if (k < g && j < count) Gt[k * ldc + j] = tile[threadIdx.x][i];
    }
}

__global__ __launch_bounds__(kSolveThreads) void k_ss_solve(SolveArgs a)
{
    const int64_t col = (int64_t)blockIdx.x * kSolveThreads + threadIdx.x;
    if (col >= a.count) return;
    const double* __restrict__ gt = a.Gt + col;
    double* w = a.W + col;
    const int64_t ldc = a.ldc;
    for (int64_t r = 0; r < a.nn; ++r) {                        // L y = Pr b, b formed on the fly
        const int64_t src = a.rsrc[r];
        double acc = 0.0;
        for (int64_t e = a.Ap[src], e1 = a.Ap[src + 1]; e < e1; ++e) acc = fma(-a.Av[e], gt[(int64_t)a.Ac[e] * ldc], acc);
        for (int64_t e = a.Lp[r], e1 = a.Lp[r + 1] - 1; e < e1; ++e) acc = fma(-a.Lv[e], w[(int64_t)a.Lc[e] * ldc], acc);      // (the last entry: the unit diagonal)
        w[r * ldc] = acc;
    }
    for (int64_t r = a.nn - 1; r >= 0; --r) {                   // U z = y
        const int64_t e0 = a.Up[r];
        double acc = w[r * ldc];
        for (int64_t e = e0 + 1, e1 = a.Up[r + 1]; e < e1; ++e) acc = fma(-a.Uv[e], w[(int64_t)a.Uc[e] * ldc], acc);
        w[r * ldc] = acc / a.Uv[e0];                            // (the first entry: the diagonal)
    }
}

// out[(j0 + j) ld + r] = [M_n; M_g][prow[r]][j] for r < nrows, 0 for nrows <= r < ld;  j < count
template <class T>
__global__ __launch_bounds__(kTile * kTileRows) void k_ss_scatter(const double* __restrict__ W, const double* __restrict__ Gt, int64_t ldc, int64_t nn,
                                                                  const int32_t* __restrict__ perm_c, const int32_t* __restrict__ prow, int64_t nrows,
                                                                  int32_t count, T* __restrict__ out, int64_t ld, int64_t j0)
{
    __shared__ double tile[kTile][kTile + 1];
    const int64_t r0 = (int64_t)blockIdx.x * kTile, c0 = (int64_t)blockIdx.y * kTile;
    for (int i = threadIdx.y; i < kTile; i += kTileRows) {
        const int64_t r = r0 + i, j = c0 + threadIdx.x;
        double v = 0.0;
        if (r < nrows && j < count) {
            const int64_t at = prow[r];
            v = at < nn ? W[(int64_t)perm_c[at] * ldc + j] : Gt[(at - nn) * ldc + j];
        }
        tile[i][threadIdx.x] = v;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < kTile; i += kTileRows) {
        const int64_t r = r0 + threadIdx.x, j = c0 + i;
        if (r < ld && j < count) out[(j0 + j) * ld + r] = (T)tile[threadIdx.x][i];
    }
}

}  // namespace jws
