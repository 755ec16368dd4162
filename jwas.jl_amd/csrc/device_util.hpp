// device_util.hpp -- what the session kernels (liability.hpp, locpar.hpp, mtmiss.hpp, annot.hpp, sem.hpp, rrm.hpp, mega.hpp, gblup.hpp,
// marker_state.hpp) share.  It defines no kernel, so any number of units may include it; the host context (ctx.hpp) includes it for
// the limits below.  Every helper fixes an ORDER of floating-point operations: with -ffp-contract=off its callers compute the bits
// of the expression written out.
#pragma once
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- limits and codes that the host context and the kernels of a session both read ----------------------------------------------
namespace jwl { constexpr int kMaxT = 4; constexpr int kMaxThr = 16; }   // liabilities: traits; thresholds per trait, -Inf and +Inf included
namespace jwp { constexpr int kMaxT = 4; constexpr int kMaxGroups = 8; } // location parameters: member terms / random effects per model
namespace jwm { constexpr int kMaxT = jwp::kMaxT; constexpr int kMaxCodes = 1 << kMaxT; }      // missing traits: observation patterns
namespace jwa { enum { kBayesC = 0, kBayesR = 1, kTree = 2 }; }          // annotation priors: the kind of a session

namespace jwu {

// rng.hpp's Box-Muller normal from the four words of one Philox block: u1 from words (1, 0), u2 from (3, 2).  (k_locpar_draw, k_annot_draw,
// k_mtmiss_impute and k_sem_draw keep the expression in their bodies: behind this call the same bits cost them 2 .. 8 more VGPRs.)
__device__ __forceinline__ double normal_from(const jw::u32x4 w)
{
    const double u1 = jw::u52(w.x, w.y), u2 = jw::u52(w.z, w.w);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}

// the 256 values of a workgroup in a fixed tree (128 .. 1); every thread returns the total.  sh: 256 doubles of LDS
__device__ inline double tree256(double* sh, double v)
{
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

// part[0], part[stride], ... (n of them): thread j adds entries j, j + 256, ... in that order, then the tree
__device__ inline double ordered_sum256(double* sh, const double* __restrict__ part, int stride, int n)
{
    double acc = 0.0;
    for (int q = threadIdx.x; q < n; q += 256) acc = acc + part[(size_t)q * stride];
    return tree256(sh, acc);
}

// the mean of ns values from the mean m of the first ns - 1 and the last value v (output.jl:556-560's form)
__device__ __forceinline__ double running_mean(double m, double v, double ns) { return m + (v - m) / ns; }

// a wave's sum by the shuffle tree (32 .. 1): lane 0 holds the total
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// acc[0 .. N) of the 256 threads of a workgroup -> out[0 .. N): shuffle tree (32 .. 1) within a wave, the four waves in wave order,
// ((w0 + w1) + w2) + w3.  sh: 4 N doubles of LDS; the caller separates two uses with a barrier.
template <int N>
__device__ __forceinline__ void block_reduce(const double (&acc)[N], double* sh, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0) sh[wave * N + q] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) out[threadIdx.x] = ((sh[threadIdx.x] + sh[N + threadIdx.x]) + sh[2 * N + threadIdx.x]) + sh[3 * N + threadIdx.x];
}

// four consecutive rows of a column as doubles (the column starts on a 16-byte boundary: ld is a multiple of 256)
__device__ __forceinline__ void load4(const float* __restrict__ x, double (&v)[4])
{
    const float4 f = *reinterpret_cast<const float4*>(x);
    v[0] = (double)f.x; v[1] = (double)f.y; v[2] = (double)f.z; v[3] = (double)f.w;
}
__device__ __forceinline__ void load4(const double* __restrict__ x, double (&v)[4])
{
    const double2 a = *reinterpret_cast<const double2*>(x), b = *reinterpret_cast<const double2*>(x + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// lower Cholesky factor of an SPD N x N matrix, row by row: L_ab = (A_ab - sum_{k < b} L_ak L_bk, k ascending) / L_bb, the diagonal a
// square root (the operation order of sampler_mt.hpp's chol_lower, which the main sweep keeps for itself)
template <int N>
__device__ __forceinline__ void chol_lower(const double (&A)[N][N], double (&L)[N][N])
{
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) L[a][b] = 0.0;
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            double s = A[a][b];
#pragma unroll
            for (int k = 0; k < b; ++k) s = s - L[a][k] * L[b][k];
            L[a][b] = a == b ? sqrt(s) : s / L[b][b];
        }
    }
}

// ---- the speculative walk of a block by one wave (mega.hpp, rrm.hpp): every pending lane evaluates its marker, the first whose effect
// changes wins and commits ---------------------------------------------------------------------------------------------------------
// the first pending lane that voted `changed` (64: none)
__device__ __forceinline__ int first_changed(bool changed, unsigned long long pending)
{
    const unsigned long long mm = __ballot(changed) & pending;
    return mm ? (int)__builtin_ctzll(mm) : 64;
}

// the pending lanes up to and including the winner kw: final with what they just evaluated (kw = 64: all of them)
__device__ __forceinline__ unsigned long long final_lanes(unsigned long long pending, int kw)
{
    return (kw >= 64) ? pending : (pending & ((kw == 63) ? ~0ull : ((2ull << kw) - 1ull)));
}

// the change list's entry of this lane: base + the changed lanes below it; base advances by the wave's changed lanes
__device__ __forceinline__ int list_entry(bool changed, int lane, int& base)
{
    const unsigned long long cm = __ballot(changed);
    const int e = base + __popcll(cm & ((1ull << lane) - 1ull));
    base += __popcll(cm);
    return e;
}

// ---- the truncated standard normal of liability.hpp (its header comment has the cases) -------------------------------------------
__device__ __forceinline__ double upper_tail(double x) { return 0.5 * erfc(x * 0.70710678118654752440); }

// standard normal truncated to [lo, hi], lo < hi, from one uniform u in (0, 1); lo + hi >= 0 (or NaN)
__device__ __forceinline__ double tn_upper(double lo, double hi, double u)
{
    const double a = upper_tail(lo);
    double z;
    if (a >= 2.2250738585072014e-308) {
        const double b = upper_tail(hi);
        const double q = fmax(a - u * (a - b), 4.9406564584124654e-324);       // (u (a - b) may round to a: never q = 0, z = Inf)
        z = 1.41421356237309504880 * erfcinv(2.0 * q);
    } else {
        z = lo - log1p(-u * (1.0 - exp(-lo * (hi - lo)))) / lo;
    }
    return fmin(fmax(z, lo), hi);
}

// (not inlined: ONE copy of erfc / erfcinv / log1p / exp in the kernel instead of one per trait of the unrolled loop -- inlined,
// every instantiation of k_liability_sample took all 256 VGPRs and NT >= 3 spilled)
__device__ __noinline__ double truncated_std_normal(double lo, double hi, double u)
{
    const bool mirror = lo + hi < 0.0;
    const double z = tn_upper(mirror ? -hi : lo, mirror ? -lo : hi, u);
    return mirror ? -z : z;
}

}  // namespace jwu
