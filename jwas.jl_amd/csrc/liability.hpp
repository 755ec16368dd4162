// liability.hpp -- threshold (binary / ordered categorical) and censored traits: the liabilities sampled on the device.
//
// The reference's step (categorical_and_censored_trait/categorical_and_censored_trait.jl:166-210, called from
// MCMC/MCMC_BayesianAlphabet.jl:186-191 before the location parameters) is per-individual work on the residual vector this
// library keeps resident: recover the current mean as liability - residual, redraw the residual from a normal truncated to the
// record's bounds (multi-trait: conditional on the other traits' residuals, nGibbs rounds), store liability and residual.
// One thread per individual; nothing couples individuals.
//
//   k_liability_sample<NT, T>   NT = 1..4 traits, T = float | double (the context's element type).  All arithmetic is double,
//                               the whole nGibbs x NT loop stays in registers, the new values are stored once (in T).
//                               Its tail leaves the per-workgroup min / max of every category of the traits that have free
//                               thresholds (:152-155), so a threshold update costs one more launch only.
//   k_liability_minmax<T>       the same partials on their own (when no draw preceded the request)
//   k_liability_minmax_reduce   one workgroup: the partials of all workgroups, in workgroup order
//
// THE TRUNCATED NORMAL is ONE counter uniform per draw and no rejection loop, so rng.hpp's contract (same seed => same chain,
// whatever the launch geometry) extends to it.  With lo < hi the standardised bounds and S(x) = erfc(x / sqrt 2) / 2:
//   lo + hi >= 0 (or NaN: both infinite)   q = S(lo) - u (S(lo) - S(hi)),  z = -Phi^-1(q) = sqrt 2 erfcinv(2 q)
//   otherwise                              the mirror image: the draw for (-hi, -lo), negated
//   S(lo) below the smallest normal double (lo beyond ~37.5)
//                                          z = lo - log1p(-u (1 - exp(-lo (hi - lo)))) / lo: the exponential tail, an
//                                          APPROXIMATION (relative error of the density ~ 1 / lo^2) that no real chain reaches;
//                                          it exists so that no input yields NaN or a liability outside its bounds
//   z is clamped into [lo, hi]; the liability is clamped into [L, U] after cmean + eps is rounded.
// The uniform: philox4x32_10(individual, iteration, 0x40000000 | Gibbs round, 2 + 16 * trait) -- see rng.hpp.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwl {

constexpr int kMaxCat = kMaxThr - 1;       // (kMaxT, kMaxThr: device_util.hpp; at most 15 categories)
constexpr int kMM = 2 * kMaxCat;        // doubles per workgroup and trait: {max, min} of every category

enum { kContinuous = 0, kCategorical = 1, kCensored = 2 };

struct LiabArgs {
    int64_t n, ld;
    void* r;                            // [nt][ld] residuals (T)
    void* y[kMaxT];                     // [n] liabilities (T); NULL for a continuous trait
    const int32_t* codes[kMaxT];        // categorical: category per record, 0 = missing
    const double* lower[kMaxT];         // censored: bounds per record
    const double* upper[kMaxT];
    const double* thr;                  // [kMaxT][kMaxThr] threshold tables
    double* part[kMaxT];                // [nworkgroups][kMM] min / max partials, NULL = none wanted
    int32_t kind[kMaxT], ncat[kMaxT];
    int32_t ngibbs, init;               // init: the set-up draw (:82-88): L == U stores the bound itself
    uint32_t iter, seed_lo, seed_hi;
    double B[kMaxT][kMaxT];             // row k: R_12 R_22^-1 of trait k against the others (B[k][k] = 0)
    double sd[kMaxT];                   // sqrt(R_11 - R_12 R_22^-1 R_21)
};

__device__ __forceinline__ double liab_uniform(uint32_t i, uint32_t iter, uint32_t round, uint32_t trait, uint32_t k0, uint32_t k1)
{
    const jw::u32x4 w = jw::philox4x32_10(i, iter, 0x40000000u | round, 2u + 16u * trait, k0, k1);
    return jw::u52(w.x, w.y);
}

// {max, min} of v over the records of every category 1..ncat of this workgroup (256 threads) -> out[2 (c - 1) + {0, 1}].
// max / min are exact, so the order of the combination does not show in the result.
__device__ __forceinline__ void block_minmax(int code, double v, int ncat, double* __restrict__ out, double* sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 1; c <= ncat; ++c) {
        double mx = code == c ? v : -INFINITY, mn = code == c ? v : INFINITY;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mx = fmax(mx, __shfl_xor(mx, off, 64));
            mn = fmin(mn, __shfl_xor(mn, off, 64));
        }
        if (lane == 0) { sh[wave] = mx; sh[4 + wave] = mn; }
        __syncthreads();
        if (threadIdx.x == 0) {
            out[2 * (c - 1)] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
            out[2 * (c - 1) + 1] = fmin(fmin(sh[4], sh[5]), fmin(sh[6], sh[7]));
        }
        __syncthreads();
    }
}

template <int NT, class T>
__global__ __launch_bounds__(256) void k_liability_sample(const LiabArgs A)
{
    __shared__ double sh[8];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < A.n;
    double r[NT], y[NT], cm[NT], L[NT], U[NT];
    int code[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        r[k] = valid ? (double)((const T*)A.r)[(size_t)k * A.ld + i] : 0.0;
        y[k] = 0.0; cm[k] = 0.0; L[k] = 0.0; U[k] = 0.0; code[k] = 0;
        if (A.kind[k] != kContinuous && valid) {
            y[k] = (double)((const T*)A.y[k])[i];
            cm[k] = y[k] - r[k];                                    // mean = liability - residual (:175)
            if (A.kind[k] == kCategorical) {
                code[k] = A.codes[k][i];
                const double* th = A.thr + k * kMaxThr;
                L[k] = code[k] ? th[code[k] - 1] : -INFINITY;      // (:115-121; 0 = missing: not truncated)
                U[k] = code[k] ? th[code[k]] : INFINITY;
            } else {
                L[k] = A.lower[k][i];
                U[k] = A.upper[k][i];
            }
        }
    }
    if (valid) {
        for (int round = 0; round < A.ngibbs; ++round) {
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                if (A.kind[k] == kContinuous) continue;
                if (L[k] == U[k]) {                                 // an exact record (:201); set-up: the bound itself (:86)
                    if (A.init) { y[k] = L[k]; r[k] = L[k] - cm[k]; }
                    continue;
                }
                double m = 0.0;
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (j != k) m = m + A.B[k][j] * r[j];
                const double s = A.sd[k];
                const double lo = ((L[k] - cm[k]) - m) / s, hi = ((U[k] - cm[k]) - m) / s;
                const double u = liab_uniform((uint32_t)i, A.iter, (uint32_t)round, (uint32_t)k, A.seed_lo, A.seed_hi);
                const double eps = m + s * jwu::truncated_std_normal(lo, hi, u);
                y[k] = fmin(fmax(cm[k] + eps, L[k]), U[k]);
                r[k] = eps;
            }
        }
#pragma unroll
        for (int k = 0; k < NT; ++k)
            if (A.kind[k] != kContinuous) {
                ((T*)A.y[k])[i] = (T)y[k];
                ((T*)A.r)[(size_t)k * A.ld + i] = (T)r[k];
            }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k)
        if (A.part[k])                                              // (uniform over the grid: every thread reaches the barriers)
            block_minmax(code[k], (double)(T)y[k], A.ncat[k], A.part[k] + (size_t)blockIdx.x * kMM, sh);
}

template <class T>
__global__ __launch_bounds__(256) void k_liability_minmax(const T* __restrict__ y, const int32_t* __restrict__ codes, int64_t n, int ncat,
                                                          double* __restrict__ part)
{
    __shared__ double sh[8];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    block_minmax(valid ? codes[i] : 0, valid ? (double)y[i] : 0.0, ncat, part + (size_t)blockIdx.x * kMM, sh);
}

// out[2 (c - 1) + {0, 1}] = {max, min} over the nparts workgroups; one workgroup of 256 threads
__global__ __launch_bounds__(256) void k_liability_minmax_reduce(const double* __restrict__ part, int nparts, int ncat, double* __restrict__ out)
{
    __shared__ double sh[256];
    for (int o = 0; o < 2 * ncat; ++o) {
        const bool is_min = o & 1;
        double v = is_min ? INFINITY : -INFINITY;
        for (int b = threadIdx.x; b < nparts; b += 256) {
            const double x = part[(size_t)b * kMM + o];
            v = is_min ? fmin(v, x) : fmax(v, x);
        }
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if ((int)threadIdx.x < w) sh[threadIdx.x] = is_min ? fmin(sh[threadIdx.x], sh[threadIdx.x + w]) : fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
            __syncthreads();
        }
        if (threadIdx.x == 0) out[o] = sh[0];
        __syncthreads();
    }
}

}  // namespace jwl
