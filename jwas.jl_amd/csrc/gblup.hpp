// gblup.hpp -- GBLUP on the device: the genomic relationship matrix and the sampler on pseudo-markers
// (markers/readgenotypes.jl:403-408, markers/BayesianAlphabet/GBLUP.jl).
//
// THE RELATIONSHIP MATRIX.  X the context's dense n x p matrix ([p][ld], marker-major, pad rows 0), d_j = sqrt(2 p_j (1 - p_j)) from
// the host in the matrix's precision:   Z = X ./ d,   K = (Z Z' + 1e-5 I) / p   (+ 1e-5 and / p in the matrix's precision).
//   k_grm<real>   one workgroup (4 waves, 2 x 2) per output tile ON OR BELOW the diagonal; the mirror is written from the same
//                 registers, so K == K' bit for bit.  Both operands are row panels of X: for a marker the rows are contiguous, so a
//                 panel is staged with coalesced 16-byte loads into LDS [marker][row] (the division by d_j applied on the way) and a
//                 lane's MFMA operand -- row lane & 31 (& 15), marker lane >> 5 (>> 4) -- is one conflict-free LDS word.
//                 float:  128 x 128 tiles, a wave owns 64 x 64 (2 x 2 v_mfma_f32_32x32x2_f32: a marker-ordered fp32 fma chain); the
//                         fp32 accumulators are folded into doubles every kGrmChunk markers.
//                 double: 64 x 64 tiles, a wave owns 32 x 32 (2 x 2 v_mfma_f64_16x16x4_f64), accumulated in double throughout.
//   k_grm_packed  k_grm<float> on 2-bit packed storage: the same tiles, chain, fold and store, hence the same bits as the dense kernel on
//                 the decoded columns; a panel is staged from one payload byte per thread and marker, the four possible x / d_j of a
//                 marker divided once per workgroup.
//
// THE SAMPLER.  L = the context's dense n x n matrix (column i the i-th eigenvector of K), D its eigenvalues; pseudo-marker i has
// the prior variance D_i G.  One step on the context's own residual r_k and effects alpha_k, k < T <= 4 traits (GBLUP!, megaGBLUP!,
// MTGBLUP!), L read once per pass for all traits:
//   pass 1   r+_k = r_k + L alpha_k                 k_gblup_mul (column parts) + k_gblup_add
//   pass 2   s_ik = l_i' r+_k                       k_gblup_rhs: one wave per column
//   sampler  diagonal (T = 1 or constraint = true): lhs = 1 + vare_kk / (G_kk D_i), alpha_ik = s_ik / lhs + z sqrt(vare_kk / lhs)
//            joint: lhs_i = R^-1 + G^-1 / D_i, S = inv(lhs_i), mu = S (R^-1 s_i), alpha_i = mu + chol_lower(S) z      k_gblup_sample
//   pass 3   r_k = r+_k - L alpha_k                 k_gblup_mul + k_gblup_sub (with sum r_k r_l and sum r_k)
// Arithmetic in double; r+, r and alpha are rounded once to the context's element type on store.  The statistics read the stored
// values.  Pad rows of L are 0, so pad rows of r+ and r stay 0.
//
// ORDER OF EVERY SUM (no floating-point atomics: two runs give the same bits, and no sum of trait k depends on T).  L alpha: a
// thread owns a row and adds the columns of its part ascending; the parts are added ascending.  s_ik: lane l adds rows 4 l .. 4 l + 3,
// 4 l + 256 ..., ascending, then a shuffle tree (32 .. 1).  Statistics: per thread one value, per workgroup a shuffle tree and the
// four waves in order, then (on the host) the workgroups ascending.
//
// DRAWS: philox4x32_10(pseudo-marker, iteration, 0x03000000, 13 + 16 q) the normal of coefficient q = first_trait + k (Box-Muller,
// jwu::normal_from) in both modes: trait k of a diagonal T-trait step draws what a one-trait step with first_trait = k draws.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwb {

constexpr int kMaxT = 4;                        // traits of a session
constexpr int kRows = 256;                      // rows per slice (= the context's)
constexpr int kMaxParts = 64;                   // column parts of k_gblup_mul
constexpr uint32_t kTag = 0x03000000u;
constexpr uint32_t kSlotZ = 13u;
// the device record of a step's parameters (doubles): vare_kk | G_kk | R^-1 | G^-1
constexpr int kParVare = 0, kParG = kMaxT, kParRinv = 2 * kMaxT, kParGinv = 2 * kMaxT + kMaxT * kMaxT, kParSize = 2 * kMaxT + 2 * kMaxT * kMaxT;

// ---- the relationship matrix ----------------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kGrmKT = 32;                      // markers per LDS tile
constexpr int kGrmChunk = 64;                   // markers per fp32 accumulation chunk (then folded into double)
constexpr int kGrmTile32 = 128, kGrmTile64 = 64;        // output tile edge: float, double

// tile index -> (ti, tj), ti >= tj
__device__ __forceinline__ void grm_tile(int idx, int& ti, int& tj)
{
    ti = 0;
    while (idx > ti) { idx -= ti + 1; ++ti; }
    tj = idx;
}

template <class real>
__device__ __forceinline__ void grm_store(real* __restrict__ K, int64_t n, int64_t p, bool diag_tile, int ga, int gc, double acc)
{
    if (ga >= n || gc >= n || (diag_tile && ga < gc)) return;
    real v = (real)acc;
    if (ga == gc) v = v + (real)1e-5;
    v = v / (real)p;
    K[(int64_t)ga * n + gc] = v;
    K[(int64_t)gc * n + ga] = v;
}

template <class real>
__global__ __launch_bounds__(256) void k_grm(const real* __restrict__ X, int64_t ld, int64_t n, int64_t p, const real* __restrict__ div, real* __restrict__ K);

// grid = nt (nt + 1) / 2 workgroups, nt = ceil(n / 128)
template <>
__global__ __launch_bounds__(256) void k_grm<float>(const float* __restrict__ X, int64_t ld, int64_t n, int64_t p, const float* __restrict__ div,
                                                    float* __restrict__ K)
{
    constexpr int E = kGrmTile32;
    __shared__ __attribute__((aligned(16))) float As[kGrmKT * E];
    __shared__ __attribute__((aligned(16))) float Bs[kGrmKT * E];
    int ti, tj;
    grm_tile((int)blockIdx.x, ti, tj);
    const bool diag = ti == tj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // staging: thread -> marker sk (+ 8, 16, 24) of the LDS tile, rows 4 sr .. 4 sr + 3 of the panel
    const int sk = tid >> 5, sr = tid & 31;
    const int64_t rowA = (int64_t)ti * E + 4 * sr, rowB = (int64_t)tj * E + 4 * sr;      // (< ld: ld is a multiple of 256)
    f32x16 acc[2][2];
    double accd[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[a][b][i] = 0.f; accd[a][b][i] = 0.0; }
    const int am = lane & 31, ah = lane >> 5;
    const float* a_rd = As + ah * E + wm * 64 + am;
    const float* b_rd = (diag ? As : Bs) + ah * E + wn * 64 + am;
    int chunk = 0;
    for (int64_t k0 = 0; k0 < p; k0 += kGrmKT) {
        float4 va[4], vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = k0 + sk + 8 * q;
            const bool in = j < p;
            const int64_t jc = in ? j : p - 1;                   // (a clamped address; a marker beyond p contributes zeros)
            const float d = div[jc];
            float4 x = *reinterpret_cast<const float4*>(X + jc * ld + rowA);
            va[q] = in ? float4{x.x / d, x.y / d, x.z / d, x.w / d} : float4{0.f, 0.f, 0.f, 0.f};
            if (!diag) {
                x = *reinterpret_cast<const float4*>(X + jc * ld + rowB);
                vb[q] = in ? float4{x.x / d, x.y / d, x.z / d, x.w / d} : float4{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();                                         // the previous tile is consumed
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<float4*>(&As[(sk + 8 * q) * E + 4 * sr]) = va[q];
            if (!diag) *reinterpret_cast<float4*>(&Bs[(sk + 8 * q) * E + 4 * sr]) = vb[q];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kGrmKT; kk += 2) {
            const float a0 = a_rd[kk * E], a1 = a_rd[kk * E + 32];
            const float b0 = b_rd[kk * E], b1 = b_rd[kk * E + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        chunk += kGrmKT;
        if (chunk >= kGrmChunk) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int i = 0; i < 16; ++i) { accd[a][b][i] = accd[a][b][i] + (double)acc[a][b][i]; acc[a][b][i] = 0.f; }
            chunk = 0;
        }
    }
    // C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); rows index the A operand
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int rr = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                grm_store<float>(K, n, p, diag, ti * E + wm * 64 + a * 32 + rr, tj * E + wn * 64 + b * 32 + (lane & 31),
                                 accd[a][b][i] + (double)acc[a][b][i]);
            }
}

// rows the matrix does not have (>= n) are 0; keep: bit u set <=> row u of the thread's four is a row of the matrix
__device__ __forceinline__ float4 grm_keep_rows(float4 v, unsigned keep)
{
    if (keep != 15u) {
        v.x = (keep & 1u) ? v.x : 0.f; v.y = (keep & 2u) ? v.y : 0.f;
        v.z = (keep & 4u) ? v.z : 0.f; v.w = (keep & 8u) ? v.w : 0.f;
    }
    return v;
}

// k_grm<float> on 2-bit packed storage (PackedCols, kernels.hpp: Q [p][ld / 4], four rows per byte; mean [p]).  The tiles, the waves, the
// LDS images, the MFMA chain, the fold and the store are k_grm<float>'s, so K has its bits; only the staging differs.  A marker has
// four possible values of x / d -- PackedCols::dec of the codes 0, 1, 2 and 3 (missing), then the dense kernel's IEEE division:
//     t[c] = ((float)c - sub) / d_j  (c < 3),   t[3] = (centered ? 0 : mu_j) / d_j,   sub = centered ? mu_j : 0
// -- formed ONCE per staged marker by the workgroup's first 128 threads (marker tid >> 2 of the LDS tile, code tid & 3: 128 divisions
// per 32-marker step where the dense kernel has 4 096 or 8 192) and shared through LDS by the A and B panels.  The four lanes of a
// marker exchange their values and lay them out as the marker's 16 PAIRS, Tp[marker][nibble] = (t[nibble & 3], t[nibble >> 2]): a
// thread's share of a marker's row panel is one payload byte, and its four rows are two 8-byte LDS reads indexed by the byte's
// nibbles -- no selection among the four values in registers (the compiler turns that into a private LDS copy with dependent reads).
// The 32 lanes that stage a marker read within its 128 bytes of Tp, one bank row: conflict-free.  Rows >= n give 0 whatever the stray
// fields of a marker's last byte hold; markers >= p give 0.
// grid = nt (nt + 1) / 2 workgroups, nt = ceil(n / 128)
__global__ __launch_bounds__(256) void k_grm_packed(const uint8_t* __restrict__ Q, int64_t ld, const float* __restrict__ mean, int32_t centered,
                                                    int64_t n, int64_t p, const float* __restrict__ div, float* __restrict__ K)
{
    constexpr int E = kGrmTile32;
    __shared__ __attribute__((aligned(16))) float As[kGrmKT * E];
    __shared__ __attribute__((aligned(16))) float Bs[kGrmKT * E];
    __shared__ __attribute__((aligned(16))) float2 Tp[kGrmKT * 16];
    int ti, tj;
    grm_tile((int)blockIdx.x, ti, tj);
    const bool diag = ti == tj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // staging: thread -> marker sk (+ 8, 16, 24) of the LDS tile, rows 4 sr .. 4 sr + 3 of the panel = byte E / 4 * tile + sr of the marker
    const int sk = tid >> 5, sr = tid & 31;
    const int64_t sb = ld >> 2;                                                          // (bytes of a marker)
    const int64_t rowA = (int64_t)ti * E + 4 * sr, rowB = (int64_t)tj * E + 4 * sr;      // (< ld: ld is a multiple of 256)
    const unsigned keepA = rowA + 4 <= n ? 15u : (rowA >= n ? 0u : (1u << (unsigned)(n - rowA)) - 1u);
    const unsigned keepB = rowB + 4 <= n ? 15u : (rowB >= n ? 0u : (1u << (unsigned)(n - rowB)) - 1u);
    const uint8_t* __restrict__ qa = Q + (rowA >> 2);
    const uint8_t* __restrict__ qb = Q + (rowB >> 2);
    f32x16 acc[2][2];
    double accd[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[a][b][i] = 0.f; accd[a][b][i] = 0.0; }
    const int am = lane & 31, ah = lane >> 5;
    const float* a_rd = As + ah * E + wm * 64 + am;
    const float* b_rd = (diag ? As : Bs) + ah * E + wn * 64 + am;
    int chunk = 0;
    // a step's global loads -- a payload byte per staged marker and panel, and the table thread's mean and divisor -- are issued a step
    // ahead, after the registers of the step before were staged, so that they are in flight under that step's MFMAs
    unsigned ba[4], bb[4];
    float mu = 0.f, dj = 1.f;
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = k0 + sk + 8 * q;
            const int64_t jc = j < p ? j : p - 1;                // (a clamped address; a marker beyond p has zeros in Tp)
            ba[q] = qa[jc * sb];
            bb[q] = diag ? 0u : (unsigned)qb[jc * sb];
        }
        if (tid < 4 * kGrmKT) {
            const int64_t j = k0 + (tid >> 2);
            const int64_t jc = j < p ? j : p - 1;
            mu = mean[jc];
            dj = div[jc];
        }
    };
    fetch(0);
    for (int64_t k0 = 0; k0 < p; k0 += kGrmKT) {
        if (tid < 4 * kGrmKT) {                                  // (waves 0 and 1; Tp was last read before the previous step's second barrier)
            const unsigned code = (unsigned)tid & 3u;
            const float x = code == 3u ? (centered ? 0.f : mu) : (float)code - (centered ? mu : 0.f);
            const float v = k0 + (tid >> 2) < p ? x / dj : 0.f;
            const int l0 = lane & ~3;
            const float t0 = __shfl(v, l0, 64), t1 = __shfl(v, l0 + 1, 64), t2 = __shfl(v, l0 + 2, 64), t3 = __shfl(v, l0 + 3, 64);
            float4* out = reinterpret_cast<float4*>(&Tp[4 * tid]);      // nibbles 4 code + k: (t[k], t[code])
            out[0] = float4{t0, v, t1, v};
            out[1] = float4{t2, v, t3, v};
        }
        __syncthreads();                                         // the previous tile is consumed; Tp is written
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float2* __restrict__ t = &Tp[16 * (sk + 8 * q)];
            const float2 a01 = t[ba[q] & 15u], a23 = t[ba[q] >> 4];
            *reinterpret_cast<float4*>(&As[(sk + 8 * q) * E + 4 * sr]) = grm_keep_rows(float4{a01.x, a01.y, a23.x, a23.y}, keepA);
            if (!diag) {
                const float2 b01 = t[bb[q] & 15u], b23 = t[bb[q] >> 4];
                *reinterpret_cast<float4*>(&Bs[(sk + 8 * q) * E + 4 * sr]) = grm_keep_rows(float4{b01.x, b01.y, b23.x, b23.y}, keepB);
            }
        }
        fetch(k0 + kGrmKT);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kGrmKT; kk += 2) {
            const float a0 = a_rd[kk * E], a1 = a_rd[kk * E + 32];
            const float b0 = b_rd[kk * E], b1 = b_rd[kk * E + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        chunk += kGrmKT;
        if (chunk >= kGrmChunk) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int i = 0; i < 16; ++i) { accd[a][b][i] = accd[a][b][i] + (double)acc[a][b][i]; acc[a][b][i] = 0.f; }
            chunk = 0;
        }
    }
    // C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); rows index the A operand
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int rr = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                grm_store<float>(K, n, p, diag, ti * E + wm * 64 + a * 32 + rr, tj * E + wn * 64 + b * 32 + (lane & 31),
                                 accd[a][b][i] + (double)acc[a][b][i]);
            }
}

// grid = nt (nt + 1) / 2 workgroups, nt = ceil(n / 64)
template <>
__global__ __launch_bounds__(256) void k_grm<double>(const double* __restrict__ X, int64_t ld, int64_t n, int64_t p, const double* __restrict__ div,
                                                     double* __restrict__ K)
{
    constexpr int E = kGrmTile64;
    __shared__ __attribute__((aligned(16))) double As[kGrmKT * E];
    __shared__ __attribute__((aligned(16))) double Bs[kGrmKT * E];
    int ti, tj;
    grm_tile((int)blockIdx.x, ti, tj);
    const bool diag = ti == tj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // staging: thread -> marker sk (+ 8, 16, 24) of the LDS tile, rows 2 sr, 2 sr + 1 of the panel
    const int sk = tid >> 5, sr = tid & 31;
    const int64_t rowA = (int64_t)ti * E + 2 * sr, rowB = (int64_t)tj * E + 2 * sr;      // (< ld: ld is a multiple of 256)
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[a][b][i] = 0.0;
    const int am = lane & 15, ah = lane >> 4;
    const double* a_rd = As + ah * E + wm * 32 + am;
    const double* b_rd = (diag ? As : Bs) + ah * E + wn * 32 + am;
    for (int64_t k0 = 0; k0 < p; k0 += kGrmKT) {
        double2 va[4], vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = k0 + sk + 8 * q;
            const bool in = j < p;
            const int64_t jc = in ? j : p - 1;
            const double d = div[jc];
            double2 x = *reinterpret_cast<const double2*>(X + jc * ld + rowA);
            va[q] = in ? double2{x.x / d, x.y / d} : double2{0.0, 0.0};
            if (!diag) {
                x = *reinterpret_cast<const double2*>(X + jc * ld + rowB);
                vb[q] = in ? double2{x.x / d, x.y / d} : double2{0.0, 0.0};
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<double2*>(&As[(sk + 8 * q) * E + 2 * sr]) = va[q];
            if (!diag) *reinterpret_cast<double2*>(&Bs[(sk + 8 * q) * E + 2 * sr]) = vb[q];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kGrmKT; kk += 4) {
            const double a0 = a_rd[kk * E], a1 = a_rd[kk * E + 16];
            const double b0 = b_rd[kk * E], b1 = b_rd[kk * E + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D layout of the f64 16 x 16 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                grm_store<double>(K, n, p, diag, ti * E + wm * 32 + a * 16 + (lane >> 4) + 4 * i, tj * E + wn * 32 + b * 16 + (lane & 15), acc[a][b][i]);
}

// ---- the sampler's passes --------------------------------------------------------------------------------------------------------------
// part[(part T + k) ld + row] = sum over the part's columns j (ascending) of L[row, j] alpha_k[j].  grid = (nslices, nparts)
template <class real, int T>
__global__ __launch_bounds__(256) void k_gblup_mul(const real* __restrict__ L, int64_t ld, int64_t n, int32_t len, const real* __restrict__ alpha,
                                                   double* __restrict__ part)
{
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * len, c1 = c0 + len < n ? c0 + len : n;
    double acc[T];
#pragma unroll
    for (int k = 0; k < T; ++k) acc[k] = 0.0;
#pragma unroll 4
    for (int64_t j = c0; j < c1; ++j) {
        const double x = (double)L[j * ld + row];
#pragma unroll
        for (int k = 0; k < T; ++k) acc[k] = acc[k] + x * (double)alpha[(int64_t)k * n + j];
    }
#pragma unroll
    for (int k = 0; k < T; ++k) part[((int64_t)blockIdx.y * T + k) * ld + row] = acc[k];
}

// r+_k = r_k + (part 0 + part 1 + ...).  grid = (nslices)
template <class real, int T>
__global__ __launch_bounds__(256) void k_gblup_add(const real* __restrict__ r, const double* __restrict__ part, int32_t nparts, int64_t ld,
                                                   real* __restrict__ rplus)
{
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x;
#pragma unroll
    for (int k = 0; k < T; ++k) {
        double s = part[(int64_t)k * ld + row];
        for (int q = 1; q < nparts; ++q) s = s + part[((int64_t)q * T + k) * ld + row];
        rplus[(int64_t)k * ld + row] = (real)((double)r[(int64_t)k * ld + row] + s);
    }
}

// r_k = r+_k - (part 0 + part 1 + ...); fin[slice][T T + T]: sum r_k r_l (k T + l), sum r_k of the slice.  grid = (nslices)
template <class real, int T>
__global__ __launch_bounds__(256) void k_gblup_sub(const real* __restrict__ rplus, const double* __restrict__ part, int32_t nparts, int64_t ld,
                                                   real* __restrict__ r, double* __restrict__ fin)
{
    __shared__ double sh[4 * (T * T + T)];
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x;
    double v[T], acc[T * T + T];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        double s = part[(int64_t)k * ld + row];
        for (int q = 1; q < nparts; ++q) s = s + part[((int64_t)q * T + k) * ld + row];
        const real out = (real)((double)rplus[(int64_t)k * ld + row] - s);
        r[(int64_t)k * ld + row] = out;
        v[k] = (double)out;
    }
#pragma unroll
    for (int k = 0; k < T; ++k) {
#pragma unroll
        for (int l = 0; l < T; ++l) acc[k * T + l] = v[k] * v[l];
        acc[T * T + k] = v[k];
    }
    jwu::block_reduce<T * T + T>(acc, sh, fin + (int64_t)blockIdx.x * (T * T + T));
}

// s[i T + k] = l_i' r+_k: one wave per column.  grid = ceil(n / 4) workgroups of 4 waves
template <class real, int T>
__global__ __launch_bounds__(256) void k_gblup_rhs(const real* __restrict__ L, int64_t ld, int64_t n, const real* __restrict__ rplus, double* __restrict__ s)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const real* __restrict__ col = L + i * ld;
    double acc[T];
#pragma unroll
    for (int k = 0; k < T; ++k) acc[k] = 0.0;
    for (int64_t row = 4 * lane; row < ld; row += 256) {
        double x[4];
        jwu::load4(col + row, x);
#pragma unroll
        for (int k = 0; k < T; ++k) {
            double w[4];
            jwu::load4(rplus + (int64_t)k * ld + row, w);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[k] = acc[k] + x[u] * w[u];
        }
    }
#pragma unroll
    for (int k = 0; k < T; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
        if (lane == 0) s[i * T + k] = v;
    }
}

// T x T inverse: Gauss-Jordan in double with partial pivoting, the operation sequence of the host's inv_small (ctx.hpp)
template <int T>
__device__ __forceinline__ void inv_small_dev(const double (&A)[T][T], double (&Ainv)[T][T])
{
    double M[T][2 * T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) { M[i][j] = A[i][j]; M[i][T + j] = (i == j) ? 1.0 : 0.0; }
#pragma unroll
    for (int c = 0; c < T; ++c) {
        int piv = c;
        double best = fabs(M[c][c]);
#pragma unroll
        for (int i = c + 1; i < T; ++i) { const double v = fabs(M[i][c]); if (v > best) { best = v; piv = i; } }
#pragma unroll
        for (int i = c + 1; i < T; ++i)
            if (i == piv) {
#pragma unroll
                for (int j = 0; j < 2 * T; ++j) { const double tmp = M[c][j]; M[c][j] = M[i][j]; M[i][j] = tmp; }
            }
        const double d = M[c][c];
#pragma unroll
        for (int j = 0; j < 2 * T; ++j) M[c][j] /= d;
#pragma unroll
        for (int i = 0; i < T; ++i) if (i != c) {
            const double f = M[i][c];
            if (f != 0.0) {
#pragma unroll
                for (int j = 0; j < 2 * T; ++j) M[i][j] -= f * M[c][j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) Ainv[i][j] = M[i][T + j];
}

struct SampleArgs {
    const double* s;                    // [n][T]
    const double* D;                    // [n]
    const double* par;                  // [kParSize]
    void *alpha, *beta;                 // [T][n] (real)
    double* stat;                       // [workgroups][T T]: sum_i alpha_ik alpha_il / D_i of the workgroup's pseudo-markers
    int64_t n;
    uint32_t iter, seed_lo, seed_hi, first;
    int32_t diagonal;
};

// one thread per pseudo-marker.  grid = ceil(n / 256)
template <class real, int T>
__global__ __launch_bounds__(256) void k_gblup_sample(const SampleArgs A)
{
    __shared__ double sh[4 * T * T];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double a[T], acc[T * T];
#pragma unroll
    for (int k = 0; k < T; ++k) a[k] = 0.0;
    double di = 1.0;
    if (i < A.n) {
        di = A.D[i];
        double z[T], s[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            z[k] = jwu::normal_from(jw::philox4x32_10((uint32_t)i, A.iter, kTag, kSlotZ + 16u * (A.first + (uint32_t)k), A.seed_lo, A.seed_hi));
            s[k] = A.s[i * T + k];
        }
        if (A.diagonal) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const double vare = A.par[kParVare + k];
                const double lhs = 1.0 + vare / (A.par[kParG + k] * di);
                a[k] = s[k] / lhs + z[k] * sqrt(vare / lhs);
            }
        } else {
            double lhs[T][T], S[T][T], C[T][T], w[T];
#pragma unroll
            for (int k = 0; k < T; ++k) {
                double t = 0.0;
#pragma unroll
                for (int l = 0; l < T; ++l) {
                    lhs[k][l] = A.par[kParRinv + k * T + l] + A.par[kParGinv + k * T + l] / di;
                    t = t + A.par[kParRinv + k * T + l] * s[l];
                }
                w[k] = t;
            }
            inv_small_dev<T>(lhs, S);
            jwu::chol_lower<T>(S, C);
#pragma unroll
            for (int k = 0; k < T; ++k) {
                double mu = 0.0;
#pragma unroll
                for (int l = 0; l < T; ++l) mu = mu + S[k][l] * w[l];
#pragma unroll
                for (int l = 0; l <= k; ++l) mu = mu + C[k][l] * z[l];
                a[k] = mu;
            }
        }
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const real out = (real)a[k];
            ((real*)A.alpha)[(int64_t)k * A.n + i] = out;
            ((real*)A.beta)[(int64_t)k * A.n + i] = out;
            a[k] = (double)out;
        }
    }
#pragma unroll
    for (int k = 0; k < T; ++k)
#pragma unroll
        for (int l = 0; l < T; ++l) acc[k * T + l] = (a[k] * a[l]) / di;
    jwu::block_reduce<T * T>(acc, sh, A.stat + (int64_t)blockIdx.x * (T * T));
}

}  // namespace jwb
