// mtmiss.hpp -- multi-trait records that miss some traits, on the device.
//
// The reference weights every record with the inverse of the OBSERVED block of R (mkRi / getRi, residual.jl:2-44) and redraws the
// residuals of the missing traits from their conditional given the observed ones every iteration (sampleMissingResiduals,
// residual.jl:51-73).  Every record carries a CODE: bit k set = trait k observed, 1 .. 2^t - 1, t <= kMaxT, so at most 15 patterns.
// The caller forms three tables per code in double on the host, [2^t][t][t] each (row-major, unused entries 0), o = the observed
// traits ascending, m = the missing ones ascending:
//   B[code]  |m| x |o|   R[m,o] inv(R[o,o])                                   (top-left corner)
//   U[code]  |m| x |m|   the upper Cholesky factor of R[m,m] - R[m,o] inv(R[o,o]) R[o,m]
//   C[code]  t x t       inv(R[o,o]) embedded in zeros: the RZ of getRi        (read by k_locpar_sums<T, true>, locpar.hpp)
//
//   k_mtmiss_impute<T>   one thread per record; a record whose code is not the full one gets, for c = 0 .. |m| - 1,
//       e_m[c] = sum_j B[c][j] e_o[j] + sum_{a <= c} z_m[a] U[a][c]           (mydata[:, o] Ri Rc' + randn U of residual.jl:69)
//   the sums in the index order written (j ascending, then a ascending), e_o widened from T, the result rounded to T once.
//   z_k: rng.hpp's Box-Muller normal (slot 4) on the counter (record, iteration, 0x10000000, 4 + 16 k).  Observed cells and
//   complete records are not written at all.  (T = float | double: the residual's element type; arithmetic in double.)
// The trait loops are unrolled over kMaxT with predicates and the compacted values are moved with selects: everything stays in
// registers.  No floating-point atomics, no waits between workgroups: a record is one thread's, launch order is the only
// synchronisation.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwm {

constexpr uint32_t kRepTag = 0x10000000u;      // (kMaxT, kMaxCodes: device_util.hpp)
constexpr uint32_t kSlot = 4u;

struct ImputeArgs {
    void* r;                            // [nt][ld] residuals (T)
    int64_t ld, n;
    const int32_t* code;                // [n]
    const double* B;                    // [2^nt][nt][nt]
    const double* U;                    // [2^nt][nt][nt]
    int32_t nt;
    uint32_t iter, seed_lo, seed_hi;
};

template <class T>
__global__ __launch_bounds__(256) void k_mtmiss_impute(const ImputeArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const int nt = A.nt;
    const int cd = A.code[i];
    if (cd == (1 << nt) - 1) return;
    T* r = (T*)A.r;
    double eo[kMaxT] = {0.0, 0.0, 0.0, 0.0}, z[kMaxT] = {0.0, 0.0, 0.0, 0.0};      // compacted: the observed residuals, the normals of the missing traits
    int no = 0, nm = 0;
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) {
        if (k >= nt) continue;
        if ((cd >> k) & 1) {
            const double v = (double)r[(size_t)k * A.ld + i];
#pragma unroll
            for (int q = 0; q < kMaxT; ++q) eo[q] = q == no ? v : eo[q];
            ++no;
        } else {
            const jw::u32x4 w = jw::philox4x32_10((uint32_t)i, A.iter, kRepTag, kSlot + 16u * (uint32_t)k, A.seed_lo, A.seed_hi);
            const double u1 = jw::u52(w.x, w.y), u2 = jw::u52(w.z, w.w);
            const double v = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
#pragma unroll
            for (int q = 0; q < kMaxT; ++q) z[q] = q == nm ? v : z[q];
            ++nm;
        }
    }
    const double* Bc = A.B + (size_t)cd * nt * nt;
    const double* Uc = A.U + (size_t)cd * nt * nt;
    int c = 0;                                                  // the position of trait k among the missing ones
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) {
        if (k >= nt || ((cd >> k) & 1)) continue;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxT; ++j)
            if (j < no) acc = acc + Bc[c * nt + j] * eo[j];
#pragma unroll
        for (int a = 0; a < kMaxT; ++a)
            if (a <= c) acc = acc + z[a] * Uc[a * nt + c];
        r[(size_t)k * A.ld + i] = (T)acc;
        ++c;
    }
}

}  // namespace jwm
