// plink.hpp -- a PLINK 1 binary genotype file (.bed, variant-major) into the 2-bit codes of packed storage (session_plink.hip has the entry
// points).  Both layouts are marker-major with four individuals per byte, individual i in byte i >> 2 at bit shift (i & 3) << 1; what
// differs is the meaning of a field, the individuals that are kept and their order, the row stride, and the markers that stay.
//
//   .bed field f           .jgb2 code, counted allele A1      counted allele A2
//   0  homozygous A1       2                                  0
//   1  missing             3                                  3
//   2  heterozygous        1                                  1
//   3  homozygous A2       0                                  2
//
// On the bit planes of a dword (hi = w >> 1 & 0x55555555, lo = w & 0x55555555): A1: hi' = ~hi, lo' = hi ^ lo; A2: hi' = lo, lo' = hi ^ lo.
// Fields past the last kept individual come out as code 0 whatever the file holds there: the pad rows of packed storage are zeros.
// Integer arithmetic only; the counts are popcounts summed by a shuffle tree and then over the waves in wave order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwk {

constexpr int kThreads = 256;
constexpr unsigned kPlane = 0x55555555u;
enum { kDirect = 0, kGatherLds = 1, kGatherGlobal = 2 };      // how k_plink_transcode reads a marker's raw row
constexpr int64_t kMaxLdsRow = 60 << 10;                     // raw rows up to this many bytes are staged in LDS (n_file <= 245 760)

struct TranscodeArgs {
    const uint8_t* raw;         // [m][rpitch] the chunk's raw rows; bytes [bpm, rpitch) of a row are not initialised
    int64_t rpitch;             // a multiple of 16
    uint8_t* out;               // [m][sb] packed rows
    int64_t sb;                 // ld / 4, a multiple of 64
    long long* counts;          // [m][4] individuals with code 0, 1, 2, 3
    const int32_t* rows;        // [n_rows rounded up to 16] file rows of the kept individuals, pads 0 (kDirect: not read)
    int64_t n_rows;             // kept individuals (kDirect: all of the file's)
    int32_t count_a1;
};

// the plane bits of the first nvalid fields of a dword
__device__ __forceinline__ unsigned field_mask(int64_t nvalid)
{
    return nvalid >= 16 ? kPlane : nvalid <= 0 ? 0u : (((1u << (2 * (int)nvalid)) - 1u) & kPlane);
}

// 16 .bed fields -> 16 codes; m: field_mask of the fields that exist; c1 .. c3 grow by the number of codes 1, 2, 3
__device__ __forceinline__ unsigned transcode16(unsigned w, unsigned m, int a1, int& c1, int& c2, int& c3)
{
    const unsigned hi = (w >> 1) & kPlane, lo = w & kPlane;
    const unsigned h = (a1 ? ~hi : lo) & m, l = (hi ^ lo) & m;
    c1 += __popc(~h & l);
    c2 += __popc(h & ~l);
    c3 += __popc(h & l);
    return (h << 1) | l;
}

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// the workgroup's counts of codes 1, 2, 3 -> out[0 .. 4); sh: 12 ints of LDS
__device__ __forceinline__ void store_counts(int c1, int c2, int c3, int64_t n_rows, int* sh, long long* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c1 = wave_sum_int(c1); c2 = wave_sum_int(c2); c3 = wave_sum_int(c3);
    if (lane == 0) { sh[wave * 3] = c1; sh[wave * 3 + 1] = c2; sh[wave * 3 + 2] = c3; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long t1 = ((sh[0] + sh[3]) + sh[6]) + sh[9], t2 = ((sh[1] + sh[4]) + sh[7]) + sh[10], t3 = ((sh[2] + sh[5]) + sh[8]) + sh[11];
        out[0] = (long long)n_rows - t1 - t2 - t3; out[1] = t1; out[2] = t2; out[3] = t3;
    }
}

// field i of a raw row
template <class P>
__device__ __forceinline__ unsigned raw_field(P row, int32_t i) { return ((unsigned)row[i >> 2] >> ((i & 3) << 1)) & 3u; }

// One workgroup per marker of a chunk.  kDirect: all individuals in file order, 64 per lane and step (one 16-byte load, one 16-byte
// store).  kGather*: output dword d holds the individuals rows[16 d .. 16 d + 16), gathered from the raw row in LDS (kGatherLds; the
// dynamic LDS is rpitch + 64 bytes) or in global memory (kGatherGlobal; 64 bytes).
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_plink_transcode(const TranscodeArgs A)
{
    extern __shared__ uint4 sh_dyn[];
    const int64_t j = blockIdx.x;
    const uint8_t* __restrict__ src = A.raw + j * A.rpitch;
    int c1 = 0, c2 = 0, c3 = 0;
    int* sh_cnt;
    if (MODE == kDirect) {
        sh_cnt = (int*)sh_dyn;
        const uint4* __restrict__ src4 = (const uint4*)src;
        uint4* __restrict__ dst4 = (uint4*)(A.out + j * A.sb);
        const int64_t nq = A.sb >> 4, nsrc = A.rpitch >> 4;
        for (int64_t q = threadIdx.x; q < nq; q += kThreads) {
            const uint4 v = q < nsrc ? src4[q] : make_uint4(0u, 0u, 0u, 0u);
            const int64_t left = A.n_rows - q * 64;
            uint4 o;
            o.x = transcode16(v.x, field_mask(left), A.count_a1, c1, c2, c3);
            o.y = transcode16(v.y, field_mask(left - 16), A.count_a1, c1, c2, c3);
            o.z = transcode16(v.z, field_mask(left - 32), A.count_a1, c1, c2, c3);
            o.w = transcode16(v.w, field_mask(left - 48), A.count_a1, c1, c2, c3);
            dst4[q] = o;
        }
    } else {
        const int64_t nsrc = A.rpitch >> 4;
        if (MODE == kGatherLds) {
            sh_cnt = (int*)(sh_dyn + nsrc);
            for (int64_t q = threadIdx.x; q < nsrc; q += kThreads) sh_dyn[q] = ((const uint4*)src)[q];
            __syncthreads();
        } else sh_cnt = (int*)sh_dyn;
        const uint8_t* lds_row = (const uint8_t*)sh_dyn;
        unsigned* __restrict__ dst = (unsigned*)(A.out + j * A.sb);
        const int64_t nd = A.sb >> 2;
        for (int64_t d = threadIdx.x; d < nd; d += kThreads) {
            const int64_t left = A.n_rows - d * 16;
            unsigned w = 0u;
            if (left > 0) {
                const int4* __restrict__ rp = (const int4*)(A.rows + d * 16);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int4 s = rp[k];
                    unsigned f;
                    if (MODE == kGatherLds)
                        f = raw_field(lds_row, s.x) | raw_field(lds_row, s.y) << 2 | raw_field(lds_row, s.z) << 4 | raw_field(lds_row, s.w) << 6;
                    else
                        f = raw_field(src, s.x) | raw_field(src, s.y) << 2 | raw_field(src, s.z) << 4 | raw_field(src, s.w) << 6;
                    w |= f << (8 * k);
                }
            }
            dst[d] = transcode16(w, field_mask(left), A.count_a1, c1, c2, c3);
        }
    }
    store_counts(c1, c2, c3, A.n_rows, sh_cnt, A.counts + j * 4);
}

// Row j of dst <- row selected[j] of src, 16 bytes per lane and step; one workgroup per kept marker.  sb: the row stride of both
__global__ void __launch_bounds__(kThreads) k_plink_compact(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t sb,
                                                            const int64_t* __restrict__ selected)
{
    const int64_t j = blockIdx.x;
    const uint4* __restrict__ s4 = (const uint4*)(src + selected[j] * sb);
    uint4* __restrict__ d4 = (uint4*)(dst + j * sb);
    const int64_t nq = sb >> 4;
    for (int64_t q = threadIdx.x; q < nq; q += kThreads) d4[q] = s4[q];
}

}  // namespace jwk
