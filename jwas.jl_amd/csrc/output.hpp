// output.hpp -- the kernels of a context's output side (output.hip): X alpha on training or output rows, sparse samples, the
// window sums of the GWAS and its session, the running posterior means.  One kernel per job for both precisions: each is a
// template on the column view (DenseCols / PackedCols: float; DenseCols64: double) or on the element type, so every unit that
// includes this header may instantiate it (a non-template __global__ here would be a duplicate host symbol at link time).
//
// The arithmetic of a view with element type T: effects are T, a term is acc = fma(double(val), double(x), acc) in list order
// (double(.) of a double is the value itself), sums over rows go through the wave shuffle tree, the four waves as
// ((0 + 1) + 2) + 3 and the slices in order.  How many column loads are in flight does not enter the arithmetic.
#pragma once
#include "kernels.hpp"
#include "ctx.hpp"

namespace jw {

// DenseCols over double: marker-major, column stride ld (a multiple of 256 rows, pad rows zero)
struct DenseCols64 {
    const double* X; int64_t ld;
    __device__ __forceinline__ double load1(int64_t j, int64_t row) const { return X[j * ld + row]; }
};
template <class CX> struct ColsElem { typedef float type; };
template <> struct ColsElem<DenseCols64> { typedef double type; };
template <class CX> using elem_t = typename ColsElem<CX>::type;

// Per-precision launch policy of X alpha over a list.  It moves speed, never bits.
//   rows per workgroup: a Float64 row is 8 bytes, so 64-row workgroups put four times as many waves on the device for the short
//   matrices this runs on; Float32 keeps one 256-row slice per workgroup;
//   dense fallback: Float32 takes the loop over all markers (k_mul_alpha) when more than a quarter of the effects are nonzero,
//   Float64 always takes the list.
template <class T> struct ListPolicy;
template <> struct ListPolicy<float>  { static constexpr int kRows = kSliceRows; static constexpr bool kDenseFallback = true; };
template <> struct ListPolicy<double> { static constexpr int kRows = 64;         static constexpr bool kDenseFallback = false; };

// ---- running posterior means (output.jl:556-577): m += (x - m) / k, the difference in T and the quotient in double -----------------
template <class T>
__global__ __launch_bounds__(256) void k_accumulate(int64_t count, int delta_is_class, double k, const T* __restrict__ alpha,
                                                    const void* __restrict__ delta_v, T* __restrict__ mean_a, T* __restrict__ mean_a2,
                                                    T* __restrict__ mean_d)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const T a = alpha[j];
    mean_a[j] = (T)((double)mean_a[j] + ((double)(a - mean_a[j])) / k);
    const T a2 = a * a;
    mean_a2[j] = (T)((double)mean_a2[j] + ((double)(a2 - mean_a2[j])) / k);
    const T ind = delta_is_class ? (reinterpret_cast<const int32_t*>(delta_v)[j] > 1 ? T(1) : T(0)) : reinterpret_cast<const T*>(delta_v)[j];
    mean_d[j] = (T)((double)mean_d[j] + ((double)(ind - mean_d[j])) / k);
}

// ---- X * alpha (EBV, output.jl:281-306) and r -= X * alpha (the initial ycorr, MCMC_BayesianAlphabet.jl:142) -----------------------
// grid = nslices, block = 256: one row per thread, columns in marker order.  Dense effects: 16 independent column loads in flight
// per thread; a zero effect contributes fma(0, x, s) = s exactly, so nothing is skipped and nothing branches.
template <class CX>
__global__ __launch_bounds__(256) void k_mul_alpha(CX cx, int64_t p, const elem_t<CX>* __restrict__ alpha, elem_t<CX>* __restrict__ out)
{
    typedef elem_t<CX> T;
    const int64_t row = (int64_t)blockIdx.x * kSliceRows + threadIdx.x;
    double s = 0.0;
    constexpr int kUn = 16;
    int64_t j = 0;
    for (; j + kUn <= p; j += kUn) {
        T x[kUn];
#pragma unroll
        for (int u = 0; u < kUn; ++u) x[u] = cx.load1(j + u, row);
#pragma unroll
        for (int u = 0; u < kUn; ++u) s = fma((double)alpha[j + u], (double)x[u], s);
    }
    for (; j < p; ++j) s = fma((double)alpha[j], (double)cx.load1(j, row), s);
    out[row] = (T)s;
}

// r[row] = fma(-alpha_j, x_j, r[row]) over the nonzero effects in marker order, in T
template <class CX>
__global__ __launch_bounds__(256) void k_sub_xalpha(CX cx, int64_t p, const elem_t<CX>* __restrict__ alpha, elem_t<CX>* __restrict__ r)
{
    typedef elem_t<CX> T;
    const int64_t row = (int64_t)blockIdx.x * kSliceRows + threadIdx.x;
    T rv = r[row];
    for (int64_t j = 0; j < p; ++j) {
        const T a = alpha[j];
        if (a != T(0)) rv = fma(-a, cx.load1(j, row), rv);
    }
    r[row] = rv;
}

// The nonzero effects of one trait as (index, value) lists in marker order.  grid = 1, block = 1024: the workgroup walks the p
// effects 1024 at a time with a running offset (ballot + wave prefix), ~30 us at p = 600 000; idx / val hold p entries, *count
// the number written.
template <class T>
__global__ __launch_bounds__(1024) void k_compact_alpha(int64_t p, const T* __restrict__ alpha, int32_t* __restrict__ idx, T* __restrict__ val,
                                                        int32_t* __restrict__ count)
{
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int64_t j0 = 0; j0 < p; j0 += 1024) {
        const int64_t j = j0 + tid;
        const T a = j < p ? alpha[j] : T(0);
        const bool nz = a != T(0);
        const unsigned long long m = __ballot(nz);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int pre = base_s, tot = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) pre += wsum[w]; tot += wsum[w]; }
        if (nz) {
            const int pos = pre + __popcll(m & ((1ull << lane) - 1ull));
            idx[pos] = (int32_t)j; val[pos] = a;
        }
        __syncthreads();
        if (tid == 0) base_s += tot;
        __syncthreads();
    }
    if (tid == 0) *count = base_s;
}

// K column loads of one row in flight, then their fma chain in list order.  NV = 5: a second effect vector over the same columns.
template <int K, int NV, class CX>
__device__ __forceinline__ void list_terms(const CX& cx, int64_t row, const int32_t* __restrict__ idx, const elem_t<CX>* __restrict__ val,
                                           const elem_t<CX>* __restrict__ val2, int e, double& acc, double& acc2)
{
    elem_t<CX> x[K];
#pragma unroll
    for (int u = 0; u < K; ++u) x[u] = cx.load1(idx[e + u], row);
#pragma unroll
    for (int u = 0; u < K; ++u) {
        acc = fma((double)val[e + u], (double)x[u], acc);
        if constexpr (NV == 5) acc2 = fma((double)val2[e + u], (double)x[u], acc2);
    }
}

// the list [e_lo, e_hi) into acc, 16 / 4 / 1 loads in flight
template <class CX>
__device__ __forceinline__ void list_sum(const CX& cx, int64_t row, const int32_t* __restrict__ idx, const elem_t<CX>* __restrict__ val, int e_lo, int e_hi,
                                         double& acc)
{
    double unused = 0.0;
    int e = e_lo;
    for (; e + 16 <= e_hi; e += 16) list_terms<16, 2>(cx, row, idx, val, nullptr, e, acc, unused);
    for (; e + 4 <= e_hi; e += 4) list_terms<4, 2>(cx, row, idx, val, nullptr, e, acc, unused);
    for (; e < e_hi; ++e) list_terms<1, 2>(cx, row, idx, val, nullptr, e, acc, unused);
}

// X * alpha over the nonzero effects only (marker order, the fma chain of k_mul_alpha -> identical results): with a sparse prior a
// saved sample has a few hundred nonzero effects among 600 000, and the loop over all markers costs 39 ms where the 600 useful
// columns cost 30 us.  One row per thread, grid = ld / ROWS (ListPolicy), so every row is inside the padded column.
template <class CX, int ROWS>
__global__ __launch_bounds__(ROWS) void k_mul_alpha_list(CX cx, int nnz, const int32_t* __restrict__ idx, const elem_t<CX>* __restrict__ val,
                                                         elem_t<CX>* __restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x;
    double s = 0.0;
    list_sum(cx, row, idx, val, 0, nnz, s);
    out[row] = (elem_t<CX>)s;
}

// ---- the EBVs of all traits on 2-bit packed output rows (jwas_hip_ebv_output; getEBV, output.jl:281-306) --------------------------
// The markers with a nonzero effect in ANY of the nt traits as one ascending list, with every trait's effect at each of them:
// k_compact_alpha's walk with the union as its predicate.  idx: [p], val: [nt][p] (trait-major), *count: the list's length.
// grid = 1, block = 1024.
template <class T>
__global__ __launch_bounds__(1024) void k_compact_alpha_union(int64_t p, int nt, const T* __restrict__ alpha, int32_t* __restrict__ idx, T* __restrict__ val,
                                                              int32_t* __restrict__ count)
{
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int64_t j0 = 0; j0 < p; j0 += 1024) {
        const int64_t j = j0 + tid;
        bool nz = false;
        if (j < p) for (int k = 0; k < nt; ++k) nz = nz || alpha[(int64_t)k * p + j] != T(0);
        const unsigned long long m = __ballot(nz);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int pre = base_s, tot = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) pre += wsum[w]; tot += wsum[w]; }
        if (nz) {
            const int pos = pre + __popcll(m & ((1ull << lane) - 1ull));
            idx[pos] = (int32_t)j;
            for (int k = 0; k < nt; ++k) val[(int64_t)k * p + pos] = alpha[(int64_t)k * p + j];
        }
        __syncthreads();
        if (tid == 0) base_s += tot;
        __syncthreads();
    }
    if (tid == 0) *count = base_s;
}

// K bytes of one thread in flight, then their terms in list order: the four rows of a byte times the NT effects of its marker.  The
// decode is PackedCols::dec and the pad-row rule of PackedCols::load1 (keep: bit k set when row k of the byte is below cx.n).
template <int K, int NT>
__device__ __forceinline__ void ebv_terms(const PackedCols& cx, int64_t byte_off, unsigned keep, const int32_t* __restrict__ idx, const float* __restrict__ val,
                                          int64_t vstride, int e, double (&s)[NT][4])
{
    unsigned b[K]; float mu[K];
#pragma unroll
    for (int u = 0; u < K; ++u) { const int64_t j = idx[e + u]; b[u] = cx.Q[j * (cx.ld >> 2) + byte_off]; mu[u] = cx.mean[j]; }
#pragma unroll
    for (int u = 0; u < K; ++u) {
        double a[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) a[k] = (double)val[(int64_t)k * vstride + e + u];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = ((keep >> q) & 1u) ? cx.dec((b[u] >> (2 * q)) & 3u, mu[u]) : 0.f;
#pragma unroll
            for (int k = 0; k < NT; ++k) s[k][q] = fma(a[k], (double)x, s[k][q]);
        }
    }
}

// out[k * ld + row] = (float) sum_j alpha_kj x_(row, j) for the NT traits at once: s = fma(double(alpha), double(x), s) over the union
// list in marker order, the chain of k_mul_alpha_list / k_mul_alpha for every trait (a zero effect of the union adds fma(0, x, s) = s),
// hence their bits.  A thread owns the four rows of one byte: it reads that byte once per listed marker (16 / 4 / 1 of them in
// flight) and keeps 4 NT sums.  grid = ld / 256, block = 64: one wave per 256-row slice, so a column's 64 bytes are one load.
template <int NT>
__global__ __launch_bounds__(64) void k_ebv_packed(PackedCols cx, int nnz, const int32_t* __restrict__ idx, const float* __restrict__ val, int64_t vstride,
                                                   float* __restrict__ out)
{
    const int64_t byte_off = (int64_t)blockIdx.x * 64 + threadIdx.x, row = byte_off << 2;
    unsigned keep = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) keep |= (row + q < cx.n ? 1u : 0u) << q;
    double s[NT][4] = {};
    int e = 0;
    for (; e + 16 <= nnz; e += 16) ebv_terms<16, NT>(cx, byte_off, keep, idx, val, vstride, e, s);
    for (; e + 4 <= nnz; e += 4) ebv_terms<4, NT>(cx, byte_off, keep, idx, val, vstride, e, s);
    for (; e < nnz; ++e) ebv_terms<1, NT>(cx, byte_off, keep, idx, val, vstride, e, s);
#pragma unroll
    for (int k = 0; k < NT; ++k)
        *reinterpret_cast<float4*>(out + (int64_t)k * cx.ld + row) = float4{(float)s[k][0], (float)s[k][1], (float)s[k][2], (float)s[k][3]};
}

// ---- window genomic values of one marker-effect sample (GWAS.jl:152-165, :199-217) ----------------------------------------------
// Window w holds the nonzero effects idx / val[wptr[w] .. wptr[w+1]); BV_w[i] = sum_j X[i, idx_j] val_j in list order (8 column
// loads in flight, one for a window's tail).  grid = nslices, block = 256 (one individual per thread);
// partial[(w * nslices + slice) * NV + v]: NV = 2: (sum, sum of squares) of BV_w;  NV = 5: two effect vectors over the same markers
// (two traits' samples): (sum1, ss1, sum2, ss2, sum of products).  The lanes of a wave are added by shuffles, the four waves as
// ((0 + 1) + 2) + 3; k_window_reduce then adds the slices in order (no atomics).  (The reduction stands in this kernel and in
// k_gwas_partial: as a shared device function it came out with another register allocation than the kernels it replaces.)
template <class CX, int NV>
__global__ __launch_bounds__(256) void k_window_partial(CX cx, int nwin, const int32_t* __restrict__ wptr, const int32_t* __restrict__ idx,
                                                        const elem_t<CX>* __restrict__ val, const elem_t<CX>* __restrict__ val2, double* __restrict__ partial)
{
    __shared__ double red[NV][4];
    const int64_t row = (int64_t)blockIdx.x * kSliceRows + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int w = 0; w < nwin; ++w) {
        double bv = 0.0, bv2 = 0.0;
        const int e_hi = wptr[w + 1];
        int e = wptr[w];
        for (; e + 8 <= e_hi; e += 8) list_terms<8, NV>(cx, row, idx, val, val2, e, bv, bv2);
        for (; e < e_hi; ++e) list_terms<1, NV>(cx, row, idx, val, val2, e, bv, bv2);
        double v[NV];
        v[0] = bv; v[1] = bv * bv;
        if constexpr (NV == 5) { v[2] = bv2; v[3] = bv2 * bv2; v[4] = bv * bv2; }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
            if (lane == 0) red[k][wave] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < NV)
            partial[((int64_t)w * gridDim.x + blockIdx.x) * NV + threadIdx.x] =
                ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
        __syncthreads();
    }
}

// out[v * nwin + w] = sum over the slices (fixed order) of value v of window w.  (A template only to live in this header.)
template <int = 0>
__global__ __launch_bounds__(256) void k_window_reduce(int nwin, int nslices, int nv, const double* __restrict__ partial, double* __restrict__ out)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nwin) return;
    for (int v = 0; v < nv; ++v) {
        double s = 0.0;
        for (int k = 0; k < nslices; ++k) s += partial[((int64_t)w * nslices + k) * nv + v];
        out[(int64_t)v * nwin + w] = s;
    }
}

// ---- the GWAS session (jwas_hip_gwas_begin / _sample / _local_ebv; GWAS.jl:149-173) ---------------------------------------------
// One saved sample is ONE ascending (idx, val) list; entry 0 of the session is "all markers" (genVar, GWAS.jl:155), entry 1 + w is
// window w = the columns [cs[w], ce[w]).
// k_gwas_slices: the slice [lo, hi) of the list that falls into every entry (lower bounds, numpy's searchsorted).
// grid = cld(nent, 256), block = 256.  (A template only to live in this header.)
template <int = 0>
__global__ __launch_bounds__(256) void k_gwas_slices(int nent, int nnz, const int32_t* __restrict__ cs, const int32_t* __restrict__ ce,
                                                     const int32_t* __restrict__ idx, int32_t* __restrict__ lo, int32_t* __restrict__ hi)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nent) return;
    if (t == 0) { lo[0] = 0; hi[0] = nnz; return; }
    auto lower = [&](int32_t key) {
        int a = 0, b = nnz;
        while (a < b) { const int m = (a + b) >> 1; if (idx[m] < key) a = m + 1; else b = m; }
        return a;
    };
    lo[t] = lower(cs[t - 1]);
    hi[t] = lower(ce[t - 1]);
}

// k_gwas_partial: k_window_partial over a grid of row slices x entry chunks.  grid = (nslices, nchunks), block = 256 (one
// individual per thread, so a column load is one coalesced instruction per wave); chunk 0 is entry 0 alone (its list is as long as
// all disjoint windows together), chunk 1 + k holds the windows [k wpc, (k + 1) wpc).  A thread keeps 16 / 4 / 1 column loads of an
// entry's list in flight and adds them in list order; the slice's (sum, sum of squares) are reduced as in k_window_partial into
// partial[(entry * nslices + slice) * 2 + {0, 1}] and the slices are added by k_window_reduce: the bits of jwas_hip_window_sums.
// LEBV: acc[w * ld_acc + row] += BV_w[row], the running SUM of the local EBVs (GWAS.jl:159-164; divided by the sample count on
// read-out); one owner per element, no atomics; an entry without a nonzero effect in this sample adds 0 and is skipped.
template <class CX, bool LEBV>
__global__ __launch_bounds__(256) void k_gwas_partial(CX cx, int nent, int wpc, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                      const int32_t* __restrict__ idx, const elem_t<CX>* __restrict__ val, double* __restrict__ partial,
                                                      double* __restrict__ acc, int64_t ld_acc)
{
    __shared__ double red[2][4];
    const int64_t row = (int64_t)blockIdx.x * kSliceRows + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w0 = blockIdx.y == 0 ? 0 : 1 + ((int)blockIdx.y - 1) * wpc;
    const int w1 = blockIdx.y == 0 ? 1 : (w0 + wpc < nent ? w0 + wpc : nent);
    for (int w = w0; w < w1; ++w) {
        double bv = 0.0;
        const int e_lo = lo[w], e_hi = hi[w];
        list_sum(cx, row, idx, val, e_lo, e_hi, bv);
        if constexpr (LEBV) { if (w >= 1 && e_hi > e_lo) acc[(int64_t)(w - 1) * ld_acc + row] += bv; }
        double v[2];
        v[0] = bv; v[1] = bv * bv;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
            if (lane == 0) red[k][wave] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 2)
            partial[((int64_t)w * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
                ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
        __syncthreads();
    }
}

}  // namespace jw

// Run f(cols) with the accessor of the Float32 context's storage (columns from j_off on).
template <class F>
static auto with_cols(jwas_hip_ctx* c, int64_t j_off, F&& f)
{
    using namespace jw;
    if (c->packed) return f(PackedCols{c->Q + j_off * (c->ld >> 2), c->ld, c->qmean + j_off, c->n, c->centered, c->w, (int32_t)c->weighted});
    return f(DenseCols{c->X + j_off * c->ld, c->ld, c->w, (int32_t)c->weighted});
}
