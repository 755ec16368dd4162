// locpar.hpp -- the non-marker location parameters (intercepts, covariates, fixed and i.i.d. random class factors) on the device.
//
// Step 1 of the reference's iteration (MCMC/MCMC_BayesianAlphabet.jl:193-220) adds X sol to the residual, forms X'Ri ycorr and runs
// the single-site scan Gibbs(A, x, b[, vare]) (iterative_solver/solver.jl:143-162) over the mixed model equations, then subtracts
// X sol again.  The levels of ONE term partition the records, so X_term' W X_term is diagonal and, given the other terms, the
// levels of a term with a diagonal prior are conditionally independent: sampling a whole term at once and updating the residual
// IS that scan, written in residual-update form.  The only serial dependence is term after term; a term is three short launches.
//
// For level l of a term of trait k (c = inv(R); one trait: c = 1), d_l = sum_{i in l} w_i x_i^2 formed once at set-up:
//   rho_i  = sum_m c_km r_m,i                                  (one trait: r_i)
//   S_l    = sum_{i in l} w_i x_i rho_i
//   lhs_l  = d_l c_kk + prior                                  prior = vare Gi (one trait, the lambda form of random_effects.jl:232),
//                                                                      Gi_kk (several traits), 0 (a fixed term)
//   mean_l = (S_l + d_l c_kk sol_l - sum_{m != k} Gi_km u_m,l) / lhs_l
//   sol_l' = mean_l + z sqrt(s / lhs_l)                        s = vare (one trait), 1 (several); lhs_l == 0: left alone (solver.jl:145)
//   r_k,i  = T(double(r_k,i) - x_i (sol_l' - sol_l))            one rounding per term
// z: rng.hpp's Box-Muller normal on the counter (level within its term, iteration, 0x20000000 | term ordinal, 3 + 16 trait).
//
// LAYOUT of a term (built on the host when the term is added): the records sorted by level, ties by ascending record; every level
// cut into PIECES of at most kPiece consecutive records of that order; a lane-group width G (a power of two <= 64, from the mean
// piece length).  k_locpar_sums gives a piece to G lanes: lane g adds records g, g + G, ... of the piece in that order, the G
// partial sums are combined by a butterfly (__shfl_xor, offsets G/2 .. 1); k_locpar_draw adds the pieces of a level in piece
// order.  The order of every addition is fixed by the layout alone -- no floating-point atomics, two runs give identical bits.
//
//   k_locpar_sums<T>      piece sums of w x rho        (T = float | double: the residual's element type; arithmetic in double)
//   k_locpar_draw         one thread per level: S_l, the draw, sol, delta_l = sol_l' - sol_l
//   k_locpar_apply<T>     one thread per record: r_k,i -= x_i delta[level_i]      (coalesced)
//   k_locpar_cross        U'U of a random effect: one workgroup per pair of member terms, a fixed strided order
//   k_locpar_accumulate   running means of sol and sol^2 (output.jl:556-560)
//
// A STRUCTURED random effect (jwas_hip_lp_set_group_structure: the polygenic effect of set_random(model, "animal", ped, G), whose
// levels have covariance inv(V) (x) G, V = the sparse A-inverse).  The data sums S_l are the ones above; only the prior couples levels:
//   lhs_l  = d_l c_kk + p_kk V_ll                              p_km = vare Gi_km (one trait), Gi_km (several)
//   mean_l = (S_l + d_l c_kk sol_l - sum_m p_km sum_j V_lj u_m,j) / lhs_l        (the sum over j skips j == l for m == k)
//   sol_l' = mean_l + z sqrt(s / lhs_l)                        (lhs_l > 0 always: V_ll > 0, p_kk > 0)
// Two levels that are not neighbours in V are conditionally independent, so the graph of V is coloured on the host (levels in
// ascending order, the smallest colour no neighbour holds) and the colours are visited in order, one launch of
// k_locpar_draw_structured per colour: a systematic-scan Gibbs sampler with a fixed visiting order.  u_k is read from sol in
// place -- earlier colours hold their new values, later ones their old ones; launch order is the only synchronisation.
// LAYOUT of a colour: its levels with at most kLongRow entries in their row of V in ascending order (one THREAD each: the row is
// added entry by entry in column order), then its levels with longer rows in ascending order (one WAVE each: lane g adds entries
// g, g + 64, ... of the row, the 64 partial sums meet in the butterfly 32 .. 1).  Fixed by the layout: identical bits run to run.
//   k_locpar_draw_structured    one launch per colour: S_l, the prior sums, the draw, sol, delta
//   k_locpar_quad_rows          u_a' V u_b, a <= b: 256 rows of V per workgroup (a thread per short row, the workgroup per long row), a fixed tree
//   k_locpar_quad_reduce        one workgroup adds the per-workgroup sums (strided, then the same tree) and fills the k x k block
//
// PER-RECORD WEIGHTS (mtmiss.hpp: multi-trait records that miss some traits; mkRi / getRi, residual.jl:2-44).  Record i carries a
// code (bit m set = trait m observed) and C[code] = inv(R[o,o]) embedded in a t x t matrix of zeros replaces inv(R):
//   rho_i  = sum_m C[code_i]_km r_m,i
//   S_l    = sum_{i in l} w_i x_i rho_i                        D_l = sum_{i in l} (w_i x_i) x_i C[code_i]_kk
//   lhs_l  = D_l + prior                                       mean_l = (S_l + D_l sol_l - ...) / lhs_l,  s = 1
// k_locpar_sums<T, true> forms the piece sums of S and of D side by side (the same piece / lane / butterfly order), the draws'
// <true> instantiations add the pieces of D in piece order where the plain ones form d_l c_kk.  A level whose records all miss
// trait k has D_l = 0: with no prior it is left alone.  The <false> instantiations are the plain code, unchanged.
#pragma once
#include "device_util.hpp"
#include "rng.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jwp {

constexpr int kPiece = 1024;            // records per piece  (kMaxT, kMaxGroups: device_util.hpp)
constexpr int kLongRow = 32;            // a row of a structure with more entries than this gets a wave, not a thread
constexpr int kMaxPairs = kMaxT * (kMaxT + 1) / 2;

struct SumArgs {
    const void* r;                      // [nt][ld] residuals (T)
    int64_t ld;
    const int32_t* rec;                 // [nin] records of the term, sorted by (level, record); NULL: 0 .. n - 1 (one level)
    const double* wx;                   // [nin] w_i x_i in that order
    const int32_t* piece_lo;            // [npieces + 1] piece p = entries piece_lo[p] .. piece_lo[p + 1] of rec / wx
    double* part;                       // [npieces] out
    int32_t npieces, G, nt, trait;
    double c[kMaxT];                    // row `trait` of inv(R) (one trait: {1})
    // per-record weights (kPat) only:
    const int32_t* code;                // [n] the pattern of every record
    const double* ctab;                 // [2^nt][nt][nt] C[code]
    const double* x;                    // [n] covariate values (NULL: ones)
    double* part2;                      // [npieces] out: piece sums of (w x) x C[code]_kk
};

template <class T, bool kPat = false>
__global__ __launch_bounds__(256) void k_locpar_sums(const SumArgs A)
{
    const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int G = A.G;
    const int64_t p = gt / G;
    const int g = (int)(gt % G);
    const bool valid = p < A.npieces;
    double acc = 0.0, acc2 = 0.0;
    if (valid) {
        const int lo = A.piece_lo[p], hi = A.piece_lo[p + 1];
        for (int j = lo + g; j < hi; j += G) {
            const int64_t i = A.rec ? A.rec[j] : j;
            double rho;
            if constexpr (kPat) {
                const double* crow = A.ctab + ((size_t)A.code[i] * A.nt + A.trait) * A.nt;
                rho = 0.0;
                for (int m = 0; m < A.nt; ++m) rho = rho + crow[m] * (double)((const T*)A.r)[(size_t)m * A.ld + i];
                acc2 = acc2 + (A.wx[j] * (A.x ? A.x[i] : 1.0)) * crow[A.trait];
            } else if (A.nt == 1) {
                rho = (double)((const T*)A.r)[i];
            } else {
                rho = 0.0;
                for (int m = 0; m < A.nt; ++m) rho = rho + A.c[m] * (double)((const T*)A.r)[(size_t)m * A.ld + i];
            }
            acc = acc + A.wx[j] * rho;
        }
    }
    for (int off = G >> 1; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);      // (groups are aligned to G: never leaves one)
    if (valid && g == 0) A.part[p] = acc;
    if constexpr (kPat) {
        for (int off = G >> 1; off >= 1; off >>= 1) acc2 = acc2 + __shfl_xor(acc2, off, 64);
        if (valid && g == 0) A.part2[p] = acc2;
    }
}

struct DrawArgs {
    const double* part;                 // [npieces]
    const int32_t* level_piece;         // [nlevels + 1] pieces of level l: level_piece[l] .. level_piece[l + 1]
    const double* d;                    // [nlevels]
    double* sol;                        // the whole solution vector
    double* delta;                      // [nlevels] out
    int64_t off;                        // this term's first entry of sol
    int64_t partner_off[kMaxT];         // random effect: the member terms' first entries, this term's own included (slot `pos`, skipped)
    double gi[kMaxT];                   // ... and row `pos` of Gi
    int32_t nlevels, npartners, pos;
    double ckk, prior, s;               // lhs = d ckk + prior, sd = sqrt(s / lhs)
    uint32_t iter, rep, slot, seed_lo, seed_hi;
    const double* part2;                // [npieces] per-record weights (kPat) only: the piece sums of D
};

template <bool kPat = false>
__global__ __launch_bounds__(256) void k_locpar_draw(const DrawArgs A)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= A.nlevels) return;
    double S = 0.0;
    for (int p = A.level_piece[l]; p < A.level_piece[l + 1]; ++p) S = S + A.part[p];
    double dc;
    if constexpr (kPat) {
        dc = 0.0;
        for (int p = A.level_piece[l]; p < A.level_piece[l + 1]; ++p) dc = dc + A.part2[p];
    } else {
        dc = A.d[l] * A.ckk;
    }
    const double lhs = dc + A.prior;
    const double old = A.sol[A.off + l];
    double delta = 0.0;
    if (lhs != 0.0) {                                                       // (solver.jl:145: zero diagonals are skipped)
        double num = S + dc * old;
        for (int m = 0; m < A.npartners; ++m)
            if (m != A.pos) num = num - A.gi[m] * A.sol[A.partner_off[m] + l];
        const double mean = num / lhs;
        const jw::u32x4 w = jw::philox4x32_10((uint32_t)l, A.iter, A.rep, A.slot, A.seed_lo, A.seed_hi);
        const double u1 = jw::u52(w.x, w.y), u2 = jw::u52(w.z, w.w);
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
        const double now = mean + z * sqrt(A.s / lhs);
        A.sol[A.off + l] = now;
        delta = now - old;
    }
    A.delta[l] = delta;
}

// r_k,i -= x_i delta[level_i]; x == NULL: 1, level == NULL: level 0 (intercept / covariate), level < 0: the record is in no level
template <class T>
__global__ __launch_bounds__(256) void k_locpar_apply(T* __restrict__ r, const double* __restrict__ x, const int32_t* __restrict__ level,
                                                      const double* __restrict__ delta, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = level ? level[i] : 0;
    if (l < 0) return;
    const double dl = delta[l];
    if (dl == 0.0) return;
    r[i] = (T)((double)r[i] - (x ? x[i] : 1.0) * dl);
}

// out[blockIdx.x] = sum_l a[l] b[l]; pair q = blockIdx.x reads offs[2 q], offs[2 q + 1].  Thread j adds levels j, j + 256, ... in
// that order, the 256 partial sums meet in a fixed tree.
__global__ __launch_bounds__(256) void k_locpar_cross(const double* __restrict__ sol, const int64_t* __restrict__ offs, int32_t nlevels,
                                                      double* __restrict__ out)
{
    __shared__ double sh[256];
    const double* a = sol + offs[2 * blockIdx.x];
    const double* b = sol + offs[2 * blockIdx.x + 1];
    double acc = 0.0;
    for (int l = threadIdx.x; l < nlevels; l += 256) acc = acc + a[l] * b[l];
    const double tot = jwu::tree256(sh, acc);
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_locpar_accumulate(const double* __restrict__ sol, double* __restrict__ mean, double* __restrict__ mean2,
                                                           int64_t q, double nsamples)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= q) return;
    const double v = sol[i];
    mean[i] = jwu::running_mean(mean[i], v, nsamples);
    mean2[i] = jwu::running_mean(mean2[i], v * v, nsamples);
}

struct StructDrawArgs {
    const double* part;                 // [npieces]
    const int32_t* level_piece;         // [nlevels + 1]
    const double* d;                    // [nlevels]
    double* sol;
    double* delta;                      // [nlevels] out (the levels of this colour)
    const int64_t* rowptr;              // [nlevels + 1] the structure V: CSR, columns ascending
    const int32_t* col;
    const double* val;
    const int32_t* lv;                  // the levels of this colour: nshort short rows, then nlong long rows
    int64_t off;                        // this term's first entry of sol
    int64_t partner_off[kMaxT];         // the member terms' first entries, this term's own included (slot `pos`)
    double p[kMaxT];                    // row `pos` of Gi, times vare in a single-trait model
    int32_t nshort, nlong, npartners, pos;
    double ckk, s;
    uint32_t iter, rep, slot, seed_lo, seed_hi;
    const double* part2;                // [npieces] per-record weights (kPat) only: the piece sums of D
};

// the draw of level l given the prior sums P[m] = sum_j V_lj u_m,j (own member: without j == l) and the diagonal vll
template <bool kPat>
__device__ inline void locpar_structured_finish(const StructDrawArgs& A, int l, const double* P, double vll)
{
    double S = 0.0;
    for (int q = A.level_piece[l]; q < A.level_piece[l + 1]; ++q) S = S + A.part[q];
    double dc;
    if constexpr (kPat) {
        dc = 0.0;
        for (int q = A.level_piece[l]; q < A.level_piece[l + 1]; ++q) dc = dc + A.part2[q];
    } else {
        dc = A.d[l] * A.ckk;
    }
    const double lhs = dc + A.p[A.pos] * vll;
    const double old = A.sol[A.off + l];
    double num = S + dc * old;
#pragma unroll
    for (int m = 0; m < kMaxT; ++m)
        if (m < A.npartners) num = num - A.p[m] * P[m];
    const double mean = num / lhs;
    const jw::u32x4 w = jw::philox4x32_10((uint32_t)l, A.iter, A.rep, A.slot, A.seed_lo, A.seed_hi);
    const double z = jwu::normal_from(w);
    const double now = mean + z * sqrt(A.s / lhs);
    A.sol[A.off + l] = now;
    A.delta[l] = now - old;
}

// grid: ceil(nshort / 256) workgroups of one thread per short row, then ceil(nlong / 4) workgroups of one wave per long row
template <bool kPat = false>
__global__ __launch_bounds__(256) void k_locpar_draw_structured(const StructDrawArgs A)
{
    const int nshort_wg = (A.nshort + 255) / 256;
    double P[kMaxT] = {0.0, 0.0, 0.0, 0.0};
    double vll = 0.0;
    if ((int)blockIdx.x < nshort_wg) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= A.nshort) return;
        const int l = A.lv[i];
        for (int64_t e = A.rowptr[l]; e < A.rowptr[l + 1]; ++e) {
            const int j = A.col[e];
            const double v = A.val[e];
            if (j == l) vll = v;
#pragma unroll
            for (int m = 0; m < kMaxT; ++m)
                if (m < A.npartners && !(j == l && m == A.pos)) P[m] = P[m] + v * A.sol[A.partner_off[m] + j];
        }
        locpar_structured_finish<kPat>(A, l, P, vll);
    } else {
        const int i = ((int)blockIdx.x - nshort_wg) * 4 + (int)(threadIdx.x >> 6);          // (wave-uniform)
        if (i >= A.nlong) return;
        const int lane = threadIdx.x & 63;
        const int l = A.lv[A.nshort + i];
        for (int64_t e = A.rowptr[l] + lane; e < A.rowptr[l + 1]; e += 64) {
            const int j = A.col[e];
            const double v = A.val[e];
            if (j == l) vll = v;
#pragma unroll
            for (int m = 0; m < kMaxT; ++m)
                if (m < A.npartners && !(j == l && m == A.pos)) P[m] = P[m] + v * A.sol[A.partner_off[m] + j];
        }
        for (int off = 32; off >= 1; off >>= 1) {
            vll = vll + __shfl_xor(vll, off, 64);                                          // (one lane holds V_ll, the others 0)
#pragma unroll
            for (int m = 0; m < kMaxT; ++m) P[m] = P[m] + __shfl_xor(P[m], off, 64);
        }
        if (lane == 0) locpar_structured_finish<kPat>(A, l, P, vll);
    }
}

struct QuadArgs {
    const double* sol;
    const int64_t* rowptr;
    const int32_t* col;
    const double* val;
    double* part;                       // [nwg][kMaxPairs]: pair (a, b), a <= b, at locpar_pair(a, b)
    int64_t member_off[kMaxT];
    int32_t nlevels, k;
};

__host__ __device__ inline int locpar_pair(int a, int b) { return a * kMaxT - a * (a - 1) / 2 + (b - a); }      // a <= b < kMaxT

// Workgroup w owns rows 256 w .. 256 w + 255.  A row of at most kLongRow entries is added by its own thread, entry by entry; a longer
// one by the whole workgroup afterwards (the long rows in ascending order; thread j adds entries j, j + 256, ... of the row).  Every
// thread ends with one partial sum per pair (a, b); the 256 of them meet in a fixed tree.
__global__ __launch_bounds__(256) void k_locpar_quad_rows(const QuadArgs A)
{
    __shared__ double sh[256];
    __shared__ int32_t is_long[256];
    const int l = blockIdx.x * 256 + threadIdx.x;
    double acc[kMaxPairs];
#pragma unroll
    for (int q = 0; q < kMaxPairs; ++q) acc[q] = 0.0;
    bool lng = false;
    if (l < A.nlevels) {
        const int64_t lo = A.rowptr[l], hi = A.rowptr[l + 1];
        lng = hi - lo > kLongRow;
        if (!lng) {
            double Vu[kMaxT] = {0.0, 0.0, 0.0, 0.0};
            for (int64_t e = lo; e < hi; ++e) {
                const int j = A.col[e];
                const double v = A.val[e];
#pragma unroll
                for (int m = 0; m < kMaxT; ++m)
                    if (m < A.k) Vu[m] = Vu[m] + v * A.sol[A.member_off[m] + j];
            }
#pragma unroll
            for (int a = 0; a < kMaxT; ++a)
#pragma unroll
                for (int b = a; b < kMaxT; ++b)
                    if (b < A.k) acc[locpar_pair(a, b)] = A.sol[A.member_off[a] + l] * Vu[b];
        }
    }
    is_long[threadIdx.x] = lng ? 1 : 0;
    __syncthreads();
    for (int i = 0; i < 256; ++i) {
        if (!is_long[i]) continue;                                                         // (uniform)
        const int row = blockIdx.x * 256 + i;
        double Vu[kMaxT] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t e = A.rowptr[row] + threadIdx.x; e < A.rowptr[row + 1]; e += 256) {
            const int j = A.col[e];
            const double v = A.val[e];
#pragma unroll
            for (int m = 0; m < kMaxT; ++m)
                if (m < A.k) Vu[m] = Vu[m] + v * A.sol[A.member_off[m] + j];
        }
#pragma unroll
        for (int a = 0; a < kMaxT; ++a)
#pragma unroll
            for (int b = a; b < kMaxT; ++b)
                if (b < A.k) acc[locpar_pair(a, b)] = acc[locpar_pair(a, b)] + A.sol[A.member_off[a] + row] * Vu[b];
    }
#pragma unroll
    for (int a = 0; a < kMaxT; ++a)
#pragma unroll
        for (int b = a; b < kMaxT; ++b) {
            if (b >= A.k) continue;                                                        // (uniform)
            const double tot = jwu::tree256(sh, acc[locpar_pair(a, b)]);
            if (threadIdx.x == 0) A.part[(size_t)blockIdx.x * kMaxPairs + locpar_pair(a, b)] = tot;
        }
}

// out: the k x k block of utu (row-major, both triangles) from the nwg per-workgroup sums
__global__ __launch_bounds__(256) void k_locpar_quad_reduce(const double* __restrict__ part, int32_t nwg, int32_t k, double* __restrict__ out)
{
    __shared__ double sh[256];
    for (int a = 0; a < k; ++a)
        for (int b = a; b < k; ++b) {
            const double tot = jwu::ordered_sum256(sh, part + locpar_pair(a, b), kMaxPairs, nwg);
            if (threadIdx.x == 0) { out[a * k + b] = tot; out[b * k + a] = tot; }
        }
}

}  // namespace jwp
