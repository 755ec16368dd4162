// marker_state.hpp -- what the sessions with a sweep of their own (session_rrm.hip, session_mega.hip) do with their MarkerState
// (ctx.hpp): allocation and the starting values, set and get of a range of rows, the running means and the product X alpha of a row.
// Host functions on ctx.hpp's plumbing, and their two kernels: templates, so that every unit that includes this header may
// instantiate them (a non-template __global__ here would be a duplicate host symbol at link time).
#pragma once
#include "ctx.hpp"

namespace jwms {

// running mean, mean of squares and model frequency of every effect (output.jl:556-560): one thread per (row, marker).  delta holds
// 0 / 1, or with kClassFrequency the class 1..4 of a BayesR chain: the model frequency is then that of class > 1.
template <bool kClassFrequency>
__global__ __launch_bounds__(256) void k_state_accumulate(const double* __restrict__ alpha, const double* __restrict__ delta, int64_t count, double ns,
                                                          double* __restrict__ mean_a, double* __restrict__ mean_a2, double* __restrict__ mean_d)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double a = alpha[i];
    mean_a[i] = jwu::running_mean(mean_a[i], a, ns);
    mean_a2[i] = jwu::running_mean(mean_a2[i], a * a, ns);
    mean_d[i] = jwu::running_mean(mean_d[i], kClassFrequency ? (delta[i] > 1.0 ? 1.0 : 0.0) : delta[i], ns);
}

// out[i] = sum_j x_ij alpha_j (j ascending, zero effects skipped): one thread per row of X (the context's matrix or its output rows)
template <class real>
__global__ __launch_bounds__(256) void k_mul_alpha(const real* __restrict__ X, int64_t ld, int64_t n, int64_t p, const double* __restrict__ alpha,
                                                   double* __restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    double s = 0.0;
    for (int64_t j = 0; j < p; ++j) {
        const double a = alpha[j];
        if (a != 0.0) s = s + (double)X[j * ld + row] * a;
    }
    out[row] = s;
}

}  // namespace jwms

// the six arrays into the session's owner; alpha, beta and the means start at 0, delta at ones (Mi.δ, MCMC_BayesianAlphabet.jl:85-117)
static inline int marker_state_begin(jwas_hip_ctx* c, MarkerState& m, DevOwner& owner, int rows, const char* name, void (*free_session)(jwas_hip_ctx*))
{
    const size_t count = (size_t)rows * (size_t)c->p, bytes = sizeof(double) * count;
    for (double** q : {&m.alpha, &m.beta, &m.delta, &m.mean_a, &m.mean_a2, &m.mean_d})
        if (int rc = alloc_or_nomem(c, owner, q, bytes, name, free_session)) return rc;
    for (double* q : {m.alpha, m.beta, m.mean_a, m.mean_a2, m.mean_d}) HIPCHK(c, hipMemsetAsync(q, 0, bytes, c->stream));
    const std::vector<double> ones(count, 1.0);
    HIPCHK(c, hipMemcpyAsync(m.delta, ones.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// rows [row0, row0 + rows) of up to three of the state's arrays -> the host
static inline int marker_rows_get(jwas_hip_ctx* c, int64_t row0, int rows, const double* const (&dev)[3], double* const (&out)[3])
{
    const size_t at = (size_t)row0 * (size_t)c->p, bytes = sizeof(double) * (size_t)rows * (size_t)c->p;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 3; ++i)
        if (out[i]) HIPCHK(c, hipMemcpyAsync(out[i], dev[i] + at, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

static inline int marker_state_get(jwas_hip_ctx* c, const MarkerState& m, int64_t row0, int rows, double* alpha, double* beta, double* delta)
{
    return marker_rows_get(c, row0, rows, {m.alpha, m.beta, m.delta}, {alpha, beta, delta});
}

// (mean, mean of squares, model frequency) of one row
static inline int marker_state_posterior(jwas_hip_ctx* c, const MarkerState& m, int64_t row, double* mean, double* mean2, double* freq)
{
    return marker_rows_get(c, row, 1, {m.mean_a, m.mean_a2, m.mean_d}, {mean, mean2, freq});
}

// rows [row0, row0 + rows) of alpha, beta, delta (any may be NULL) from the host: every value finite, delta 0 or 1
static inline int marker_state_set(jwas_hip_ctx* c, MarkerState& m, int64_t row0, int rows, const double* alpha, const double* beta, const double* delta)
{
    const size_t cnt = (size_t)rows * (size_t)c->p, at = (size_t)row0 * (size_t)c->p;
    for (const double* src : {alpha, beta, delta})
        if (src)
            for (size_t i = 0; i < cnt; ++i) NEED(c, std::isfinite(src[i]), JWAS_HIP_EINVAL, "state value %zu is not finite (%g)", i, src[i]);
    if (delta)
        for (size_t i = 0; i < cnt; ++i) NEED(c, delta[i] == 0.0 || delta[i] == 1.0, JWAS_HIP_EINVAL, "delta[%zu] = %g is not 0 or 1", i, delta[i]);
    HIPCHK(c, hipSetDevice(c->device));
    if (alpha) HIPCHK(c, hipMemcpyAsync(m.alpha + at, alpha, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
    if (beta) HIPCHK(c, hipMemcpyAsync(m.beta + at, beta, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
    if (delta) HIPCHK(c, hipMemcpyAsync(m.delta + at, delta, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// the state joins the running means as sample number `nsamples`
template <bool kClassFrequency>
static inline int marker_state_accumulate(jwas_hip_ctx* c, MarkerState& m, int rows, double nsamples)
{
    NEED(c, nsamples >= 1.0, JWAS_HIP_EINVAL, "nsamples must be >= 1 (got %g)", nsamples);
    const int64_t count = (int64_t)rows * c->p;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(jwms::k_state_accumulate<kClassFrequency>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, (const double*)m.alpha,
                       (const double*)m.delta, count, nsamples, m.mean_a, m.mean_a2, m.mean_d);
    HIPCHK(c, hipGetLastError());
    return JWAS_HIP_OK;
}

// out[0 .. n) = X alpha_row for the n rows of X ([p][ld], the context's element type); dev_row: at least n doubles on the device
static inline int marker_state_mul_alpha(jwas_hip_ctx* c, const MarkerState& m, int64_t row, const void* X, int64_t ld, int64_t n, double* dev_row, double* out)
{
    with_real(c, [&](auto real) {
        using real_t = decltype(real);
        hipLaunchKernelGGL(jwms::k_mul_alpha<real_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const real_t*)X, ld, n, c->p,
                           (const double*)(m.alpha + (size_t)row * (size_t)c->p), dev_row);
    });
    HIPCHK(c, hipGetLastError());
    return to_host(c, out, dev_row, sizeof(double) * (size_t)n);
}
