// output.hip -- the output side of a context: state, residual, posterior, x'x and marker-covariance transfer, the running means,
// X alpha on training and output rows, sparse samples, the window sums of the GWAS and its session.  One body per job, templated on the
// element type T of the half of the context it works on (ctx.hpp: Side<T>); the extern "C" pairs NAME / NAME_f64 are its two wrappers.
// Kernels: output.hpp.
#define JW_PLAIN_KERNEL static
#include "output.hpp"

#include <cstring>
#include <type_traits>

using namespace jw;

namespace {

// What every entry point of element type T checks first, in the order of its precision: a Float32 entry point names its twin to a
// Float64 context before it looks at its arguments (twin: "NAME (use NAME_f64)"), a Float64 one looks at them first.
template <class T>
int entry_guard(jwas_hip_ctx* c, bool args_ok, const char* null_message, const char* twin)
{
    if constexpr (std::is_same<T, float>::value) { if (c) NOT_F64(c, twin); }
    NEED(c, c && args_ok, JWAS_HIP_EINVAL, "%s", null_message);
    if constexpr (std::is_same<T, double>::value) ONLY_F64(c);
    return JWAS_HIP_OK;
}
#define GUARD(T, c, args_ok, null_message, twin) do { if (int rc_ = entry_guard<T>(c, args_ok, null_message, twin)) return rc_; } while (0)

template <class T> constexpr const char* load_output_name() { return sizeof(T) == 8 ? "jwas_hip_load_output_dense_f64" : "jwas_hip_load_output_dense_f32"; }

bool have_genotypes(jwas_hip_ctx* c) { return IS_F64(c) ? c->f64->X != nullptr : HAVE_STORAGE(c); }

// output rows are resident: dense, or (Float32) 2-bit packed
bool have_output_rows(jwas_hip_ctx* c, Side<float>& S) { return S.Xout != nullptr || c->Qout != nullptr; }
bool have_output_rows(jwas_hip_ctx*, Side<double>& S) { return S.Xout != nullptr; }

// the packed output rows as a view: the training set's means and centring, and n_out rows -- the pad-row mask is the view's
PackedCols packed_output_view(jwas_hip_ctx* c) { return PackedCols{c->Qout, c->ld_out, c->qmean, c->n_out, c->centered, nullptr, 0}; }

// f(view) of the training rows (the context's storage) or of the output rows
template <class F>
auto with_view(jwas_hip_ctx* c, Side<float>& S, bool out_rows, F&& f)
{
    if (out_rows && c->Qout) return f(packed_output_view(c));
    if (out_rows) return f(DenseCols{S.Xout, S.ld_out, nullptr, 0});
    return with_cols(c, 0, f);
}
template <class F>
auto with_view(jwas_hip_ctx* c, Side<double>& S, bool out_rows, F&& f)
{
    return out_rows ? f(DenseCols64{S.Xout, S.ld_out}) : f(DenseCols64{S.X, c->ld});
}

// ---- transfer ------------------------------------------------------------------------------------------------------------------------
// up to three [p] vectors of one trait, host <-> device; the third: T at the trait's offset, or (classes) the int32 classes of a
// BayesR chain
template <class T>
int state_copy(jwas_hip_ctx* c, int32_t trait, const void* a, const void* b, const void* d, T* dev_a, T* dev_b, void* dev_d, bool classes, bool to_device)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb = sizeof(T) * c->p, off = (size_t)trait * c->p;
    void* dev[3] = {dev_a + off, dev_b + off, classes ? dev_d : (void*)((T*)dev_d + off)};
    const void* host[3] = {a, b, d};
    const size_t bytes[3] = {nb, nb, classes ? sizeof(int32_t) * c->p : nb};
    for (int i = 0; i < 3; ++i) {
        if (!host[i]) continue;
        if (to_device) HIPCHK(c, hipMemcpyAsync(dev[i], host[i], bytes[i], hipMemcpyHostToDevice, c->stream));
        else HIPCHK(c, hipMemcpyAsync(const_cast<void*>(host[i]), dev[i], bytes[i], hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

template <class T>
int state_io(jwas_hip_ctx* c, int32_t trait, const void* a, const void* b, const void* d, bool to_device, const char* twin)
{
    GUARD(T, c, true, "ctx is NULL", twin);
    NEED_TRAIT(c, trait);
    auto& S = side<T>(c);
    return state_copy<T>(c, trait, a, b, d, S.alpha, S.beta, S.delta, c->method == JWAS_HIP_BAYESR, to_device);
}

template <class T>
int get_posterior(jwas_hip_ctx* c, int32_t trait, T* ma, T* ma2, T* md)
{
    GUARD(T, c, true, "ctx is NULL", "jwas_hip_get_posterior (use jwas_hip_get_posterior_f64)");
    NEED_TRAIT(c, trait);
    auto& S = side<T>(c);
    return state_copy<T>(c, trait, ma, ma2, md, S.mean_a, S.mean_a2, S.mean_d, false, false);
}

template <class T>
int residual_io(jwas_hip_ctx* c, int32_t trait, const T* in, T* out, const char* twin)
{
    GUARD(T, c, in || out, "NULL argument", twin);
    NEED_TRAIT(c, trait);
    HIPCHK(c, hipSetDevice(c->device));
    T* rk = side<T>(c).r + (size_t)trait * c->ld;
    if (in) HIPCHK(c, hipMemcpyAsync(rk, in, sizeof(T) * c->n, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemcpyAsync(out, rk, sizeof(T) * c->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

template <class T>
int get_xpx(jwas_hip_ctx* c, T* out)
{
    GUARD(T, c, out != nullptr, "NULL argument", "jwas_hip_get_xpx (use jwas_hip_get_xpx_f64)");
    NEED(c, side<T>(c).xpx, JWAS_HIP_ESTATE, "jwas_hip_setup_blocks has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, out, side<T>(c).xpx, sizeof(T) * c->p);
}

template <class T>
int get_marker_covariances(jwas_hip_ctx* c, T* out)
{
    GUARD(T, c, out != nullptr, "NULL argument", "jwas_hip_get_marker_covariances (use jwas_hip_get_marker_covariances_f64)");
    auto& S = side<T>(c);
    NEED(c, S.var_mat && S.var_mat_resident, JWAS_HIP_ESTATE, "no per-marker effect covariances are resident");
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, out, S.var_mat, sizeof(T) * (size_t)c->ntraits * c->ntraits * c->p);
}

// ---- X alpha -----------------------------------------------------------------------------------------------------------------------------
// The nonzero effects of trait `trait` as device lists in marker order (S.cmp_idx / S.cmp_val, owned by the context), compacted on
// the device; *nnz = their number.  A failed allocation leaves nothing half allocated.
template <class T>
hipError_t compact_alpha(jwas_hip_ctx* c, int32_t trait, int* nnz)
{
    auto& S = side<T>(c);
    hipError_t e = hipSuccess;
    if (!S.cmp_idx) {
        e = S.load_mem.alloc(&S.cmp_idx, sizeof(int32_t) * ((size_t)c->p + 1));
        if (e == hipSuccess) e = S.load_mem.alloc(&S.cmp_val, sizeof(T) * (size_t)c->p);
        if (e != hipSuccess) { S.load_mem.free_one(S.cmp_idx); return e; }
    }
    hipLaunchKernelGGL(k_compact_alpha<T>, dim3(1), dim3(1024), 0, c->stream, c->p, (const T*)(S.alpha + (size_t)trait * c->p), S.cmp_idx, S.cmp_val,
                       S.cmp_idx + c->p);
    e = hipGetLastError();
    int32_t cnt = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&cnt, S.cmp_idx + c->p, sizeof cnt, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    *nnz = (int)cnt;
    return e;
}

// out[0 .. n_rows) = M alpha_trait, M = the training or the output rows (leading dimension ld): over the compacted list, or
// (ListPolicy) over all markers when the effects are dense -- the same fma chain in marker order, hence the same bits
template <class T>
int mul_alpha_rows(jwas_hip_ctx* c, int32_t trait, bool out_rows, int64_t ld, int64_t n_rows, T* out, const char* who)
{
    typedef ListPolicy<T> P;
    auto& S = side<T>(c);
    HIPCHK(c, hipSetDevice(c->device));
    T* tmp = nullptr;
    HIPCHK(c, hipMalloc(&tmp, sizeof(T) * ld));
    int nnz = 0;
    hipError_t e = compact_alpha<T>(c, trait, &nnz);
    if (e == hipSuccess) {
        with_view(c, S, out_rows, [&](auto cx) {
            if constexpr (P::kDenseFallback) {
                if ((int64_t)nnz * 4 > c->p) {
                    hipLaunchKernelGGL((k_mul_alpha<decltype(cx)>), dim3((unsigned)(ld / kSliceRows)), dim3(256), 0, c->stream, cx, c->p,
                                       (const T*)(S.alpha + (size_t)trait * c->p), tmp);
                    return 0;
                }
            }
            hipLaunchKernelGGL((k_mul_alpha_list<decltype(cx), P::kRows>), dim3((unsigned)(ld / P::kRows)), dim3(P::kRows), 0, c->stream, cx, nnz,
                               (const int32_t*)S.cmp_idx, (const T*)S.cmp_val, tmp);
            return 0;
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, sizeof(T) * n_rows, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "%s: %s", who, hipGetErrorString(e));
    return JWAS_HIP_OK;
}

template <class T>
int mul_alpha(jwas_hip_ctx* c, int32_t trait, T* out, const char* who)
{
    GUARD(T, c, out != nullptr, "NULL argument", "jwas_hip_mul_alpha (use jwas_hip_mul_alpha_f64)");
    NEED_TRAIT(c, trait);
    return mul_alpha_rows<T>(c, trait, false, c->ld, c->n, out, who);
}

// EBV = output_genotypes * alpha for a saved sample (output.jl:281-306)
template <class T>
int mul_alpha_output(jwas_hip_ctx* c, int32_t trait, T* out, const char* who)
{
    GUARD(T, c, out != nullptr, "NULL argument", "jwas_hip_mul_alpha_output (use jwas_hip_mul_alpha_output_f64)");
    NEED_TRAIT(c, trait);
    auto& S = side<T>(c);
    NEED(c, have_output_rows(c, S), JWAS_HIP_ESTATE, "%s has not been called", load_output_name<T>());
    return mul_alpha_rows<T>(c, trait, true, S.ld_out, S.n_out, out, who);
}

// One saved marker-effect sample as a sparse record (output.jl:443-526 writes the dense text row; with a sparse prior a sample has a
// few hundred nonzero effects among 600 000).  idx / val: caller arrays of `capacity` entries, marker order; *nnz_out is filled even
// when they are too short (grow and call again).
template <class T>
int get_alpha_sparse(jwas_hip_ctx* c, int32_t trait, int64_t capacity, int32_t* idx, T* val, int64_t* nnz_out)
{
    GUARD(T, c, nnz_out != nullptr, "NULL argument", "jwas_hip_get_alpha_sparse (use jwas_hip_get_alpha_sparse_f64)");
    NEED_TRAIT(c, trait);
    HIPCHK(c, hipSetDevice(c->device));
    int nnz = 0;
    HIPCHK(c, compact_alpha<T>(c, trait, &nnz));
    *nnz_out = nnz;
    NEED(c, nnz <= capacity, JWAS_HIP_EINVAL, "%d nonzero effects do not fit the caller's %lld entries", nnz, (long long)capacity);
    if (nnz > 0) {
        NEED(c, idx && val, JWAS_HIP_EINVAL, "idx / val is NULL");
        HIPCHK(c, hipMemcpyAsync(idx, side<T>(c).cmp_idx, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(val, side<T>(c).cmp_val, sizeof(T) * nnz, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return JWAS_HIP_OK;
}

// Output rows: the reference keeps Mi.output_genotypes = Z_out * genotypes for mme.output_ID (all genotyped individuals by default,
// input_data_validation.jl:150-154; tools4genotypes.jl:290-296) next to the training rows: a second resident matrix; a second call
// replaces it, a load of genotypes and jwas_hip_destroy free it.
template <class T>
int load_output_dense(jwas_hip_ctx* c, const T* Xh, int64_t n_out, int64_t p, int64_t ld_host)
{
    GUARD(T, c, true, "ctx is NULL", "jwas_hip_load_output_dense_f32 (use jwas_hip_load_output_dense_f64)");
    NEED(c, Xh, JWAS_HIP_EINVAL, "X_out is NULL");
    NEED(c, have_genotypes(c), JWAS_HIP_ESTATE, "no genotype matrix loaded");
    NEED(c, n_out >= 1, JWAS_HIP_EINVAL, "n_out must be >= 1 (got %lld)", (long long)n_out);
    NEED(c, p == c->p, JWAS_HIP_EINVAL, "output genotypes have %lld markers, the training matrix %lld", (long long)p, (long long)c->p);
    NEED(c, ld_host >= n_out, JWAS_HIP_EINVAL, "ld_host (%lld) must be >= n_out (%lld)", (long long)ld_host, (long long)n_out);
    auto& S = side<T>(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if constexpr (std::is_same<T, float>::value) drop_output_rows(c);      // (dense or packed: at most one output matrix is resident)
    else { if (c->gw.out_rows) gwas_free(c); S.load_mem.free_one(S.Xout); S.n_out = S.ld_out = 0; }
    const int64_t ld = round_up(n_out, kSliceRows);
    HIPCHK(c, S.load_mem.alloc(&S.Xout, sizeof(T) * (size_t)ld * p));
    S.n_out = n_out; S.ld_out = ld;
    if (ld != n_out) HIPCHK(c, hipMemsetAsync(S.Xout, 0, sizeof(T) * (size_t)ld * p, c->stream));      // pad rows zero
    HIPCHK(c, hipMemcpy2DAsync(S.Xout, sizeof(T) * ld, Xh, sizeof(T) * ld_host, sizeof(T) * n_out, (size_t)p, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// The EBVs of all traits on packed output rows in one launch (k_ebv_packed): the union list, the kernel, [t][n_out] to the host.
int ebv_output_packed(jwas_hip_ctx* c, float* out)
{
    const int t = c->ntraits;
    const int64_t ld = c->ld_out, n_out = c->n_out;
    if (!c->ebv_idx) {
        hipError_t ea = c->load_mem.alloc(&c->ebv_idx, sizeof(int32_t) * ((size_t)c->p + 1));
        if (ea == hipSuccess) ea = c->load_mem.alloc(&c->ebv_val, sizeof(float) * (size_t)kMaxT * c->p);
        if (ea != hipSuccess) {
            (void)hipGetLastError();
            c->load_mem.free_one(c->ebv_idx); c->load_mem.free_one(c->ebv_val);
            return fail(c, JWAS_HIP_ENOMEM, "jwas_hip_ebv_output: %s (the list of the nonzero effects)", hipGetErrorString(ea));
        }
    }
    float* tmp = nullptr;
    HIPCHK(c, hipMalloc(&tmp, sizeof(float) * (size_t)t * ld));
    hipLaunchKernelGGL(k_compact_alpha_union<float>, dim3(1), dim3(1024), 0, c->stream, c->p, t, (const float*)c->alpha, c->ebv_idx, c->ebv_val, c->ebv_idx + c->p);
    hipError_t e = hipGetLastError();
    int32_t nnz = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&nnz, c->ebv_idx + c->p, sizeof nnz, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) {
        const PackedCols cx = packed_output_view(c);
        with_traits(t, [&](auto nt) {
            hipLaunchKernelGGL((k_ebv_packed<decltype(nt)::value>), dim3((unsigned)(ld / kSliceRows)), dim3(64), 0, c->stream, cx, (int)nnz,
                               (const int32_t*)c->ebv_idx, (const float*)c->ebv_val, c->p, tmp);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(out, sizeof(float) * (size_t)n_out, tmp, sizeof(float) * (size_t)ld, sizeof(float) * (size_t)n_out, (size_t)t, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "jwas_hip_ebv_output: %s", hipGetErrorString(e));
    return JWAS_HIP_OK;
}

// ---- window sums -----------------------------------------------------------------------------------------------------------------------
// Window genomic variances of one saved marker-effect sample: the O(samples x n x p) inner loop of the reference's window-based GWAS
// (src/3.GWAS/src/GWAS.jl:152-165: genVar = var(X*alpha), var_w = var(X[:, w] * alpha[w]); :199-217 for two traits' samples) as one
// launch over the nonzero effects only.  The caller derives var = (ss - sum^2/n) / (n - 1).
template <class T>
int window_sums(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx, const T* val, const T* val2,
                double* const* outs /* 2 or 5 arrays of nwin */, const char* who)
{
    const int nv = val2 ? 5 : 2;
    GUARD(T, c, true, "ctx is NULL", val2 ? "jwas_hip_window_sums2 (use jwas_hip_window_sums2_f64)" : "jwas_hip_window_sums (use jwas_hip_window_sums_f64)");
    auto& S = side<T>(c);
    NEED(c, wptr, JWAS_HIP_EINVAL, "NULL argument");
    for (int v = 0; v < nv; ++v) NEED(c, outs[v], JWAS_HIP_EINVAL, "NULL output array");
    NEED(c, nwin >= 1, JWAS_HIP_EINVAL, "nwin must be >= 1 (got %d)", nwin);
    NEED(c, have_genotypes(c), JWAS_HIP_ESTATE, "no genotype matrix loaded");
    NEED(c, !use_output_rows || have_output_rows(c, S), JWAS_HIP_ESTATE, "%s has not been called", load_output_name<T>());
    NEED(c, wptr[0] == 0, JWAS_HIP_EINVAL, "wptr[0] must be 0");
    for (int w = 0; w < nwin; ++w) NEED(c, wptr[w + 1] >= wptr[w], JWAS_HIP_EINVAL, "wptr must be non-decreasing");
    const int64_t nnz = wptr[nwin];
    NEED(c, nnz == 0 || (idx && val), JWAS_HIP_EINVAL, "idx / val is NULL");
    for (int64_t e = 0; e < nnz; ++e) NEED(c, idx[e] >= 0 && idx[e] < c->p, JWAS_HIP_EINVAL, "marker index %d out of range", idx[e]);
    HIPCHK(c, hipSetDevice(c->device));
    const int nsl = (int)((use_output_rows ? S.ld_out : c->ld) / kSliceRows);
    const size_t ne = (size_t)(nnz > 0 ? nnz : 1);
    int32_t *d_wptr = nullptr, *d_idx = nullptr; T *d_val = nullptr, *d_val2 = nullptr; double *d_part = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc(&d_wptr, sizeof(int32_t) * (nwin + 1));
    if (e == hipSuccess) e = hipMalloc(&d_idx, sizeof(int32_t) * ne);
    if (e == hipSuccess) e = hipMalloc(&d_val, sizeof(T) * ne);
    if (e == hipSuccess && val2) e = hipMalloc(&d_val2, sizeof(T) * ne);
    if (e == hipSuccess) e = hipMalloc(&d_part, sizeof(double) * nv * (size_t)nwin * nsl);
    if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * nv * (size_t)nwin);
    if (e == hipSuccess) e = hipMemcpyAsync(d_wptr, wptr, sizeof(int32_t) * (nwin + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(d_idx, idx, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(d_val, val, sizeof(T) * nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz && val2) e = hipMemcpyAsync(d_val2, val2, sizeof(T) * nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        with_view(c, S, use_output_rows != 0, [&](auto cx) {
            if (val2) hipLaunchKernelGGL((k_window_partial<decltype(cx), 5>), dim3((unsigned)nsl), dim3(256), 0, c->stream, cx, nwin, d_wptr, d_idx, d_val, d_val2, d_part);
            else      hipLaunchKernelGGL((k_window_partial<decltype(cx), 2>), dim3((unsigned)nsl), dim3(256), 0, c->stream, cx, nwin, d_wptr, d_idx, d_val, d_val2, d_part);
            return 0;
        });
        hipLaunchKernelGGL((k_window_reduce<>), dim3((unsigned)((nwin + 255) / 256)), dim3(256), 0, c->stream, nwin, nsl, nv, d_part, d_out);
        e = hipGetLastError();
    }
    for (int v = 0; v < nv && e == hipSuccess; ++v)
        e = hipMemcpyAsync(outs[v], d_out + (size_t)v * nwin, sizeof(double) * nwin, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_wptr); (void)hipFree(d_idx); (void)hipFree(d_val); (void)hipFree(d_val2); (void)hipFree(d_part); (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "%s: %s", who, hipGetErrorString(e));
    return JWAS_HIP_OK;
}

template <class T>
int window_sums2(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx, const T* val1, const T* val2,
                 double* const (&outs)[5], const char* who)
{
    GUARD(T, c, val2 != nullptr, "NULL argument", "jwas_hip_window_sums2 (use jwas_hip_window_sums2_f64)");
    return window_sums<T>(c, use_output_rows, nwin, wptr, idx, val1, val2, outs, who);
}

// ---- the GWAS session (src/3.GWAS/src/GWAS.jl:149-173) -----------------------------------------------------------------------------
// Window variances AND local EBVs of the saved samples with everything resident: the window ranges are uploaded once, a sample
// arrives as its (idx, val) list (no per-window duplicates), no allocation per sample.
constexpr int kGwasTargetWG = 2048;      // 256 CUs x 8 workgroups of 4 waves: every SIMD's 8 wave slots

int64_t gwas_windows_per_chunk(int64_t nwin, int64_t nsl)
{
    const int64_t wpc = (nwin * nsl + kGwasTargetWG - 1) / kGwasTargetWG;
    return wpc < 1 ? 1 : wpc;
}

// the matrix a session runs on (NULL: none), its rows and leading dimension
const void* gwas_matrix(jwas_hip_ctx* c, bool out_rows, int64_t* n_rows, int64_t* ld)
{
    if (out_rows) return output_rows_ptr(c, n_rows, ld);
    *n_rows = c->n; *ld = c->ld;
    return !IS_F64(c) && c->packed ? (const void*)c->Q : genotypes_ptr(c);
}

template <class T>
int gwas_sample(jwas_hip_ctx* c, int32_t nnz, const int32_t* idx, const T* val, double* out_sum, double* out_ss)
{
    GUARD(T, c, true, "ctx is NULL", "jwas_hip_gwas_sample (use jwas_hip_gwas_sample_f64)");
    auto& g = c->gw;
    NEED(c, out_sum && out_ss, JWAS_HIP_EINVAL, "NULL output array");
    NEED(c, nnz >= 0, JWAS_HIP_EINVAL, "nnz must be >= 0 (got %d)", nnz);
    NEED(c, nnz == 0 || (idx && val), JWAS_HIP_EINVAL, "idx / val is NULL");
    NEED(c, g.active, JWAS_HIP_ESTATE, "jwas_hip_gwas_begin has not been called");
    int64_t n_rows = 0, ld = 0;
    NEED(c, gwas_matrix(c, g.out_rows, &n_rows, &ld) == g.mat && ld == g.ld && n_rows == g.n_rows, JWAS_HIP_ESTATE,
         "the genotypes were reloaded after jwas_hip_gwas_begin");
    for (int32_t e = 0; e < nnz; ++e) {
        NEED(c, idx[e] >= 0 && idx[e] < c->p, JWAS_HIP_EINVAL, "marker index %d out of range", idx[e]);
        NEED(c, e == 0 || idx[e] > idx[e - 1], JWAS_HIP_EINVAL, "idx must be strictly ascending (entry %d: %d after %d)", e, idx[e], idx[e - 1]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (nnz > g.cap) {                                          // grow on demand (rare: a denser sample than any before)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int64_t cap = g.cap;
        while (cap < nnz) cap *= 2;
        if (cap > c->p) cap = c->p;
        int32_t* ni = nullptr; void* nv = nullptr;
        hipError_t ea = hipMalloc(&ni, 4 * (size_t)cap);
        if (ea == hipSuccess) ea = hipMalloc(&nv, 8 * (size_t)cap);
        if (ea != hipSuccess) {
            (void)hipGetLastError(); (void)hipFree(ni); (void)hipFree(nv);
            return fail(c, JWAS_HIP_ENOMEM, "jwas_hip_gwas_sample: %s (a list of %lld effects)", hipGetErrorString(ea), (long long)cap);
        }
        (void)hipFree(g.idx); (void)hipFree(g.val);
        g.idx = ni; g.val = nv; g.cap = cap;
    }
    const int nent = g.nwin + 1;
    hipError_t e = hipSuccess;
    if (nnz) e = hipMemcpyAsync(g.idx, idx, 4 * (size_t)nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(g.val, val, sizeof(T) * (size_t)nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((k_gwas_slices<>), dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, c->stream, nent, (int)nnz, g.cs, g.ce, g.idx, g.lo, g.hi);
        const dim3 grid((unsigned)g.nsl, (unsigned)g.nchunks);
        with_view(c, side<T>(c), g.out_rows, [&](auto cx) {
            if (g.local_ebv) hipLaunchKernelGGL((k_gwas_partial<decltype(cx), true>), grid, dim3(256), 0, c->stream, cx, nent, g.wpc, g.lo, g.hi, g.idx, (const T*)g.val, g.part, g.acc, g.ld);
            else             hipLaunchKernelGGL((k_gwas_partial<decltype(cx), false>), grid, dim3(256), 0, c->stream, cx, nent, g.wpc, g.lo, g.hi, g.idx, (const T*)g.val, g.part, g.acc, g.ld);
            return 0;
        });
        hipLaunchKernelGGL((k_window_reduce<>), dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, c->stream, nent, g.nsl, 2, g.part, g.out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(g.host_out, g.out, 16 * (size_t)nent, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "jwas_hip_gwas_sample: %s", hipGetErrorString(e));
    std::memcpy(out_sum, g.host_out, 8 * (size_t)nent);
    std::memcpy(out_ss, g.host_out + nent, 8 * (size_t)nent);
    g.nsamples += 1;
    return JWAS_HIP_OK;
}

}  // namespace

void gwas_free(jwas_hip_ctx* c)
{
    auto& g = c->gw;
    for (void* q : {(void*)g.cs, (void*)g.ce, (void*)g.lo, (void*)g.hi, (void*)g.idx, g.val, (void*)g.part, (void*)g.out, (void*)g.acc}) (void)hipFree(q);
    if (g.host_out) (void)hipHostFree(g.host_out);
    g = jwas_hip_ctx::Gwas();
}

extern "C" {

int jwas_hip_set_state(jwas_hip_ctx* c, int32_t trait, const float* a, const float* b, const void* d)
{
    return state_io<float>(c, trait, a, b, d, true, "jwas_hip_set_state (use jwas_hip_set_state_f64)");
}
int jwas_hip_set_state_f64(jwas_hip_ctx* c, int32_t trait, const double* a, const double* b, const void* d)
{
    return state_io<double>(c, trait, a, b, d, true, "");
}
int jwas_hip_get_state(jwas_hip_ctx* c, int32_t trait, float* a, float* b, void* d)
{
    return state_io<float>(c, trait, a, b, d, false, "jwas_hip_get_state (use jwas_hip_get_state_f64)");
}
int jwas_hip_get_state_f64(jwas_hip_ctx* c, int32_t trait, double* a, double* b, void* d)
{
    return state_io<double>(c, trait, a, b, d, false, "");
}

int jwas_hip_set_residual(jwas_hip_ctx* c, int32_t trait, const float* rh)
{
    return residual_io<float>(c, trait, rh, nullptr, "jwas_hip_set_residual (use jwas_hip_set_residual_f64)");
}
int jwas_hip_set_residual_f64(jwas_hip_ctx* c, int32_t trait, const double* rh) { return residual_io<double>(c, trait, rh, nullptr, ""); }
int jwas_hip_get_residual(jwas_hip_ctx* c, int32_t trait, float* rh)
{
    return residual_io<float>(c, trait, nullptr, rh, "jwas_hip_get_residual (use jwas_hip_get_residual_f64)");
}
int jwas_hip_get_residual_f64(jwas_hip_ctx* c, int32_t trait, double* rh) { return residual_io<double>(c, trait, nullptr, rh, ""); }

int jwas_hip_get_posterior(jwas_hip_ctx* c, int32_t trait, float* ma, float* ma2, float* md) { return get_posterior<float>(c, trait, ma, ma2, md); }
int jwas_hip_get_posterior_f64(jwas_hip_ctx* c, int32_t trait, double* ma, double* ma2, double* md) { return get_posterior<double>(c, trait, ma, ma2, md); }

int jwas_hip_get_xpx(jwas_hip_ctx* c, float* out) { return get_xpx<float>(c, out); }
int jwas_hip_get_xpx_f64(jwas_hip_ctx* c, double* out) { return get_xpx<double>(c, out); }

int jwas_hip_get_marker_covariances(jwas_hip_ctx* c, float* out) { return get_marker_covariances<float>(c, out); }
int jwas_hip_get_marker_covariances_f64(jwas_hip_ctx* c, double* out) { return get_marker_covariances<double>(c, out); }

// Float64 context, multi-trait BayesA/B: the p x t x t per-marker covariances in double from the host (a Float32 context takes them
// with every sweep: jwas_sweep_params.var_effect_matrix)
int jwas_hip_set_marker_covariances_f64(jwas_hip_ctx* c, const double* mat)
{
    NEED(c, c && mat, JWAS_HIP_EINVAL, "NULL argument");
    ONLY_F64(c);
    NEED(c, c->method == JWAS_HIP_MTBAYESB1 || c->method == JWAS_HIP_MTBAYESB2, JWAS_HIP_ESTATE,
         "jwas_hip_set_marker_covariances_f64 needs init_state(JWAS_HIP_MTBAYESB1 | JWAS_HIP_MTBAYESB2, t)");
    auto* F = c->f64;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t mb = sizeof(double) * (size_t)c->ntraits * c->ntraits * c->p;
    if (!F->var_mat) HIPCHK(c, F->chain_mem.alloc(&F->var_mat, mb));
    HIPCHK(c, hipMemcpyAsync(F->var_mat, mat, mb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    F->var_mat_resident = true;
    return JWAS_HIP_OK;
}

// running posterior means of the current state as sample number k (output.jl:556-577)
int jwas_hip_accumulate(jwas_hip_ctx* c, double k)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, c->method >= 0, JWAS_HIP_ESTATE, "jwas_hip_init_state has not been called");
    NEED(c, k >= 1.0, JWAS_HIP_EINVAL, "nsamples must be >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t count = (int64_t)c->ntraits * c->p;
    on_side(c, [&](auto& S) {
        typedef typename std::decay<decltype(S)>::type::real T;
        hipLaunchKernelGGL(k_accumulate<T>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, count, (int)(c->method == JWAS_HIP_BAYESR), k,
                           (const T*)S.alpha, (const void*)S.delta, S.mean_a, S.mean_a2, S.mean_d);
        return 0;
    });
    HIPCHK(c, hipGetLastError());
    return JWAS_HIP_OK;
}

// r_trait -= X alpha_trait (the initial ycorr, MCMC_BayesianAlphabet.jl:142)
int jwas_hip_residual_sub_xalpha(jwas_hip_ctx* c, int32_t trait)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED_TRAIT(c, trait);
    HIPCHK(c, hipSetDevice(c->device));
    on_side(c, [&](auto& S) {
        return with_view(c, S, false, [&](auto cx) {
            hipLaunchKernelGGL((k_sub_xalpha<decltype(cx)>), dim3((unsigned)c->nslices), dim3(256), 0, c->stream, cx, c->p,
                               (const elem_t<decltype(cx)>*)(S.alpha + (size_t)trait * c->p), S.r + (size_t)trait * c->ld);
            return 0;
        });
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// getEBV's X * alpha (output.jl:281-306) on the training rows
int jwas_hip_mul_alpha(jwas_hip_ctx* c, int32_t trait, float* out) { return mul_alpha<float>(c, trait, out, "jwas_hip_mul_alpha"); }
int jwas_hip_mul_alpha_f64(jwas_hip_ctx* c, int32_t trait, double* out) { return mul_alpha<double>(c, trait, out, "jwas_hip_mul_alpha_f64"); }

int jwas_hip_load_output_dense_f32(jwas_hip_ctx* c, const float* Xh, int64_t n_out, int64_t p, int64_t ld_host)
{
    return load_output_dense<float>(c, Xh, n_out, p, ld_host);
}
int jwas_hip_load_output_dense_f64(jwas_hip_ctx* c, const double* Xh, int64_t n_out, int64_t p, int64_t ld_host)
{
    return load_output_dense<double>(c, Xh, n_out, p, ld_host);
}

int jwas_hip_mul_alpha_output(jwas_hip_ctx* c, int32_t trait, float* out) { return mul_alpha_output<float>(c, trait, out, "jwas_hip_mul_alpha_output"); }
int jwas_hip_mul_alpha_output_f64(jwas_hip_ctx* c, int32_t trait, double* out)
{
    return mul_alpha_output<double>(c, trait, out, "jwas_hip_mul_alpha_output_f64");
}

// Output rows as a second 2-bit packed matrix beside packed training storage (Mi.output_genotypes, tools4genotypes.jl:290-296, in the
// layout of Packed2BitBackend, streaming_genotypes.jl:7-25): decoded with the training means and centring.  The new matrix is
// complete before the earlier output rows go, so an error leaves them in place.
int jwas_hip_load_output_packed2bit(jwas_hip_ctx* c, const uint8_t* payload, int64_t n_out, int64_t p, int64_t stride_bytes)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, payload, JWAS_HIP_EINVAL, "payload is NULL");
    NEED(c, c->packed && c->Q, JWAS_HIP_ESTATE, "packed output rows need 2-bit packed training storage: their means and centring are its own");
    NEED(c, n_out >= 1 && n_out < (1ll << 31), JWAS_HIP_EINVAL, "n_out must be within [1, 2^31) (got %lld)", (long long)n_out);
    NEED(c, p == c->p, JWAS_HIP_EINVAL, "output genotypes have %lld markers, the training matrix %lld", (long long)p, (long long)c->p);
    const int64_t width = (n_out + 3) / 4;
    NEED(c, stride_bytes >= width, JWAS_HIP_EINVAL, "stride_bytes (%lld) must be >= cld(n_out,4) = %lld", (long long)stride_bytes, (long long)width);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t ld = round_up(n_out, kSliceRows);
    const size_t sb = (size_t)(ld >> 2);
    uint8_t* q = nullptr;
    hipError_t e = hipMalloc(&q, sb * (size_t)p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, JWAS_HIP_ENOMEM, "jwas_hip_load_output_packed2bit: device allocation of %zu bytes failed", sb * (size_t)p); }
    e = hipMemsetAsync(q, 0, sb * (size_t)p, c->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(q, sb, payload, (size_t)stride_bytes, (size_t)width, (size_t)p, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(q); return fail(c, JWAS_HIP_EHIP, "jwas_hip_load_output_packed2bit: %s", hipGetErrorString(e)); }
    drop_output_rows(c);
    c->load_mem.ptrs.push_back(q);
    c->Qout = q; c->n_out = n_out; c->ld_out = ld;
    return JWAS_HIP_OK;
}

// getEBV (output.jl:281-306) for all traits of the context at once: out[k * n_out + i].  Packed output rows: one launch of
// k_ebv_packed; dense ones: jwas_hip_mul_alpha_output trait by trait.  The bits are jwas_hip_mul_alpha_output's either way.
int jwas_hip_ebv_output(jwas_hip_ctx* c, float* out)
{
    if (c) NOT_F64(c, "jwas_hip_ebv_output (use jwas_hip_mul_alpha_output_f64 per trait)");
    NEED(c, c && out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, c->method >= 0, JWAS_HIP_ESTATE, "jwas_hip_init_state has not been called");
    NEED(c, have_output_rows(c, *c), JWAS_HIP_ESTATE, "no output rows are loaded (jwas_hip_load_output_dense_f32, jwas_hip_load_output_packed2bit, jwas_hip_plink_commit_output)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->Qout) return ebv_output_packed(c, out);
    for (int32_t k = 0; k < c->ntraits; ++k)
        if (int rc = mul_alpha_rows<float>(c, k, true, c->ld_out, c->n_out, out + (size_t)k * c->n_out, "jwas_hip_ebv_output")) return rc;
    return JWAS_HIP_OK;
}

int jwas_hip_get_alpha_sparse(jwas_hip_ctx* c, int32_t trait, int64_t capacity, int32_t* idx, float* val, int64_t* nnz_out)
{
    return get_alpha_sparse<float>(c, trait, capacity, idx, val, nnz_out);
}
int jwas_hip_get_alpha_sparse_f64(jwas_hip_ctx* c, int32_t trait, int64_t capacity, int32_t* idx, double* val, int64_t* nnz_out)
{
    return get_alpha_sparse<double>(c, trait, capacity, idx, val, nnz_out);
}

int jwas_hip_window_sums(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx, const float* val,
                         double* out_sum, double* out_ss)
{
    double* outs[2] = {out_sum, out_ss};
    return window_sums<float>(c, use_output_rows, nwin, wptr, idx, val, nullptr, outs, "jwas_hip_window_sums");
}
int jwas_hip_window_sums_f64(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx, const double* val,
                             double* out_sum, double* out_ss)
{
    double* outs[2] = {out_sum, out_ss};
    return window_sums<double>(c, use_output_rows, nwin, wptr, idx, val, nullptr, outs, "jwas_hip_window_sums_f64");
}

// ... and the window genetic covariance / correlation of two traits' samples (GWAS.jl:199-217)
int jwas_hip_window_sums2(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx, const float* val1,
                          const float* val2, double* out_sum1, double* out_ss1, double* out_sum2, double* out_ss2, double* out_cross)
{
    return window_sums2<float>(c, use_output_rows, nwin, wptr, idx, val1, val2, {out_sum1, out_ss1, out_sum2, out_ss2, out_cross}, "jwas_hip_window_sums");
}
int jwas_hip_window_sums2_f64(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* wptr, const int32_t* idx, const double* val1,
                              const double* val2, double* out_sum1, double* out_ss1, double* out_sum2, double* out_ss2, double* out_cross)
{
    return window_sums2<double>(c, use_output_rows, nwin, wptr, idx, val1, val2, {out_sum1, out_ss1, out_sum2, out_ss2, out_cross}, "jwas_hip_window_sums_f64");
}

int64_t jwas_hip_gwas_estimate_bytes(int64_t n_rows, int64_t nwin, int64_t max_nnz, int32_t local_ebv)
{
    if (n_rows < 1 || nwin < 1 || max_nnz < 0) return 0;
    const int64_t ld = round_up(n_rows, kSliceRows), nsl = ld / kSliceRows, nent = nwin + 1;
    int64_t bytes = 2 * 4 * nwin + 2 * 4 * nent;                 // column ranges + list slices
    bytes += (max_nnz > 0 ? max_nnz : 1) * (4 + 8);              // idx + val (double at most)
    bytes += 2 * 8 * nent * nsl + 2 * 8 * nent;                  // slice partials + sums
    if (local_ebv) bytes += 8 * ld * nwin;                       // the local-EBV accumulator
    return bytes;
}

int jwas_hip_gwas_begin(jwas_hip_ctx* c, int32_t use_output_rows, int32_t nwin, const int32_t* col_start, const int32_t* col_end, int32_t local_ebv)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, col_start && col_end, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, nwin >= 1, JWAS_HIP_EINVAL, "nwin must be >= 1 (got %d)", nwin);
    NEED(c, have_genotypes(c), JWAS_HIP_ESTATE, "no genotype matrix loaded");
    int64_t n_rows = 0, ld = 0;
    NEED(c, !use_output_rows || IS_F64(c) || !c->Qout, JWAS_HIP_EUNSUP,
         "jwas_hip_gwas_begin: a session on 2-bit packed output rows is not available (jwas_hip_window_sums(use_output_rows) runs on them)");
    NEED(c, !use_output_rows || output_rows_ptr(c, &n_rows, &ld), JWAS_HIP_ESTATE, "%s has not been called",
         IS_F64(c) ? load_output_name<double>() : load_output_name<float>());
    for (int w = 0; w < nwin; ++w) {
        NEED(c, col_start[w] <= col_end[w], JWAS_HIP_EINVAL, "window %d: col_start %d > col_end %d", w, col_start[w], col_end[w]);
        NEED(c, col_start[w] >= 0 && col_end[w] <= c->p, JWAS_HIP_EINVAL, "window %d: columns [%d, %d) outside [0, %lld]", w, col_start[w], col_end[w], (long long)c->p);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    gwas_free(c);
    auto& g = c->gw;
    g.mat = gwas_matrix(c, use_output_rows != 0, &g.n_rows, &g.ld);
    g.out_rows = use_output_rows != 0; g.local_ebv = local_ebv != 0; g.nwin = nwin;
    g.nsl = (int)(g.ld / kSliceRows);
    g.wpc = (int)gwas_windows_per_chunk(nwin, g.nsl);
    g.nchunks = 1 + (nwin + g.wpc - 1) / g.wpc;
    const size_t nent = (size_t)nwin + 1;
    g.cap = 4096;
    hipError_t e = g.local_ebv ? hipMalloc(&g.acc, 8 * (size_t)g.ld * nwin) : hipSuccess;      // the largest first: refuse early
    if (e == hipSuccess) e = hipMalloc(&g.cs, 4 * (size_t)nwin);
    if (e == hipSuccess) e = hipMalloc(&g.ce, 4 * (size_t)nwin);
    if (e == hipSuccess) e = hipMalloc(&g.lo, 4 * nent);
    if (e == hipSuccess) e = hipMalloc(&g.hi, 4 * nent);
    if (e == hipSuccess) e = hipMalloc(&g.idx, 4 * (size_t)g.cap);
    if (e == hipSuccess) e = hipMalloc(&g.val, 8 * (size_t)g.cap);
    if (e == hipSuccess) e = hipMalloc(&g.part, 16 * nent * (size_t)g.nsl);
    if (e == hipSuccess) e = hipMalloc(&g.out, 16 * nent);
    if (e == hipSuccess) e = hipHostMalloc(&g.host_out, 16 * nent);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const int64_t rows = g.n_rows, ldr = g.ld;
        gwas_free(c);
        return fail(c, JWAS_HIP_ENOMEM, "jwas_hip_gwas_begin: %s (the session needs %.3f GB, %lld rows x %d windows x 8 bytes of it for the local EBVs)",
                    hipGetErrorString(e), jwas_hip_gwas_estimate_bytes(rows, nwin, 4096, local_ebv) / 1e9, (long long)(local_ebv ? ldr : 0), nwin);
    }
    e = hipMemcpyAsync(g.cs, col_start, 4 * (size_t)nwin, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(g.ce, col_end, 4 * (size_t)nwin, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && g.local_ebv) e = hipMemsetAsync(g.acc, 0, 8 * (size_t)g.ld * nwin, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { gwas_free(c); return fail(c, JWAS_HIP_EHIP, "jwas_hip_gwas_begin: %s", hipGetErrorString(e)); }
    g.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_gwas_sample(jwas_hip_ctx* c, int32_t nnz, const int32_t* idx, const float* val, double* out_sum, double* out_ss)
{
    return gwas_sample<float>(c, nnz, idx, val, out_sum, out_ss);
}
int jwas_hip_gwas_sample_f64(jwas_hip_ctx* c, int32_t nnz, const int32_t* idx, const double* val, double* out_sum, double* out_ss)
{
    return gwas_sample<double>(c, nnz, idx, val, out_sum, out_ss);
}

int jwas_hip_gwas_local_ebv(jwas_hip_ctx* c, double* out, int64_t* nsamples)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, out && nsamples, JWAS_HIP_EINVAL, "NULL argument");
    auto& g = c->gw;
    NEED(c, g.active, JWAS_HIP_ESTATE, "jwas_hip_gwas_begin has not been called");
    NEED(c, g.local_ebv, JWAS_HIP_ESTATE, "the session was begun without local_ebv");
    HIPCHK(c, hipSetDevice(c->device));
    // window-major rows [0, n_rows) of every window's padded column; the padding rows stay on the device
    HIPCHK(c, hipMemcpy2DAsync(out, 8 * (size_t)g.n_rows, g.acc, 8 * (size_t)g.ld, 8 * (size_t)g.n_rows, (size_t)g.nwin, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *nsamples = g.nsamples;
    if (g.nsamples > 0) {
        const double s = (double)g.nsamples;
        const int64_t cnt = g.n_rows * g.nwin;
        for (int64_t i = 0; i < cnt; ++i) out[i] /= s;
    }
    return JWAS_HIP_OK;
}

int jwas_hip_gwas_geometry(jwas_hip_ctx* c, int32_t* nslices, int32_t* windows_per_chunk, int32_t* nchunks)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, c->gw.active, JWAS_HIP_ESTATE, "jwas_hip_gwas_begin has not been called");
    if (nslices) *nslices = c->gw.nsl;
    if (windows_per_chunk) *windows_per_chunk = c->gw.wpc;
    if (nchunks) *nchunks = c->gw.nchunks;
    return JWAS_HIP_OK;
}

int jwas_hip_gwas_end(jwas_hip_ctx* c) { return session_drop(c, gwas_free); }

}  // extern "C"
