// session_ssbr.hip -- single-step analysis (ssbr.hpp), jwas_hip_ss_begin .. _end: the imputation of impute_genotypes and the J vector
// of make_JVecs (single_step/SSBR.jl:83-159) as a sparse solve with many right-hand sides on the factors of A^nn.
//
// The solve kernel (ssbr.hpp, k_ss_solve) runs one thread per marker column; a thread reads from the work matrix only what it wrote
// itself.  No barriers between workgroups, no atomics, no flags, no waits: it cannot hang.  Everything it indexes with -- row
// pointers, columns, permutations, target rows -- is validated on the host in jwas_hip_ss_begin / _set_rows before any launch.
#include "ctx.hpp"
#include "ssbr.hpp"

void ss_free(jwas_hip_ctx* c) { DevOwner::reset(c->ss); }

static int need_ss(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::ss, "jwas_hip_ss_begin")) return rc;
    return refuse_shards(c, "single-step imputation sessions");
}

static int64_t ss_bytes(int64_t nn, int64_t g, int64_t nnz_l, int64_t nnz_u, int64_t nnz_a, int64_t ldc)
{
    // three row-pointer arrays, (column, value) of every stored entry, the two permutations, W, Gt and the staging block
    return 8 * 3 * (nn + 1) + 12 * (nnz_l + nnz_u + nnz_a) + 4 * 2 * nn + 8 * ldc * (nn + 2 * g);
}

// a CSR matrix with nrows rows and ncols columns: row pointers from 0, non-decreasing; columns in range, strictly ascending in a row
static int check_csr(jwas_hip_ctx* c, const char* what, int64_t nrows, int64_t ncols, const int64_t* ptr, const int32_t* col, const double* val)
{
    NEED(c, ptr && col && val, JWAS_HIP_EINVAL, "%s: NULL argument", what);
    NEED(c, ptr[0] == 0, JWAS_HIP_EINVAL, "%s: the row pointers must start at 0 (got %lld)", what, (long long)ptr[0]);
    for (int64_t r = 0; r < nrows; ++r) {
        NEED(c, ptr[r + 1] >= ptr[r], JWAS_HIP_EINVAL, "%s: the row pointers decrease at row %lld", what, (long long)r);
        for (int64_t e = ptr[r]; e < ptr[r + 1]; ++e) {
            NEED(c, col[e] >= 0 && col[e] < ncols, JWAS_HIP_EINVAL, "%s: column %d of row %lld is outside [0,%lld)", what, col[e], (long long)r, (long long)ncols);
            NEED(c, e == ptr[r] || col[e] > col[e - 1], JWAS_HIP_EINVAL, "%s: the columns of row %lld are not strictly ascending", what, (long long)r);
            NEED(c, std::isfinite(val[e]), JWAS_HIP_EINVAL, "%s: the value at row %lld, column %d is not finite (%g)", what, (long long)r, col[e], val[e]);
        }
    }
    return JWAS_HIP_OK;
}

static int check_perm(jwas_hip_ctx* c, const char* what, int64_t n, const int32_t* perm)
{
    NEED(c, perm, JWAS_HIP_EINVAL, "%s: NULL argument", what);
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        NEED(c, perm[i] >= 0 && perm[i] < n, JWAS_HIP_EINVAL, "%s[%lld] = %d is outside [0,%lld)", what, (long long)i, perm[i], (long long)n);
        NEED(c, !seen[(size_t)perm[i]], JWAS_HIP_EINVAL, "%s is not a permutation: %d appears twice", what, perm[i]);
        seen[(size_t)perm[i]] = 1;
    }
    return JWAS_HIP_OK;
}

// the block at `stage` -> Gt, the solve; T: the element type of the staged block
template <class T>
static void ss_stage_and_solve(jwas_hip_ctx* c, int32_t count)
{
    auto& b = c->ss;
    const dim3 tile(jws::kTile, jws::kTileRows);
    hipLaunchKernelGGL((jws::k_ss_stage<T>), dim3((unsigned)((b.g + jws::kTile - 1) / jws::kTile), (unsigned)((count + jws::kTile - 1) / jws::kTile)), tile, 0, c->stream,
                       (const T*)b.stage, b.g, b.g, count, b.Gt, b.ldc);
    jws::SolveArgs a = {};
    a.Lp = b.Lp; a.Up = b.Up; a.Ap = b.Ap; a.Lc = b.Lc; a.Uc = b.Uc; a.Ac = b.Ac; a.Lv = b.Lv; a.Uv = b.Uv; a.Av = b.Av;
    a.rsrc = b.rsrc; a.Gt = b.Gt; a.W = b.W; a.nn = b.nn; a.ldc = b.ldc; a.count = count;
    hipLaunchKernelGGL(jws::k_ss_solve, dim3((unsigned)((count + jws::kSolveThreads - 1) / jws::kSolveThreads)), dim3(jws::kSolveThreads), 0, c->stream, a);
}

template <class T>
static void ss_scatter(jwas_hip_ctx* c, const int32_t* prow, int64_t nrows, int32_t count, T* out, int64_t ld, int64_t j0)
{
    auto& b = c->ss;
    hipLaunchKernelGGL((jws::k_ss_scatter<T>), dim3((unsigned)((ld + jws::kTile - 1) / jws::kTile), (unsigned)((count + jws::kTile - 1) / jws::kTile)),
                       dim3(jws::kTile, jws::kTileRows), 0, c->stream, (const double*)b.W, (const double*)b.Gt, b.ldc, b.nn, (const int32_t*)b.perm_c, prow, nrows,
                       count, out, ld, j0);
}

// the matrix behind a target, as it is NOW: its rows, leading dimension and storage (NULL: none)
static void* ss_target(jwas_hip_ctx* c, int target, int64_t* n, int64_t* ld)
{
    if (target == 0) {
        *n = c->n; *ld = c->ld;
        return c->packed ? nullptr : const_cast<void*>(genotypes_ptr(c));
    }
    return const_cast<void*>(output_rows_ptr(c, n, ld));
}

extern "C" {

int jwas_hip_ss_begin(jwas_hip_ctx* c, int64_t n_n, int64_t g, const int64_t* L_ptr, const int32_t* L_col, const double* L_val, const int64_t* U_ptr,
                      const int32_t* U_col, const double* U_val, const int32_t* perm_r, const int32_t* perm_c, const int64_t* A_ptr, const int32_t* A_col,
                      const double* A_val, int64_t budget_bytes, int64_t* ldc_out)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    if (int rc = refuse_shards(c, "single-step imputation sessions")) return rc;
    NEED(c, n_n >= 1 && g >= 1 && n_n < (1ll << 31) && g < (1ll << 31) && n_n + g < (1ll << 31), JWAS_HIP_EINVAL,
         "the numbers of non-genotyped (%lld) and genotyped (%lld) individuals must be >= 1 and below 2^31 together", (long long)n_n, (long long)g);
    if (int rc = check_csr(c, "L", n_n, n_n, L_ptr, L_col, L_val)) return rc;
    if (int rc = check_csr(c, "U", n_n, n_n, U_ptr, U_col, U_val)) return rc;
    if (int rc = check_csr(c, "Ai_ng", n_n, g, A_ptr, A_col, A_val)) return rc;
    for (int64_t r = 0; r < n_n; ++r) {
        NEED(c, L_ptr[r + 1] > L_ptr[r] && L_col[L_ptr[r + 1] - 1] == r && L_val[L_ptr[r + 1] - 1] == 1.0, JWAS_HIP_EINVAL,
             "L is not unit lower triangular: row %lld does not end with a stored diagonal of 1", (long long)r);      // (ascending columns: nothing above the diagonal)
        NEED(c, U_ptr[r + 1] > U_ptr[r] && U_col[U_ptr[r]] == r, JWAS_HIP_EINVAL, "U is not upper triangular with a stored diagonal: row %lld does not start at its diagonal",
             (long long)r);
        NEED(c, U_val[U_ptr[r]] != 0.0, JWAS_HIP_EINVAL, "U has a zero diagonal at row %lld", (long long)r);       // (finite: check_csr)
    }
    if (int rc = check_perm(c, "perm_r", n_n, perm_r)) return rc;
    if (int rc = check_perm(c, "perm_c", n_n, perm_c)) return rc;
    const int64_t nnz_l = L_ptr[n_n], nnz_u = U_ptr[n_n], nnz_a = A_ptr[n_n];
    // markers per chunk: the largest multiple of the granule the budget pays for
    const int64_t fixed = ss_bytes(n_n, g, nnz_l, nnz_u, nnz_a, 0), per_col = 8 * (n_n + 2 * g);
    NEED(c, budget_bytes >= fixed + per_col * jws::kChunkGranule, JWAS_HIP_ENOMEM,
         "the byte budget (%lld) does not pay for the factors and one chunk of %d markers (%lld bytes)", (long long)budget_bytes, jws::kChunkGranule,
         (long long)(fixed + per_col * jws::kChunkGranule));
    const int64_t ldc = std::min<int64_t>(jws::kMaxChunk, (budget_bytes - fixed) / per_col / jws::kChunkGranule * jws::kChunkGranule);
    if (int rc = session_drop(c, ss_free)) return rc;
    auto& b = c->ss;
    b.nn = n_n; b.g = g; b.ldc = ldc; b.nnz_l = nnz_l; b.nnz_u = nnz_u; b.nnz_a = nnz_a;
    auto alloc = [&](auto** ptr, size_t bytes) { return alloc_or_nomem(c, b.mem, ptr, std::max<size_t>(bytes, 8), "single-step imputation session", ss_free); };
    std::vector<int32_t> rsrc((size_t)n_n);
    for (int64_t i = 0; i < n_n; ++i) rsrc[(size_t)perm_r[i]] = (int32_t)i;       // row i of A^nn sits at position perm_r[i]
    struct Up { void** dst; const void* src; size_t bytes; };
    const size_t rp = sizeof(int64_t) * (size_t)(n_n + 1), pm = sizeof(int32_t) * (size_t)n_n;
    const Up ups[] = {
        {(void**)&b.Lp, L_ptr, rp}, {(void**)&b.Up, U_ptr, rp}, {(void**)&b.Ap, A_ptr, rp},
        {(void**)&b.Lc, L_col, 4 * (size_t)nnz_l}, {(void**)&b.Uc, U_col, 4 * (size_t)nnz_u}, {(void**)&b.Ac, A_col, 4 * (size_t)nnz_a},
        {(void**)&b.Lv, L_val, 8 * (size_t)nnz_l}, {(void**)&b.Uv, U_val, 8 * (size_t)nnz_u}, {(void**)&b.Av, A_val, 8 * (size_t)nnz_a},
        {(void**)&b.rsrc, rsrc.data(), pm}, {(void**)&b.perm_c, perm_c, pm},
    };
    for (const Up& u : ups) {
        if (int rc = alloc((char**)u.dst, u.bytes)) return rc;
        if (u.bytes) HIPCHK(c, hipMemcpyAsync(*u.dst, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = alloc(&b.Gt, sizeof(double) * (size_t)g * (size_t)ldc)) return rc;
    if (int rc = alloc(&b.W, sizeof(double) * (size_t)n_n * (size_t)ldc)) return rc;
    if (int rc = alloc((char**)&b.stage, sizeof(double) * (size_t)g * (size_t)ldc)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the caller's arrays may go away once this returns)
    b.active = true;
    if (ldc_out) *ldc_out = ldc;
    return JWAS_HIP_OK;
}

int jwas_hip_ss_set_rows(jwas_hip_ctx* c, int32_t target, int64_t nrows, const int32_t* prow)
{
    if (int rc = need_ss(c)) return rc;
    auto& b = c->ss;
    NEED(c, target == 0 || target == 1, JWAS_HIP_EINVAL, "target must be 0 (the sweep matrix) or 1 (the output matrix), got %d", target);
    NEED(c, prow, JWAS_HIP_EINVAL, "NULL argument");
    int64_t n = 0, ld = 0;
    NEED(c, ss_target(c, target, &n, &ld), JWAS_HIP_ESTATE, target == 0 ? "no dense genotype matrix to impute into: allocate or load it first"
                                                                        : "no output matrix to impute into: load it first");
    NEED(c, nrows == n, JWAS_HIP_EINVAL, "nrows (%lld) differs from the rows of the target matrix (%lld)", (long long)nrows, (long long)n);
    for (int64_t r = 0; r < nrows; ++r)
        NEED(c, prow[r] >= 0 && prow[r] < b.nn + b.g, JWAS_HIP_EINVAL, "prow[%lld] = %d is outside [0,%lld)", (long long)r, prow[r], (long long)(b.nn + b.g));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.mem.free_one(b.prow[target]);
    b.nrows[target] = 0;
    if (b.mem.alloc(&b.prow[target], sizeof(int32_t) * (size_t)nrows) != hipSuccess)
        return fail(c, JWAS_HIP_ENOMEM, "single-step imputation session: device allocation of %zu bytes failed", sizeof(int32_t) * (size_t)nrows);
    HIPCHK(c, hipMemcpyAsync(b.prow[target], prow, sizeof(int32_t) * (size_t)nrows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.nrows[target] = nrows;
    return JWAS_HIP_OK;
}

int jwas_hip_ss_impute(jwas_hip_ctx* c, int64_t j0, int64_t count, const void* Mg, int64_t ldg)
{
    if (int rc = need_ss(c)) return rc;
    auto& b = c->ss;
    NEED(c, Mg, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, count >= 1 && count <= b.ldc, JWAS_HIP_EINVAL, "count (%lld) must be in [1,%lld], the session's markers per chunk", (long long)count, (long long)b.ldc);
    NEED(c, ldg >= b.g, JWAS_HIP_EINVAL, "ldg (%lld) must be >= the number of genotyped individuals (%lld)", (long long)ldg, (long long)b.g);
    NEED(c, b.nrows[0] || b.nrows[1], JWAS_HIP_ESTATE, "no target rows: call jwas_hip_ss_set_rows first");
    // (both targets have the sweep matrix's p markers: an output matrix exists only next to a sweep matrix and is loaded with its p)
    NEED(c, c->p > 0, JWAS_HIP_ESTATE, "no genotype matrix: allocate or load the sweep matrix first");
    NEED(c, j0 >= 0 && j0 + count <= c->p, JWAS_HIP_EINVAL, "column range [%lld,%lld) outside [0,%lld)", (long long)j0, (long long)(j0 + count), (long long)c->p);
    void* mat[2] = {};
    int64_t ld[2] = {};
    for (int tg = 0; tg < 2; ++tg)
        if (b.nrows[tg]) {
            int64_t n = 0;
            mat[tg] = ss_target(c, tg, &n, &ld[tg]);
            NEED(c, mat[tg] && n == b.nrows[tg], JWAS_HIP_ESTATE, "the %s matrix was replaced after jwas_hip_ss_set_rows (rows %lld, the target's %lld)",
                 tg ? "output" : "sweep", (long long)n, (long long)b.nrows[tg]);
        }
    if (b.nrows[0]) {
        NEED(c, c->nblocks == 0, JWAS_HIP_ESTATE, "impute before jwas_hip_setup_blocks: x'x and the Grams depend on the matrix");
        NEED(c, !c->rr.active && !c->mg.active, JWAS_HIP_ESTATE, "a random-regression or mega-trait session holds Grams of this matrix: end it first");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t el = IS_F64(c) ? sizeof(double) : sizeof(float);
    HIPCHK(c, hipMemcpy2DAsync(b.stage, el * (size_t)b.g, Mg, el * (size_t)ldg, el * (size_t)b.g, (size_t)count, hipMemcpyHostToDevice, c->stream));
    with_real(c, [&](auto real) {
        using real_t = decltype(real);
        ss_stage_and_solve<real_t>(c, (int32_t)count);
        for (int tg = 0; tg < 2; ++tg)
            if (b.nrows[tg]) ss_scatter<real_t>(c, b.prow[tg], b.nrows[tg], (int32_t)count, (real_t*)mat[tg], ld[tg], j0);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the caller's block may go away; the staging block is reused by the next chunk)
    return JWAS_HIP_OK;
}

int jwas_hip_ss_solve_host(jwas_hip_ctx* c, int64_t count, const double* Mg, int64_t ldg, int64_t nrows, const int32_t* prow, double* out)
{
    if (int rc = need_ss(c)) return rc;
    auto& b = c->ss;
    NEED(c, Mg && prow && out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, count >= 1 && count <= b.ldc, JWAS_HIP_EINVAL, "count (%lld) must be in [1,%lld], the session's markers per chunk", (long long)count, (long long)b.ldc);
    NEED(c, ldg >= b.g, JWAS_HIP_EINVAL, "ldg (%lld) must be >= the number of genotyped individuals (%lld)", (long long)ldg, (long long)b.g);
    NEED(c, nrows >= 1 && nrows < (1ll << 31), JWAS_HIP_EINVAL, "nrows must be in [1,2^31) (got %lld)", (long long)nrows);
    for (int64_t r = 0; r < nrows; ++r)
        NEED(c, prow[r] >= 0 && prow[r] < b.nn + b.g, JWAS_HIP_EINVAL, "prow[%lld] = %d is outside [0,%lld)", (long long)r, prow[r], (long long)(b.nn + b.g));
    for (int64_t j = 0; j < count; ++j)
        for (int64_t k = 0; k < b.g; ++k)
            NEED(c, std::isfinite(Mg[j * ldg + k]), JWAS_HIP_EINVAL, "Mg[%lld][%lld] is not finite (%g)", (long long)k, (long long)j, Mg[j * ldg + k]);
    HIPCHK(c, hipSetDevice(c->device));
    DevOwner tmp;
    int32_t* d_prow = nullptr;
    double* d_out = nullptr;
    if (tmp.alloc(&d_prow, sizeof(int32_t) * (size_t)nrows) != hipSuccess || tmp.alloc(&d_out, sizeof(double) * (size_t)nrows * (size_t)count) != hipSuccess) {
        tmp.release();
        return fail(c, JWAS_HIP_ENOMEM, "jwas_hip_ss_solve_host: device allocation of %lld x %lld doubles failed", (long long)nrows, (long long)count);
    }
    hipError_t e = hipMemcpyAsync(d_prow, prow, sizeof(int32_t) * (size_t)nrows, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(b.stage, sizeof(double) * (size_t)b.g, Mg, sizeof(double) * (size_t)ldg, sizeof(double) * (size_t)b.g, (size_t)count, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ss_stage_and_solve<double>(c, (int32_t)count);
        ss_scatter<double>(c, d_prow, nrows, (int32_t)count, d_out, nrows, 0);      // (leading dimension = nrows: no pad rows)
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)nrows * (size_t)count, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    tmp.release();
    if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "jwas_hip_ss_solve_host: %s", hipGetErrorString(e));
    return JWAS_HIP_OK;
}

int jwas_hip_ss_get_columns(jwas_hip_ctx* c, int32_t target, int64_t j0, int64_t count, int64_t ld, void* out)
{
    if (int rc = need_ss(c)) return rc;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, target == 0 || target == 1, JWAS_HIP_EINVAL, "target must be 0 (the sweep matrix) or 1 (the output matrix), got %d", target);
    int64_t n = 0, ldt = 0;
    const char* mat = (const char*)ss_target(c, target, &n, &ldt);
    NEED(c, mat, JWAS_HIP_ESTATE, "the target has no dense matrix");
    NEED(c, ld == ldt, JWAS_HIP_EINVAL, "ld (%lld) differs from the target's leading dimension (%lld)", (long long)ld, (long long)ldt);
    NEED(c, j0 >= 0 && count >= 1 && j0 + count <= c->p, JWAS_HIP_EINVAL, "column range [%lld,%lld) outside [0,%lld)", (long long)j0, (long long)(j0 + count), (long long)c->p);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t el = IS_F64(c) ? sizeof(double) : sizeof(float);
    return to_host(c, out, mat + el * (size_t)j0 * (size_t)ld, el * (size_t)count * (size_t)ld);
}

int64_t jwas_hip_ss_estimate_bytes(int64_t n_n, int64_t g, int64_t nnz_l, int64_t nnz_u, int64_t nnz_a, int64_t markers_per_chunk)
{
    const int64_t ldc = std::min<int64_t>(jws::kMaxChunk, round_up(std::max<int64_t>(markers_per_chunk, 1), jws::kChunkGranule));
    return ss_bytes(std::max<int64_t>(n_n, 1), std::max<int64_t>(g, 1), std::max<int64_t>(nnz_l, 0), std::max<int64_t>(nnz_u, 0), std::max<int64_t>(nnz_a, 0), ldc);
}

int jwas_hip_ss_end(jwas_hip_ctx* c)
{
    if (int rc = session_guard(c, &jwas_hip_ctx::ss, "jwas_hip_ss_begin")) return rc;
    return session_drop(c, ss_free);
}

}  // extern "C"
