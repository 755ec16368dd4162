// session_locpar.hip -- the location parameters (locpar.hpp), jwas_hip_locpar_begin .. _end and jwas_hip_lp_*:
// MCMC_BayesianAlphabet.jl:193-220, iterative_solver/solver.jl:143-162.  With per-record weights (jwas_hip_mtmiss_set_record_weights)
// a step reads the codes and the table C of the context's missing-trait state.
#include "ctx.hpp"
#include "locpar.hpp"

static_assert(jwp::kMaxGroups == JWAS_HIP_LOCPAR_MAX_GROUPS && jwp::kMaxT == JWAS_HIP_MAX_TRAITS, "limit mismatch");

static int need_locpar(jwas_hip_ctx* c) { return session_guard(c, &jwas_hip_ctx::lp, "jwas_hip_locpar_begin", nullptr); }

void locpar_free(jwas_hip_ctx* c)
{
    auto& b = c->lp;
    for (auto& v : b.structs) v.mem.release();
    DevOwner::reset(b);
}

template <class V>
static hipError_t locpar_upload(DevOwner& mem, V** dev, const std::vector<V>& host)
{
    hipError_t e = mem.alloc(dev, sizeof(V) * std::max<size_t>(host.size(), 1));
    if (e == hipSuccess && !host.empty()) e = hipMemcpy(*dev, host.data(), sizeof(V) * host.size(), hipMemcpyHostToDevice);
    return e;
}

// the term's layout from level[] (NULL: every record in level 0) and x[] (NULL: ones): records sorted by (level, record), pieces of
// at most kPiece records, the lane-group width, d = sum w x^2
static int locpar_add_term(jwas_hip_ctx* c, int32_t trait, const double* x, const int32_t* level, int64_t nlevels, int32_t group)
{
    auto& b = c->lp;
    const int64_t n = c->n;
    jwas_hip_ctx::Locpar::Term T;
    T.trait = trait; T.group = group; T.nlevels = nlevels;
    std::vector<int32_t> start((size_t)nlevels + 1, 0), rec;
    if (level) {
        for (int64_t i = 0; i < n; ++i) if (level[i] >= 0) ++start[(size_t)level[i] + 1];
        for (int64_t l = 0; l < nlevels; ++l) start[(size_t)l + 1] += start[(size_t)l];
        rec.resize((size_t)start[(size_t)nlevels]);
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; ++i) if (level[i] >= 0) rec[(size_t)fill[(size_t)level[i]]++] = (int32_t)i;      // (stable: ties by ascending record)
    } else {
        start[1] = (int32_t)n;
    }
    T.nin = start[(size_t)nlevels];
    std::vector<double> wx((size_t)T.nin), d((size_t)nlevels, 0.0);
    std::vector<int32_t> piece_lo, level_piece((size_t)nlevels + 1, 0);
    for (int64_t l = 0; l < nlevels; ++l) {
        for (int32_t j = start[(size_t)l]; j < start[(size_t)l + 1]; ++j) {
            const int64_t i = level ? rec[(size_t)j] : j;
            const double xi = x ? x[i] : 1.0;
            wx[(size_t)j] = b.w_host[(size_t)i] * xi;
            d[(size_t)l] = d[(size_t)l] + wx[(size_t)j] * xi;
        }
        for (int32_t j = start[(size_t)l]; j < start[(size_t)l + 1]; j += jwp::kPiece) piece_lo.push_back(j);
        level_piece[(size_t)l + 1] = (int32_t)piece_lo.size();
    }
    T.npieces = (int)piece_lo.size();
    piece_lo.push_back((int32_t)T.nin);
    // (pieces of different levels are adjacent in the sorted order: piece p ends where piece p + 1 starts)
    const int64_t avg = T.npieces ? (T.nin + T.npieces - 1) / T.npieces : 1;
    T.G = 1;
    while (T.G < 64 && T.G < avg) T.G <<= 1;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipSuccess;
    DevOwner mem;                                           // (the session adopts the buffers of a term that was added, and only those)
    if (x) { std::vector<double> xv(x, x + n); e = locpar_upload(mem, &T.x, xv); }
    if (level && e == hipSuccess) {
        std::vector<int32_t> lv(level, level + n);
        e = locpar_upload(mem, &T.level, lv);
        if (e == hipSuccess) e = locpar_upload(mem, &T.rec, rec);
    }
    if (e == hipSuccess) e = locpar_upload(mem, &T.wx, wx);
    if (e == hipSuccess) e = locpar_upload(mem, &T.piece_lo, piece_lo);
    if (e == hipSuccess) e = locpar_upload(mem, &T.level_piece, level_piece);
    if (e == hipSuccess) e = locpar_upload(mem, &T.d, d);
    if (e != hipSuccess) {
        mem.release();
        return fail(c, JWAS_HIP_EHIP, "uploading the term's layout failed: %s", hipGetErrorString(e));
    }
    b.mem.adopt(mem);
    T.off = b.q;
    if (group >= 0) {
        auto& g = b.groups[group];
        T.pos = g.nmembers;
        g.term[g.nmembers++] = (int)b.terms.size();
        g.nlevels = nlevels;
        b.ngroups = std::max(b.ngroups, group + 1);
    }
    b.q += nlevels;
    b.terms.push_back(T);
    return JWAS_HIP_OK;
}

static int locpar_check_add(jwas_hip_ctx* c, int32_t trait, int64_t n)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, !c->lp.finalized, JWAS_HIP_ESTATE, "terms are added before sol is first used (call jwas_hip_locpar_begin to start over)");
    NEED(c, trait >= 0 && trait < c->lp.nt, JWAS_HIP_EINVAL, "trait %d outside [0,%d)", trait, c->lp.nt);
    NEED(c, n == c->n, JWAS_HIP_EINVAL, "n (%lld) differs from the number of records (%lld)", (long long)n, (long long)c->n);
    NEED(c, c->lp.terms.size() < 0x10000000u, JWAS_HIP_EINVAL, "too many terms");
    return JWAS_HIP_OK;
}

// allocate sol, its means and the scratch of the largest term on the first use
static int locpar_finalize(jwas_hip_ctx* c)
{
    auto& b = c->lp;
    if (b.finalized) return JWAS_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int64_t maxp = 1, maxl = 1;
    for (auto& t : b.terms) { maxp = std::max<int64_t>(maxp, t.npieces); maxl = std::max(maxl, t.nlevels); }
    const size_t qb = sizeof(double) * (size_t)std::max<int64_t>(b.q, 1);
    for (double** v : {&b.sol, &b.mean, &b.mean2}) { HIPCHK(c, b.mem.alloc(v, qb)); HIPCHK(c, hipMemsetAsync(*v, 0, qb, c->stream)); }
    HIPCHK(c, b.mem.alloc(&b.part, sizeof(double) * (size_t)maxp));
    b.maxp = maxp;
    HIPCHK(c, b.mem.alloc(&b.delta, sizeof(double) * (size_t)maxl));
    std::vector<int64_t> offs((size_t)jwp::kMaxGroups * 32, 0);
    for (int g = 0; g < b.ngroups; ++g)
        for (int a = 0; a < b.groups[g].nmembers; ++a)
            for (int e = 0; e < b.groups[g].nmembers; ++e) {
                offs[(size_t)(g * 16 + a * b.groups[g].nmembers + e) * 2] = b.terms[(size_t)b.groups[g].term[a]].off;
                offs[(size_t)(g * 16 + a * b.groups[g].nmembers + e) * 2 + 1] = b.terms[(size_t)b.groups[g].term[e]].off;
            }
    HIPCHK(c, locpar_upload(b.mem, &b.cross_offs, offs));
    HIPCHK(c, b.mem.alloc(&b.cross_out, sizeof(double) * jwp::kMaxGroups * 16));
    HIPCHK(c, hipMemsetAsync(b.cross_out, 0, sizeof(double) * jwp::kMaxGroups * 16, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.finalized = true;
    return JWAS_HIP_OK;
}

extern "C" {

int jwas_hip_locpar_begin(jwas_hip_ctx* c, int32_t ntraits)
{
    if (int rc = begin_guard(c, "location parameters")) return rc;
    NEED(c, ntraits == c->ntraits, JWAS_HIP_EINVAL, "ntraits (%d) differs from jwas_hip_init_state's (%d)", ntraits, c->ntraits);
    if (int rc = session_drop(c, locpar_free)) return rc;
    auto& b = c->lp;
    b.nt = ntraits;
    b.w_host.assign((size_t)c->n, 1.0);
    if (IS_F64(c)) {
        HIPCHK(c, hipMemcpy(b.w_host.data(), c->f64->w, sizeof(double) * (size_t)c->n, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> w32((size_t)c->n);
        HIPCHK(c, hipMemcpy(w32.data(), c->w, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < c->n; ++i) b.w_host[(size_t)i] = (double)w32[(size_t)i];
    }
    b.active = true;
    return JWAS_HIP_OK;
}

int jwas_hip_locpar_add_covariate(jwas_hip_ctx* c, int32_t trait, int64_t n, const double* x)
{
    if (int rc = locpar_check_add(c, trait, n)) return rc;
    if (x)
        for (int64_t i = 0; i < n; ++i) NEED(c, std::isfinite(x[i]), JWAS_HIP_EINVAL, "record %lld: the covariate is not finite (%g)", (long long)i, x[i]);
    return locpar_add_term(c, trait, x, nullptr, 1, -1);
}

int jwas_hip_locpar_add_factor(jwas_hip_ctx* c, int32_t trait, int64_t n, const int32_t* level, int64_t nlevels, int32_t group)
{
    if (int rc = locpar_check_add(c, trait, n)) return rc;
    NEED(c, level, JWAS_HIP_EINVAL, "level is NULL");
    NEED(c, nlevels >= 1 && nlevels < (int64_t)1 << 31, JWAS_HIP_EINVAL, "nlevels must be 1 .. 2^31 - 1 (got %lld)", (long long)nlevels);
    for (int64_t i = 0; i < n; ++i)
        NEED(c, level[i] >= -1 && level[i] < nlevels, JWAS_HIP_EINVAL, "record %lld: level %d outside -1..%lld", (long long)i, level[i], (long long)nlevels - 1);
    NEED(c, group >= -1 && group < jwp::kMaxGroups, JWAS_HIP_EINVAL, "random_group must be -1 (fixed) or 0..%d (got %d)", jwp::kMaxGroups - 1, group);
    if (group >= 0) {
        const auto& g = c->lp.groups[group];
        NEED(c, g.nmembers < jwp::kMaxT, JWAS_HIP_EINVAL, "random effect %d already has %d member terms", group, g.nmembers);
        for (int a = 0; a < g.nmembers; ++a)
            NEED(c, c->lp.terms[(size_t)g.term[a]].trait != trait, JWAS_HIP_EUNSUP,
                 "random effect %d already has a term of trait %d: correlated terms within a trait stay on the reference", group, trait);
        NEED(c, g.nmembers == 0 || g.nlevels == nlevels, JWAS_HIP_EINVAL, "the member terms of random effect %d must have the same levels (%lld, got %lld)",
             group, (long long)g.nlevels, (long long)nlevels);
        const auto& v = c->lp.structs[group];
        NEED(c, !v.set || v.nlevels == nlevels, JWAS_HIP_EINVAL, "random effect %d has a structure of %lld levels (the term has %lld)", group,
             (long long)v.nlevels, (long long)nlevels);
    }
    return locpar_add_term(c, trait, nullptr, level, nlevels, group);
}

int jwas_hip_locpar_size(jwas_hip_ctx* c, int64_t* out_q)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, out_q, JWAS_HIP_EINVAL, "NULL argument");
    *out_q = c->lp.q;
    return JWAS_HIP_OK;
}

int jwas_hip_locpar_set_sol(jwas_hip_ctx* c, int64_t q, const double* sol)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, sol, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, q == c->lp.q, JWAS_HIP_EINVAL, "q (%lld) differs from the number of location parameters (%lld)", (long long)q, (long long)c->lp.q);
    if (int rc = locpar_finalize(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->lp.sol, sol, sizeof(double) * (size_t)q, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_locpar_get_sol(jwas_hip_ctx* c, int64_t q, double* out)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, q == c->lp.q, JWAS_HIP_EINVAL, "q (%lld) differs from the number of location parameters (%lld)", (long long)q, (long long)c->lp.q);
    if (int rc = locpar_finalize(c)) return rc;
    return to_host(c, out, c->lp.sol, sizeof(double) * (size_t)q);
}

int jwas_hip_locpar_step(jwas_hip_ctx* c, const jwas_locpar_params* P, jwas_locpar_stats* S)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, P, JWAS_HIP_EINVAL, "params is NULL");
    auto& b = c->lp;
    const int t = b.nt, nterms = (int)b.terms.size();
    const int first = P->first_term, last = P->last_term < 0 ? nterms : P->last_term;
    NEED(c, P->iteration >= 1, JWAS_HIP_EINVAL, "jwas_hip_locpar_step: iteration must be >= 1");
    NEED(c, first >= 0 && first <= last && last <= nterms, JWAS_HIP_EINVAL, "jwas_hip_locpar_step: terms %d..%d outside 0..%d", first, last, nterms);
    const bool pat = c->mt.weights;                             // the per-record Ri of jwas_hip_mtmiss_set_record_weights: Rinv is not read
    if (pat) {
        NEED(c, c->mt.active && c->mt.nt == t && t > 1, JWAS_HIP_ESTATE, "jwas_hip_init_state changed the number of traits after jwas_hip_mtmiss_begin");
    } else if (t == 1) {
        NEED(c, std::isfinite(P->vare) && P->vare > 0.0, JWAS_HIP_EINVAL, "jwas_hip_locpar_step: vare must be positive and finite (got %g)", P->vare);
    } else {
        for (int k = 0; k < t; ++k) {
            NEED(c, P->Rinv[k * t + k] > 0.0, JWAS_HIP_EINVAL, "jwas_hip_locpar_step: inv(R) needs a positive diagonal");
            for (int j = 0; j < t; ++j)
                NEED(c, std::isfinite(P->Rinv[k * t + j]) && P->Rinv[k * t + j] == P->Rinv[j * t + k], JWAS_HIP_EINVAL, "jwas_hip_locpar_step: inv(R) must be finite and symmetric");
        }
    }
    for (int g = 0; g < b.ngroups; ++g) {
        const int kk = b.groups[g].nmembers;
        for (int a = 0; a < kk; ++a) {
            NEED(c, P->Gi[16 * g + a * kk + a] > 0.0, JWAS_HIP_EINVAL, "jwas_hip_locpar_step: Gi of random effect %d needs a positive diagonal", g);
            for (int e = 0; e < kk; ++e)
                NEED(c, std::isfinite(P->Gi[16 * g + a * kk + e]) && P->Gi[16 * g + a * kk + e] == P->Gi[16 * g + e * kk + a], JWAS_HIP_EINVAL,
                     "jwas_hip_locpar_step: Gi of random effect %d must be finite and symmetric", g);
        }
    }
    if (int rc = locpar_finalize(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t esz = IS_F64(c) ? 8 : 4;
    if (pat && !b.part2) HIPCHK(c, b.mem.alloc(&b.part2, sizeof(double) * (size_t)b.maxp));
    const double* ctab = pat ? c->mt.tab + 2 * jwm::kMaxCodes * 16 : nullptr;
    if (S) { if (int rc = step_timer_begin(c)) return rc; }
    for (int j = first; j < last; ++j) {
        const auto& T = b.terms[(size_t)j];
        const int k = T.trait;
        if (T.npieces > 0) {
            jwp::SumArgs A = {};
            A.r = residual_ptr(c); A.ld = c->ld; A.rec = T.rec; A.wx = T.wx; A.piece_lo = T.piece_lo; A.part = b.part;
            A.npieces = T.npieces; A.G = T.G; A.nt = t; A.trait = k;
            for (int m = 0; m < t; ++m) A.c[m] = t == 1 ? 1.0 : pat ? 0.0 : P->Rinv[k * t + m];
            const dim3 grid((unsigned)(((int64_t)T.npieces * T.G + 255) / 256)), block(256);
            if (pat) { A.code = c->mt.code; A.ctab = ctab; A.x = T.x; A.part2 = b.part2; }
            with_real(c, [&](auto real) {
                using R = decltype(real);
                if (pat) hipLaunchKernelGGL((jwp::k_locpar_sums<R, true>), grid, block, 0, c->stream, A);
                else     hipLaunchKernelGGL((jwp::k_locpar_sums<R>), grid, block, 0, c->stream, A);
            });
        }
        jwp::DrawArgs D = {};
        D.part = b.part; D.level_piece = T.level_piece; D.d = T.d; D.sol = b.sol; D.delta = b.delta; D.off = T.off;
        D.nlevels = (int32_t)T.nlevels; D.pos = T.pos; D.npartners = 0;
        D.ckk = t == 1 ? 1.0 : pat ? 0.0 : P->Rinv[k * t + k];
        D.s = t == 1 ? P->vare : 1.0;
        D.part2 = pat ? b.part2 : nullptr;
        D.prior = 0.0;
        if (T.group >= 0) {
            const auto& g = b.groups[T.group];
            const int kk = g.nmembers;
            D.npartners = kk;
            for (int m = 0; m < kk; ++m) { D.partner_off[m] = b.terms[(size_t)g.term[m]].off; D.gi[m] = P->Gi[16 * T.group + T.pos * kk + m]; }
            D.prior = t == 1 ? P->vare * D.gi[T.pos] : D.gi[T.pos];
        }
        D.iter = P->iteration; D.rep = 0x20000000u | (uint32_t)j; D.slot = 3u + 16u * (uint32_t)k;
        split_seed(P->seed, D.seed_lo, D.seed_hi);
        if (T.group >= 0 && b.structs[T.group].set) {                   // a structured effect: colour by colour, one launch each
            const auto& V = b.structs[T.group];
            jwp::StructDrawArgs Q = {};
            Q.part = D.part; Q.level_piece = D.level_piece; Q.d = D.d; Q.sol = D.sol; Q.delta = D.delta; Q.off = D.off;
            Q.rowptr = V.rowptr; Q.col = V.col; Q.val = V.val;
            Q.npartners = D.npartners; Q.pos = D.pos; Q.ckk = D.ckk; Q.s = D.s;
            for (int m = 0; m < D.npartners; ++m) { Q.partner_off[m] = D.partner_off[m]; Q.p[m] = t == 1 ? P->vare * D.gi[m] : D.gi[m]; }
            Q.iter = D.iter; Q.rep = D.rep; Q.slot = D.slot; Q.seed_lo = D.seed_lo; Q.seed_hi = D.seed_hi; Q.part2 = D.part2;
            for (int col = 0; col < V.ncolors; ++col) {
                Q.lv = V.lv + V.color_lo[(size_t)col];
                Q.nshort = V.nshort[(size_t)col];
                Q.nlong = V.color_lo[(size_t)col + 1] - V.color_lo[(size_t)col] - Q.nshort;
                const unsigned wgs = (unsigned)((Q.nshort + 255) / 256 + (Q.nlong + 3) / 4);
                if (pat) hipLaunchKernelGGL(jwp::k_locpar_draw_structured<true>, dim3(wgs), dim3(256), 0, c->stream, Q);
                else     hipLaunchKernelGGL(jwp::k_locpar_draw_structured<false>, dim3(wgs), dim3(256), 0, c->stream, Q);
            }
        } else if (pat) {
            hipLaunchKernelGGL(jwp::k_locpar_draw<true>, dim3((unsigned)((T.nlevels + 255) / 256)), dim3(256), 0, c->stream, D);
        } else {
            hipLaunchKernelGGL(jwp::k_locpar_draw<false>, dim3((unsigned)((T.nlevels + 255) / 256)), dim3(256), 0, c->stream, D);
        }
        char* rk = (char*)residual_ptr(c) + esz * (size_t)k * (size_t)c->ld;
        const dim3 agrid((unsigned)((c->n + 255) / 256));
        with_real(c, [&](auto real) { hipLaunchKernelGGL((jwp::k_locpar_apply<decltype(real)>), agrid, dim3(256), 0, c->stream, (decltype(real)*)rk, T.x, T.level, b.delta, c->n); });
    }
    for (int g = 0; g < b.ngroups; ++g) {
        const int kk = b.groups[g].nmembers;
        if (kk > 0 && b.structs[g].set) {                                // U' V U
            const auto& V = b.structs[g];
            jwp::QuadArgs Q = {};
            Q.sol = b.sol; Q.rowptr = V.rowptr; Q.col = V.col; Q.val = V.val; Q.part = V.qpart; Q.nlevels = (int32_t)V.nlevels; Q.k = kk;
            for (int m = 0; m < kk; ++m) Q.member_off[m] = b.terms[(size_t)b.groups[g].term[m]].off;
            hipLaunchKernelGGL(jwp::k_locpar_quad_rows, dim3((unsigned)V.nwg), dim3(256), 0, c->stream, Q);
            hipLaunchKernelGGL(jwp::k_locpar_quad_reduce, dim3(1), dim3(256), 0, c->stream, V.qpart, (int32_t)V.nwg, (int32_t)kk, b.cross_out + (size_t)g * 16);
        } else if (kk > 0)
            hipLaunchKernelGGL(jwp::k_locpar_cross, dim3((unsigned)(kk * kk)), dim3(256), 0, c->stream, b.sol, b.cross_offs + (size_t)g * 32,
                               (int32_t)b.groups[g].nlevels, b.cross_out + (size_t)g * 16);
    }
    HIPCHK(c, hipGetLastError());
    if (S) {
        std::memset(S, 0, sizeof *S);
        return step_timer_end(c, S->utu, b.cross_out, sizeof(double) * jwp::kMaxGroups * 16, &S->step_ms);
    }
    return JWAS_HIP_OK;
}

int jwas_hip_locpar_accumulate(jwas_hip_ctx* c, double nsamples)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, nsamples >= 1.0, JWAS_HIP_EINVAL, "nsamples must be >= 1 (got %g)", nsamples);
    if (int rc = locpar_finalize(c)) return rc;
    auto& b = c->lp;
    if (b.q == 0) return JWAS_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(jwp::k_locpar_accumulate, dim3((unsigned)((b.q + 255) / 256)), dim3(256), 0, c->stream, b.sol, b.mean, b.mean2, b.q, nsamples);
    HIPCHK(c, hipGetLastError());
    return JWAS_HIP_OK;
}

int jwas_hip_locpar_get_means(jwas_hip_ctx* c, int64_t q, double* out_mean, double* out_mean2)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, out_mean, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, q == c->lp.q, JWAS_HIP_EINVAL, "q (%lld) differs from the number of location parameters (%lld)", (long long)q, (long long)c->lp.q);
    if (int rc = locpar_finalize(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(out_mean, c->lp.mean, sizeof(double) * (size_t)q, hipMemcpyDeviceToHost, c->stream));
    if (out_mean2) HIPCHK(c, hipMemcpyAsync(out_mean2, c->lp.mean2, sizeof(double) * (size_t)q, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

int jwas_hip_lp_set_group_structure(jwas_hip_ctx* c, int32_t group, int64_t nlevels, const int64_t* indptr, const int32_t* indices, const double* values)
{
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    if (int rc = refuse_shards(c, "location parameters")) return rc;
    if (int rc = need_locpar(c)) return rc;
    auto& b = c->lp;
    NEED(c, group >= 0 && group < jwp::kMaxGroups, JWAS_HIP_EINVAL, "random_group must be 0..%d (got %d)", jwp::kMaxGroups - 1, group);
    NEED(c, !b.finalized && b.groups[group].nmembers == 0, JWAS_HIP_ESTATE,
         "the structure of random effect %d is set before its first member term is added and before sol is first used", group);
    NEED(c, indptr && indices && values, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, nlevels >= 1 && nlevels < (int64_t)1 << 31, JWAS_HIP_EINVAL, "nlevels must be 1 .. 2^31 - 1 (got %lld)", (long long)nlevels);
    NEED(c, indptr[0] == 0, JWAS_HIP_EINVAL, "indptr[0] must be 0");
    for (int64_t l = 0; l < nlevels; ++l) {
        NEED(c, indptr[l + 1] >= indptr[l], JWAS_HIP_EINVAL, "indptr decreases at row %lld", (long long)l);
        bool diag = false;
        for (int64_t e = indptr[l]; e < indptr[l + 1]; ++e) {
            NEED(c, indices[e] >= 0 && indices[e] < nlevels, JWAS_HIP_EINVAL, "row %lld: column %d outside 0..%lld", (long long)l, indices[e], (long long)nlevels - 1);
            NEED(c, e == indptr[l] || indices[e] > indices[e - 1], JWAS_HIP_EINVAL, "row %lld: columns must be ascending without duplicates", (long long)l);
            NEED(c, std::isfinite(values[e]), JWAS_HIP_EINVAL, "row %lld, column %d: the value is not finite", (long long)l, indices[e]);
            if (indices[e] == l) { diag = true; NEED(c, values[e] > 0.0, JWAS_HIP_EINVAL, "row %lld: the diagonal must be positive (got %g)", (long long)l, values[e]); }
        }
        NEED(c, diag, JWAS_HIP_EINVAL, "row %lld has no diagonal entry", (long long)l);
    }
    for (int64_t l = 0; l < nlevels; ++l)                       // (every column index is in range from here on)
        for (int64_t e = indptr[l]; e < indptr[l + 1]; ++e) {
            const int32_t j = indices[e];
            const int32_t* lo = indices + indptr[j];
            const int32_t* hi = indices + indptr[j + 1];
            const int32_t* at = std::lower_bound(lo, hi, (int32_t)l);
            NEED(c, at != hi && *at == (int32_t)l && values[at - indices] == values[e], JWAS_HIP_EINVAL,
                 "the structure is not symmetric at (%lld, %d)", (long long)l, j);
        }
    const int64_t nnz = indptr[nlevels];
    // colours: levels in ascending order, the smallest colour no neighbour holds; then the levels of every colour, short rows first
    jwas_hip_ctx::Locpar::Structure V;
    V.nlevels = nlevels; V.nnz = nnz;
    V.color.assign((size_t)nlevels, -1);
    std::vector<int64_t> held;                                  // held[colour] == l + 1: a neighbour of l has it
    for (int64_t l = 0; l < nlevels; ++l) {
        for (int64_t e = indptr[l]; e < indptr[l + 1]; ++e) {
            const int32_t cj = indices[e] != l ? V.color[(size_t)indices[e]] : -1;
            if (cj >= 0) held[(size_t)cj] = l + 1;
        }
        int32_t pick = 0;
        while (pick < (int32_t)held.size() && held[(size_t)pick] == l + 1) ++pick;
        if (pick == (int32_t)held.size()) held.push_back(0);
        V.color[(size_t)l] = pick;
    }
    V.ncolors = (int)held.size();
    V.color_lo.assign((size_t)V.ncolors + 1, 0);
    V.nshort.assign((size_t)V.ncolors, 0);
    for (int64_t l = 0; l < nlevels; ++l) {
        ++V.color_lo[(size_t)V.color[(size_t)l] + 1];
        if (indptr[l + 1] - indptr[l] <= jwp::kLongRow) ++V.nshort[(size_t)V.color[(size_t)l]];
    }
    for (int q = 0; q < V.ncolors; ++q) V.color_lo[(size_t)q + 1] += V.color_lo[(size_t)q];
    std::vector<int32_t> lv((size_t)nlevels), at_short(V.color_lo.begin(), V.color_lo.end() - 1), at_long((size_t)V.ncolors);
    for (int q = 0; q < V.ncolors; ++q) at_long[(size_t)q] = V.color_lo[(size_t)q] + V.nshort[(size_t)q];
    for (int64_t l = 0; l < nlevels; ++l) {
        const size_t q = (size_t)V.color[(size_t)l];
        lv[(size_t)(indptr[l + 1] - indptr[l] <= jwp::kLongRow ? at_short[q]++ : at_long[q]++)] = (int32_t)l;
    }
    V.nwg = (int)((nlevels + 255) / 256);
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = locpar_upload(V.mem, &V.rowptr, std::vector<int64_t>(indptr, indptr + nlevels + 1));
    if (e == hipSuccess) e = locpar_upload(V.mem, &V.col, std::vector<int32_t>(indices, indices + nnz));
    if (e == hipSuccess) e = locpar_upload(V.mem, &V.val, std::vector<double>(values, values + nnz));
    if (e == hipSuccess) e = locpar_upload(V.mem, &V.lv, lv);
    if (e == hipSuccess) e = V.mem.alloc(&V.qpart, sizeof(double) * jwp::kMaxPairs * (size_t)V.nwg);
    if (e != hipSuccess) {
        V.mem.release();
        return fail(c, JWAS_HIP_EHIP, "uploading the structure failed: %s", hipGetErrorString(e));
    }
    auto& old = b.structs[group];                               // (a structure set twice: the later one holds)
    old.mem.release();
    V.set = true;
    old = std::move(V);
    return JWAS_HIP_OK;
}

int jwas_hip_lp_get_group_colors(jwas_hip_ctx* c, int32_t group, int64_t nlevels, int32_t* out_color, int32_t* out_ncolors)
{
    if (int rc = need_locpar(c)) return rc;
    NEED(c, group >= 0 && group < jwp::kMaxGroups, JWAS_HIP_EINVAL, "random_group must be 0..%d (got %d)", jwp::kMaxGroups - 1, group);
    const auto& V = c->lp.structs[group];
    NEED(c, V.set, JWAS_HIP_EINVAL, "random effect %d has no structure", group);
    NEED(c, nlevels == V.nlevels, JWAS_HIP_EINVAL, "nlevels (%lld) differs from the structure's (%lld)", (long long)nlevels, (long long)V.nlevels);
    NEED(c, out_color && out_ncolors, JWAS_HIP_EINVAL, "NULL argument");
    std::copy(V.color.begin(), V.color.end(), out_color);
    *out_ncolors = V.ncolors;
    return JWAS_HIP_OK;
}

int64_t jwas_hip_lp_structure_estimate_bytes(int64_t nlevels, int64_t nnz)
{
    // the row pointers (int64), columns (int32) and values (double) of V, the levels colour by colour (int32), the per-workgroup
    // sums of the quadratic forms
    return 8 * (nlevels + 1) + 12 * nnz + 4 * nlevels + (int64_t)sizeof(double) * jwp::kMaxPairs * (nlevels / 256 + 1);
}

int64_t jwas_hip_locpar_estimate_bytes(int64_t n, int64_t nterms, int64_t total_levels)
{
    // per term: x, w x (doubles), level, the sorted records (int32), the piece starts and piece sums of its full pieces; per entry
    // of sol: sol, two means, d, delta, one piece sum (doubles), the level's piece range and one piece start of its own (int32)
    return nterms * (24 * n + 12 * (n / jwp::kPiece + 2)) + total_levels * (6 * 8 + 2 * 4) + (int64_t)sizeof(double) * jwp::kMaxGroups * 16 * 3;
}

int jwas_hip_locpar_end(jwas_hip_ctx* c) { return session_drop(c, locpar_free); }

}  // extern "C"
