// session_plink.hip -- PLINK 1 binary filesets into packed storage (plink.hpp), jwas_hip_plink_scan .. _commit / _discard, and
// jwas_hip_get_packed2bit: the device side of prepare_streaming_genotypes (streaming_genotypes.jl:499-656,819-877) for a .bed file.
#include "ctx.hpp"
#include "plink.hpp"

#include <cstdio>

void plink_free(jwas_hip_ctx* c) { DevOwner::reset(c->pk); }

namespace {

// what a scan holds only while it runs: the open file, two pinned chunks and their device copies, the events that say a pair is free again
struct ScanScratch {
    FILE* f = nullptr;
    void* pin[2] = {};
    uint8_t* raw[2] = {};
    hipEvent_t done[2] = {};
    int32_t* rows = nullptr;
    ~ScanScratch()
    {
        if (f) std::fclose(f);
        for (int k = 0; k < 2; ++k) {
            if (pin[k]) (void)hipHostFree(pin[k]);
            (void)hipFree(raw[k]);
            if (done[k]) (void)hipEventDestroy(done[k]);
        }
        (void)hipFree(rows);
    }
};

}  // namespace

extern "C" {

int jwas_hip_plink_scan(jwas_hip_ctx* c, const char* bed_path, int64_t n_file, int64_t p_file, const int64_t* rows, int64_t n_rows,
                        int32_t count_a1, int64_t* counts)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c && bed_path && counts, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, n_file > 0 && p_file > 0, JWAS_HIP_EINVAL, "the fileset must be non-empty (n_file=%lld, p_file=%lld)", (long long)n_file, (long long)p_file);
    NEED(c, n_file < (1ll << 31) && p_file < (1ll << 31), JWAS_HIP_EUNSUP, "n_file=%lld / p_file=%lld exceeds the 2^31 limit of one context", (long long)n_file, (long long)p_file);
    const int64_t nr = rows ? n_rows : n_file;
    std::vector<int32_t> rows32;
    if (rows) {
        NEED(c, n_rows > 0, JWAS_HIP_EINVAL, "n_rows must be positive (got %lld)", (long long)n_rows);
        rows32.assign((size_t)round_up(n_rows, 16), 0);
        std::vector<bool> seen((size_t)n_file, false);
        for (int64_t i = 0; i < n_rows; ++i) {
            NEED(c, rows[i] >= 0 && rows[i] < n_file, JWAS_HIP_EINVAL, "rows[%lld] = %lld outside [0,%lld)", (long long)i, (long long)rows[i], (long long)n_file);
            NEED(c, !seen[(size_t)rows[i]], JWAS_HIP_EINVAL, "rows[%lld] = %lld is listed twice", (long long)i, (long long)rows[i]);
            seen[(size_t)rows[i]] = true;
            rows32[(size_t)i] = (int32_t)rows[i];
        }
    }
    ScanScratch S;
    const int64_t bpm = (n_file + 3) / 4;                       // bytes per marker in the file
    S.f = std::fopen(bed_path, "rb");
    NEED(c, S.f, JWAS_HIP_EINVAL, "PLINK .bed file is not found: %s", bed_path);
    unsigned char magic[3] = {};
    NEED(c, std::fread(magic, 1, 3, S.f) == 3 && magic[0] == 0x6C && magic[1] == 0x1B, JWAS_HIP_EINVAL, "%s is not a PLINK 1 .bed file (magic bytes 6C 1B)", bed_path);
    NEED(c, magic[2] == 0x01, JWAS_HIP_EINVAL, "%s: mode byte %02X: only variant-major .bed files (mode 01) are read", bed_path, (unsigned)magic[2]);
    std::fseek(S.f, 0, SEEK_END);
    const int64_t fsz = (int64_t)std::ftell(S.f);
    NEED(c, fsz == 3 + p_file * bpm, JWAS_HIP_EINVAL, "%s has %lld bytes; %lld individuals x %lld markers need %lld", bed_path, (long long)fsz,
         (long long)n_file, (long long)p_file, (long long)(3 + p_file * bpm));
    std::fseek(S.f, 3, SEEK_SET);
    if (int rc = session_drop(c, plink_free)) return rc;        // (an earlier scan that was never committed)

    auto& b = c->pk;
    b.n_rows = nr; b.p_file = p_file; b.ld = round_up(nr, jwas_hip_ctx::kRowPad);
    const int64_t sb = b.ld >> 2, rpitch = round_up(bpm, 16);
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(1, (64ll << 20) / rpitch), std::min<int64_t>(p_file, 1ll << 20));      // <= 64 MB of markers at a time
    long long* d_counts = nullptr;
    if (int rc = alloc_or_nomem(c, b.mem, &b.stage, (size_t)sb * p_file + 1024, "jwas_hip_plink_scan", plink_free)) return rc;
    if (int rc = alloc_or_nomem(c, b.mem, &d_counts, sizeof(long long) * 4 * (size_t)p_file, "jwas_hip_plink_scan", plink_free)) return rc;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = hipHostMalloc(&S.pin[k], (size_t)(chunk * bpm));
        if (e == hipSuccess) e = hipMalloc(&S.raw[k], (size_t)(chunk * rpitch));
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S.done[k], hipEventDisableTiming);
    }
    if (e == hipSuccess && rows) {
        e = hipMalloc(&S.rows, sizeof(int32_t) * rows32.size());
        if (e == hipSuccess) e = hipMemcpyAsync(S.rows, rows32.data(), sizeof(int32_t) * rows32.size(), hipMemcpyHostToDevice, c->stream);
    }
    const int mode = !rows ? jwk::kDirect : rpitch <= jwk::kMaxLdsRow ? jwk::kGatherLds : jwk::kGatherGlobal;
    const size_t lds = 64 + (mode == jwk::kGatherLds ? (size_t)rpitch : 0);
    bool short_read = false;
    // chunk k is read from the file while chunk k - 1 is copied and transcoded; a buffer pair is reused once its chunk's kernel has finished
    for (int64_t j0 = 0, k = 0; e == hipSuccess && j0 < p_file; j0 += chunk, ++k) {
        const int64_t m = std::min(chunk, p_file - j0);
        const int s = (int)(k & 1);
        if (k >= 2) e = hipEventSynchronize(S.done[s]);
        if (e != hipSuccess) break;
        if ((int64_t)std::fread(S.pin[s], (size_t)bpm, (size_t)m, S.f) != m) { short_read = true; break; }
        e = hipMemcpy2DAsync(S.raw[s], (size_t)rpitch, S.pin[s], (size_t)bpm, (size_t)bpm, (size_t)m, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        jwk::TranscodeArgs A = {};
        A.raw = S.raw[s]; A.rpitch = rpitch; A.out = b.stage + j0 * sb; A.sb = sb; A.counts = d_counts + j0 * 4;
        A.rows = S.rows; A.n_rows = nr; A.count_a1 = count_a1 ? 1 : 0;
        const dim3 grid((unsigned)m), block(jwk::kThreads);
        if (mode == jwk::kDirect) hipLaunchKernelGGL(jwk::k_plink_transcode<jwk::kDirect>, grid, block, lds, c->stream, A);
        else if (mode == jwk::kGatherLds) hipLaunchKernelGGL(jwk::k_plink_transcode<jwk::kGatherLds>, grid, block, lds, c->stream, A);
        else hipLaunchKernelGGL(jwk::k_plink_transcode<jwk::kGatherGlobal>, grid, block, lds, c->stream, A);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(S.done[s], c->stream);
    }
    if (e == hipSuccess && !short_read) e = hipMemcpyAsync(counts, d_counts, sizeof(long long) * 4 * (size_t)p_file, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);  // (always: the scratch buffers go away behind this)
    if (e == hipSuccess) e = e_sync;
    if (short_read || e != hipSuccess) {
        plink_free(c);
        if (short_read) return fail(c, JWAS_HIP_EINVAL, "jwas_hip_plink_scan: %s ended early", bed_path);
        return fail(c, JWAS_HIP_EHIP, "jwas_hip_plink_scan: uploading / transcoding %s failed (%s)", bed_path, hipGetErrorString(e));
    }
    b.mem.free_one(d_counts);
    b.pending = true;
    return JWAS_HIP_OK;
}

int jwas_hip_plink_commit(jwas_hip_ctx* c, const int64_t* selected, int64_t p_sel, const float* means, int32_t centered)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, c->pk.pending, JWAS_HIP_ESTATE, "jwas_hip_plink_scan has not been called (or its scan was dropped by a later load)");
    NEED(c, selected && means, JWAS_HIP_EINVAL, "selected / means is NULL");
    const int64_t p_file = c->pk.p_file, n = c->pk.n_rows;
    NEED(c, p_sel > 0 && p_sel <= p_file, JWAS_HIP_EINVAL, "p_sel (%lld) outside [1,%lld]", (long long)p_sel, (long long)p_file);
    for (int64_t j = 0; j < p_sel; ++j)
        NEED(c, selected[j] >= 0 && selected[j] < p_file && (j == 0 || selected[j] > selected[j - 1]), JWAS_HIP_EINVAL,
             "selected must be strictly ascending within [0,%lld) (entry %lld: %lld)", (long long)p_file, (long long)j, (long long)selected[j]);
    HIPCHK(c, hipSetDevice(c->device));
    // the staging buffer leaves the pending scan: alloc_storage frees whatever the context holds, scans included
    uint8_t* stage = c->pk.stage;
    c->pk.mem.ptrs.clear();
    plink_free(c);
    if (p_sel == p_file) {                                      // every marker stays: the staging buffer becomes the storage
        if (int rc = alloc_storage(c, n, p_sel, true, stage)) return rc;
    } else {
        DevOwner tmp;
        tmp.ptrs.push_back(stage);
        int64_t* d_sel = nullptr;
        int rc = alloc_storage(c, n, p_sel, true);
        hipError_t e = hipSuccess;
        if (!rc) {
            e = tmp.alloc(&d_sel, sizeof(int64_t) * (size_t)p_sel);
            if (e == hipSuccess) e = hipMemcpyAsync(d_sel, selected, sizeof(int64_t) * (size_t)p_sel, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(jwk::k_plink_compact, dim3((unsigned)p_sel), dim3(jwk::kThreads), 0, c->stream, stage, c->Q, c->ld >> 2, d_sel);
                e = hipGetLastError();
            }
            const hipError_t e_sync = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = e_sync;
        }
        tmp.release();
        if (rc) return rc;
        if (e != hipSuccess) return fail(c, JWAS_HIP_EHIP, "jwas_hip_plink_commit: compacting the kept markers failed (%s)", hipGetErrorString(e));
    }
    c->centered = centered ? 1 : 0;
    HIPCHK(c, hipMemcpyAsync(c->qmean, means, sizeof(float) * (size_t)p_sel, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// The scanned individuals become the context's packed OUTPUT rows (Mi.output_genotypes, tools4genotypes.jl:290-296, for the output_ID
// of check_outputID, input_data_validation.jl:143-196): the staging rows of the training selection, nothing else of the context changes.
int jwas_hip_plink_commit_output(jwas_hip_ctx* c, const int64_t* selected, int64_t p_sel)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c, JWAS_HIP_EINVAL, "ctx is NULL");
    NEED(c, c->pk.pending, JWAS_HIP_ESTATE, "jwas_hip_plink_scan has not been called (or its scan was dropped by a later load)");
    NEED(c, c->packed && c->Q, JWAS_HIP_ESTATE, "packed output rows need 2-bit packed training storage: their means and centring are its own");
    NEED(c, selected, JWAS_HIP_EINVAL, "selected is NULL");
    const int64_t p_file = c->pk.p_file, n_out = c->pk.n_rows, ld = c->pk.ld, sb = ld >> 2;
    NEED(c, p_sel == c->p, JWAS_HIP_EINVAL, "p_sel (%lld) differs from the training matrix's %lld markers: the selection is the training set's", (long long)p_sel,
         (long long)c->p);
    NEED(c, p_sel <= p_file, JWAS_HIP_EINVAL, "p_sel (%lld) exceeds the scanned file's %lld markers", (long long)p_sel, (long long)p_file);
    for (int64_t j = 0; j < p_sel; ++j)
        NEED(c, selected[j] >= 0 && selected[j] < p_file && (j == 0 || selected[j] > selected[j - 1]), JWAS_HIP_EINVAL,
             "selected must be strictly ascending within [0,%lld) (entry %lld: %lld)", (long long)p_file, (long long)j, (long long)selected[j]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint8_t* q = nullptr;
    if (p_sel == p_file) {                                      // every marker stays: the staging buffer becomes the output rows
        q = c->pk.stage;
        c->pk.mem.ptrs.clear();
        plink_free(c);
    } else {
        DevOwner tmp;
        int64_t* d_sel = nullptr;
        hipError_t e = hipMalloc(&q, (size_t)sb * p_sel);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            plink_free(c);
            return fail(c, JWAS_HIP_ENOMEM, "jwas_hip_plink_commit_output: device allocation of %zu bytes failed", (size_t)sb * p_sel);
        }
        e = tmp.alloc(&d_sel, sizeof(int64_t) * (size_t)p_sel);
        if (e == hipSuccess) e = hipMemcpyAsync(d_sel, selected, sizeof(int64_t) * (size_t)p_sel, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(jwk::k_plink_compact, dim3((unsigned)p_sel), dim3(jwk::kThreads), 0, c->stream, c->pk.stage, q, sb, d_sel);
            e = hipGetLastError();
        }
        const hipError_t e_sync = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = e_sync;
        tmp.release();
        plink_free(c);                                          // (the pending scan is consumed)
        if (e != hipSuccess) {
            (void)hipFree(q);
            return fail(c, JWAS_HIP_EHIP, "jwas_hip_plink_commit_output: compacting the kept markers failed (%s)", hipGetErrorString(e));
        }
    }
    drop_output_rows(c);
    c->load_mem.ptrs.push_back(q);
    c->Qout = q; c->n_out = n_out; c->ld_out = ld;
    return JWAS_HIP_OK;
}

int jwas_hip_plink_discard(jwas_hip_ctx* c)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    return session_drop(c, plink_free);
}

int jwas_hip_get_packed2bit(jwas_hip_ctx* c, int64_t j0, int64_t m, uint8_t* out, int64_t stride_bytes)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c && out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, c->packed && c->Q, JWAS_HIP_ESTATE, "the context holds no 2-bit packed genotypes (see jwas_hip_storage_info)");
    NEED(c, j0 >= 0 && m >= 0 && j0 + m <= c->p, JWAS_HIP_EINVAL, "marker range [%lld,%lld) outside [0,%lld)", (long long)j0, (long long)(j0 + m), (long long)c->p);
    const int64_t width = (c->n + 3) / 4;
    NEED(c, stride_bytes >= width, JWAS_HIP_EINVAL, "stride_bytes (%lld) must be >= cld(n,4) = %lld", (long long)stride_bytes, (long long)width);
    HIPCHK(c, hipSetDevice(c->device));
    if (m == 0) return JWAS_HIP_OK;
    const size_t sb = (size_t)(c->ld >> 2);
    HIPCHK(c, hipMemcpy2DAsync(out, (size_t)stride_bytes, c->Q + j0 * sb, sb, (size_t)width, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

// ... and of the packed output rows: cld(n_out,4) bytes of every marker, the .jgb2 payload of the output individuals
// (streaming_genotypes.jl:600-654)
int jwas_hip_get_output_packed2bit(jwas_hip_ctx* c, int64_t j0, int64_t m, uint8_t* out, int64_t stride_bytes)
{
    if (c) NOT_F64(c, "2-bit packed storage");
    NEED(c, c && out, JWAS_HIP_EINVAL, "NULL argument");
    NEED(c, c->Qout, JWAS_HIP_ESTATE, "the context holds no 2-bit packed output rows (jwas_hip_load_output_packed2bit, jwas_hip_plink_commit_output)");
    NEED(c, j0 >= 0 && m >= 0 && j0 + m <= c->p, JWAS_HIP_EINVAL, "marker range [%lld,%lld) outside [0,%lld)", (long long)j0, (long long)(j0 + m), (long long)c->p);
    const int64_t width = (c->n_out + 3) / 4;
    NEED(c, stride_bytes >= width, JWAS_HIP_EINVAL, "stride_bytes (%lld) must be >= cld(n_out,4) = %lld", (long long)stride_bytes, (long long)width);
    HIPCHK(c, hipSetDevice(c->device));
    if (m == 0) return JWAS_HIP_OK;
    const size_t sb = (size_t)(c->ld_out >> 2);
    HIPCHK(c, hipMemcpy2DAsync(out, (size_t)stride_bytes, c->Qout + j0 * sb, sb, (size_t)width, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return JWAS_HIP_OK;
}

}  // extern "C"
