// bi_launch.h -- mailbox set-up of in-launch finishing, the k_finish launch and state checks (main translation unit).  The
// instantiation tables of the heavy kernel families are in tu_*.hip, declared in bi_common.h.
#pragma once

namespace {

// the mailbox of in-launch finishing: allocated and emptied once (every collector leaves its slots empty again)
constexpr int64_t kMailSlots = (int64_t)1 << 20;       // 8 MB
constexpr int64_t kMailFlagWords = (int64_t)1 << 16;

int ensure_mail(bi_ctx* c) {
    if (c->mail.p) return BI_OK;
    void* p = nullptr;
    void* f = nullptr;
    // not from the recycle cache: these must keep their contents between calls
    if (hipMalloc(&p, (size_t)kMailSlots * sizeof(double)) != hipSuccess) return BI_ERR_NOMEM;
    if (hipMalloc(&f, (size_t)kMailFlagWords * sizeof(unsigned)) != hipSuccess) { (void)hipFree(p); return BI_ERR_NOMEM; }
    hipLaunchKernelGGL(k_mail_init, dim3((unsigned)((kMailSlots + 255) / 256)), dim3(256), 0, c->stream, (unsigned long long*)p, kMailSlots);
    if (hipGetLastError() != hipSuccess || hipMemsetAsync(f, 0, (size_t)kMailFlagWords * sizeof(unsigned), c->stream) != hipSuccess) {
        (void)hipFree(p);
        (void)hipFree(f);
        return BI_ERR_HIP;
    }
    c->mail.p = p; c->mail.bytes = (size_t)kMailSlots * sizeof(double); c->mail.owner = nullptr;
    c->mail_flags.p = f; c->mail_flags.bytes = (size_t)kMailFlagWords * sizeof(unsigned); c->mail_flags.owner = nullptr;
    return BI_OK;
}

// a launch that finishes through the mailbox: the collector's patience, and the injected faults (consumed here)
void arm_mail(bi_ctx* c, LaunchArgs& a) {
    a.mail_timeout = c->mail_timeout_ms * kMailTicksPerMs;
    a.skip_post = (int)c->debug_skip_post;
    a.late_post = (int)c->debug_late_post;
    c->debug_skip_post = c->debug_late_post = -1;
}

// after a collector gave up (BI_ST_INTERNAL) the mailbox may hold values nobody took: empty it again
void reset_mail(bi_ctx* c) {
    if (!c->mail.p) return;
    ++c->n_mail_resets;
    (void)hipStreamSynchronize(c->stream);
    hipLaunchKernelGGL(k_mail_init, dim3((unsigned)((kMailSlots + 255) / 256)), dim3(256), 0, c->stream, (unsigned long long*)c->mail.p, kMailSlots);
    (void)hipMemsetAsync(c->mail_flags.p, 0, (size_t)kMailFlagWords * sizeof(unsigned), c->stream);
    (void)hipStreamSynchronize(c->stream);
}

int check_ready(bi_ctx* c, bool need_data) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    if (!c->model_ready) return fail(c, BI_ERR_STATE, "no model uploaded (prepare() first)");
    if (need_data && !c->data_ready) return fail(c, BI_ERR_STATE, "no data uploaded (set_data() first)");
    return BI_OK;
}

int n_tiles_of(const bi_ctx* c) { return (int)(c->Bp / kTile); }

// ---- the narrow copy of the dense counts ----
// Called by every writer of c->counts [T][Bp] after its last write is queued and BEFORE its own stream synchronisation, which
// also brings the per-dataset flags to the host: no synchronisation of its own.  Failing to allocate the extra byte per
// bin is not an error: the context then simply has no narrow copy.
void build_narrow_counts(bi_ctx* c, int64_t T) {
    c->cnt8_valid = false;
    c->cnt8_all = -1;
    if (c->unbinned || T < 1 || !c->counts.p) return;
    const std::string keep = c->err;
    if (dev_alloc(c, c->cnt8, (size_t)T * c->Bp) || dev_alloc(c, c->cnt8_bad, (size_t)T * sizeof(unsigned))) {
        (void)hipGetLastError();
        c->err = keep;
        return;
    }
    if (hipMemsetAsync(c->cnt8_bad.p, 0, (size_t)T * sizeof(unsigned), c->stream) != hipSuccess) { (void)hipGetLastError(); return; }
    const unsigned nbx = (unsigned)((c->Bp + (int64_t)kThreads * kNarrowPerThread - 1) / ((int64_t)kThreads * kNarrowPerThread));
    const int64_t chunk = 32768;  // datasets per launch (gridDim.y limit)
    for (int64_t t0 = 0; t0 < T; t0 += chunk)
        hipLaunchKernelGGL(k_counts_narrow, dim3(nbx, (unsigned)std::min(chunk, T - t0)), dim3(kThreads), 0, c->stream,
                           (const double*)c->counts.p + t0 * c->Bp, c->B, c->Bp, (uint8_t*)c->cnt8.p + t0 * c->Bp, (unsigned*)c->cnt8_bad.p + t0);
    c->h_cnt8_bad.assign((size_t)T, 1u);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(c->h_cnt8_bad.data(), c->cnt8_bad.p, (size_t)T * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    c->cnt8_valid = true;
}

// is there a narrow copy that dense launches may read at all ...
bool narrow_on(const bi_ctx* c) { return c->narrow_counts && c->cnt8_valid && !c->unbinned && c->dense_counts; }
// ... does it represent dataset ds exactly ...
bool narrow_has(const bi_ctx* c, int64_t ds) {
    return c->cnt8_valid && ds >= 0 && ds < (int64_t)c->h_cnt8_bad.size() && c->h_cnt8_bad[(size_t)ds] == 0u;
}
// ... and every one of the T datasets (batches planned on the device: their dataset list exists only there)
bool narrow_has_all(bi_ctx* c) {
    if (!c->cnt8_valid) return false;
    if (c->cnt8_all < 0) c->cnt8_all = std::all_of(c->h_cnt8_bad.begin(), c->h_cnt8_bad.end(), [](uint32_t f) { return f == 0u; }) ? 1 : 0;
    return c->cnt8_all == 1;
}

// ---- the packed shadow of the template rows ----
// Called at the end of every model upload (bi_model_end), after the last write to c->ps is queued; every writer of c->ps runs
// between bi_model_begin -- which drops the shadow -- and bi_model_end.  Not having one is never an error: parameter off,
// more than a quarter of the free device memory, a failed allocation or a model without a packed form all leave the
// context streaming ps.  Synchronises the stream (the eligibility word comes to the host).
void drop_packed_rows(bi_ctx* c, bool release) {
    c->pk_valid = false;
    if (release) { dev_free(c->pk); dev_free(c->pk_base); }
}

void build_packed_rows(bi_ctx* c) {
    c->pk_valid = false;
    if (!c->packed_rows || c->pk_skip || c->unbinned || c->bb_source >= 0 || !c->ps.p || c->B < 1) { drop_packed_rows(c, true); return; }
    const int64_t n_chunks = c->A * c->S * (c->Bp / kTile);
    const size_t pk_bytes = (size_t)n_chunks * kPkChunk;
    const size_t base_bytes = ((size_t)n_chunks + 2) / 2 * sizeof(uint32_t);        // (read two bases at a time)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); drop_packed_rows(c, true); return; }
    if (!(c->pk.p && c->pk.bytes >= pk_bytes) && pk_bytes > free_b / 4) { drop_packed_rows(c, true); return; }
    const std::string keep = c->err;
    if (dev_alloc(c, c->pk, pk_bytes) || dev_alloc(c, c->pk_base, base_bytes) || dev_alloc(c, c->pk_bad, sizeof(unsigned))) {
        (void)hipGetLastError();
        c->err = keep;
        drop_packed_rows(c, true);
        return;
    }
    unsigned bad = 1u;
    hipError_t e = hipMemsetAsync(c->pk_bad.p, 0, sizeof(unsigned), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->pk_base.p, 0, base_bytes, c->stream);
    const int64_t per_launch = (int64_t)1 << 30;             // chunks per launch (gridDim.x limit)
    for (int64_t q0 = 0; q0 < n_chunks && e == hipSuccess; q0 += per_launch) {
        hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)std::min(per_launch, n_chunks - q0)), dim3(kThreads), 0, c->stream,
                           (const double*)c->ps.p, q0, (uint8_t*)c->pk.p, (uint16_t*)c->pk_base.p, (unsigned*)c->pk_bad.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, c->pk_bad.p, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); drop_packed_rows(c, true); return; }
    if (bad != 0u) { drop_packed_rows(c, true); return; }    // no packed form: the memory goes back
    c->pk_valid = true;
}

// may a dense value launch read the shadow (a property of the model, not of the batch)
bool packed_on(const bi_ctx* c) { return c->packed_rows && c->pk_valid && !c->unbinned && c->bb_source < 0 && c->pk.p; }

void use_packed_rows(bi_ctx* c, LaunchArgs& a) {
    a.pk = (const uint8_t*)c->pk.p;
    a.pk_base = (const uint32_t*)c->pk_base.p;
    ++c->n_packed_launches;
}

// k_finish over n_slots (item, slot) sums, G slots per item, of nbx per-block partials each: 64 lanes per slot up to 64
// blocks, else a whole block
void launch_finish(bi_ctx* c, const double* partial, const unsigned* pflags, int nbx, int G, int64_t n_slots, const int64_t* perm,
                   const double* slot_lg, double* out, int32_t* status) {
    const int lanes = nbx > 64 ? kThreads : 64;
    const int per_block = kThreads / lanes;
    hipLaunchKernelGGL(k_finish, dim3((unsigned)((n_slots + per_block - 1) / per_block)), dim3(kThreads), 0, c->stream, partial, pflags,
                       nbx, G, lanes, n_slots, perm, slot_lg, out, status);
}

}  // namespace
