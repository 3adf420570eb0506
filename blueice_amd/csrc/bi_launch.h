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
