// bi_sourcewise_nonempty.h -- source-wise models: the non-empty-bin form of the data (host half; the kernels are
// k_sourcewise_nonempty and k_sourcewise_gather, bi_k_sourcewise_nonempty.h).  bi_sourcewise_build_nonempty, bi_sourcewise_drop_nonempty.
//
// The dense store of bi_factored.h makes every evaluation of every point walk all B bins.  Templates of a source-wise model are
// finite and >= 0 and rates outside [0, inf) are BI_ST_UNPHYSICAL, so mu_b >= 0 everywhere and, without any further condition,
//     ll = sum_{b in Z_t} n_b log mu_b  -  sum_s lambda_s  -  sum_b lgamma(n_b + 1),     lambda_s = r_s sum_c w_c R_{s,c}
// with Z_t = {b : n_b != 0} in ascending bin order and R_{s,c} the total of anchor row (s, c) over ALL bins (h_rowsum, summed in
// long double where bi_factored_set_anchor has the row on the host; it does not depend on the data, so there are no per-dataset
// row totals as the grid model's h_Tz).  The gradient follows from g_b = n_b / mu_b at the listed bins and N_s = sum_c w_c R_{s,c}:
//     d ll / d rs_s = M_s (sum_Z g tau_s - N_s)
//     d ll / d z_i  = sum_{s: i in O_s} rs_s [M_s (sum_Z g ups_s,i - d_i N_s) + d_i M_s (sum_Z g tau_s - N_s)]
// (factored_eval, bi_factored.h: the subtractions on the host, then FacBatch::gradient unchanged).
//
// The form: the lists are built from the dense counts on the device (k_nz_count / k_nz_scatter of the grid model, which take a
// counts pointer), then per dataset a compacted copy of ALL the model's rows over its list, [rows][np_t] with np_t the list
// length padded to whole tiles (at least one), and its compacted counts [np_t]; templates and counts are 0 in the padding, so a
// padded bin contributes exactly nothing.  The rows of a source-wise model are few (sum_s prod n_i, 20 - 100), so the copy is a
// plain gather, one thread per (compact bin, row, dataset), a few launches per call.  The list keeps bin order: that order fixes
// the bits.
//
// Nothing builds the form unless asked; where it is built and the parameter sourcewise_form is 1, bi_eval_factored (and through
// it bi_fit_batched_factored), bi_eval_sourcewise_planned and bi_sample_stretch_sourcewise run on it.  Every other source-wise
// call keeps reading the dense store, which stays resident and valid.  Released by whatever replaces the counts or the model
// (fac_drop_nonempty, bi_factored.h).
#pragma once

namespace {

int sourcewise_build_nonempty(bi_ctx* c, int64_t* nnz_out) {
    const char* who = "bi_sourcewise_build_nonempty";
    bi_ctx::Factored& m = c->fac;
    fac_drop_nonempty(m);
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t T = m.T, B = m.B, Bp = m.Bp, rows = m.row_first[(size_t)m.S];
    const int nchunks = (int)((B + kNzChunk - 1) / kNzChunk);
    const int64_t tchunk = 32768;
    int rc;
    ScratchBuf d_cnt, d_off, d_nz_off, nz_idx, nz_n;
    if ((rc = dev_alloc(c, d_cnt, (size_t)T * nchunks * sizeof(int32_t)))) return rc;
    for (int64_t t0 = 0; t0 < T; t0 += tchunk) {
        const int64_t n = std::min(tchunk, T - t0);
        hipLaunchKernelGGL(k_nz_count, dim3((unsigned)nchunks, (unsigned)n), dim3(kThreads), 0, c->stream,
                           (const double*)m.counts.p + t0 * Bp, B, Bp, (int32_t*)d_cnt.p + t0 * nchunks, nchunks);
    }
    std::vector<int32_t> h_cnt((size_t)T * nchunks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt.data(), d_cnt.p, h_cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s (count): %s", who, hipGetErrorString(e));

    // the lists' offsets, and the layout of the compacted copies
    std::vector<int64_t> h_off(h_cnt.size()), nz_off((size_t)T + 1, 0), tab((size_t)3 * T);
    int64_t run = 0, tot_ps = 0, tot_cnt = 0, max_np = kTile;
    for (int64_t t = 0; t < T; ++t) {
        nz_off[(size_t)t] = run;
        for (int k = 0; k < nchunks; ++k) { h_off[(size_t)t * nchunks + k] = run; run += h_cnt[(size_t)t * nchunks + k]; }
        const int64_t nnz = run - nz_off[(size_t)t];
        const int64_t np = std::max<int64_t>(kTile, (nnz + kTile - 1) / kTile * kTile);
        tab[(size_t)t] = tot_ps;
        tab[(size_t)(T + t)] = np;
        tab[(size_t)(2 * T + t)] = tot_cnt;
        tot_ps += rows * np;
        tot_cnt += np;
        max_np = std::max(max_np, np);
        if (nnz_out) nnz_out[t] = nnz;
    }
    nz_off[(size_t)T] = run;
    const int64_t bytes = (tot_ps + tot_cnt) * (int64_t)sizeof(double);
    if (bytes > c->compact_budget)
        return fail(c, BI_ERR_INVALID, "%s: the compacted copies of %lld datasets (%lld listed bins, %lld rows) take %lld bytes, more than "
                    "compact_budget = %lld: nothing is built, the dense store stays in use",
                    who, (long long)T, (long long)run, (long long)rows, (long long)bytes, (long long)c->compact_budget);

    if ((rc = dev_upload(c, d_off, h_off)) || (rc = dev_upload(c, d_nz_off, nz_off)) ||
        (rc = dev_alloc(c, nz_idx, (size_t)std::max<int64_t>(run, 1) * sizeof(int32_t))) ||
        (rc = dev_alloc(c, nz_n, (size_t)std::max<int64_t>(run, 1) * sizeof(double))) ||
        (rc = dev_alloc(c, m.ne_ps, (size_t)tot_ps * sizeof(double))) || (rc = dev_alloc(c, m.ne_cnt, (size_t)tot_cnt * sizeof(double))) ||
        (rc = dev_upload(c, m.ne_tab, tab))) {
        (void)hipStreamSynchronize(c->stream);
        fac_drop_nonempty(m);
        return rc;
    }
    for (int64_t t0 = 0; t0 < T; t0 += tchunk) {
        const int64_t n = std::min(tchunk, T - t0);
        hipLaunchKernelGGL(k_nz_scatter, dim3((unsigned)nchunks, (unsigned)n), dim3(kThreads), 0, c->stream,
                           (const double*)m.counts.p + t0 * Bp, B, Bp, (const int64_t*)d_off.p + t0 * nchunks, nchunks,
                           (int32_t*)nz_idx.p, (double*)nz_n.p);
    }
    // the gather: grid (blocks of the longest list, rows + the counts, datasets), cut so that a launch stays below 2^22 blocks
    SourcewiseGatherArgs g{};
    g.ps = (const double*)m.ps.p;
    g.nz_idx = (const int32_t*)nz_idx.p;
    g.nz_n = (const double*)nz_n.p;
    g.nz_off = (const int64_t*)d_nz_off.p;
    g.ne_off = (const int64_t*)m.ne_tab.p;
    g.ne_np = g.ne_off + T;
    g.ne_cnt_off = g.ne_off + 2 * T;
    g.out_ps = (double*)m.ne_ps.p;
    g.out_cnt = (double*)m.ne_cnt.p;
    g.Bp = Bp;
    g.rows = rows;
    const int64_t gx = max_np / kThreads, gy = std::min<int64_t>(rows + 1, 65535);
    const int64_t gz = std::max<int64_t>(1, std::min<int64_t>(65535, ((int64_t)1 << 22) / (gx * gy)));
    for (int64_t t0 = 0; t0 < T; t0 += gz) {
        g.t0 = t0;
        launch_sourcewise_gather(c, g, dim3((unsigned)gx, (unsigned)gy, (unsigned)std::min(gz, T - t0)));
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        fac_drop_nonempty(m);
        return fail(c, BI_ERR_HIP, "%s (gather): %s", who, hipGetErrorString(e));
    }
    m.ne_off.assign(tab.begin(), tab.begin() + T);
    m.ne_np.assign(tab.begin() + T, tab.begin() + 2 * T);
    m.ne_cnt_off.assign(tab.begin() + 2 * T, tab.end());
    m.ne_max_nbx = (int)std::min<int64_t>(max_np / kTile, kFacBlocks);
    m.ne_bytes = bytes;
    m.ne_ready = true;
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_sourcewise_build_nonempty(bi_ctx* c, int64_t* nnz) {
    int rc = fac_check(c, "bi_sourcewise_build_nonempty", true);
    if (rc) return rc;
    try {
        return sourcewise_build_nonempty(c, nnz);
    } catch (const std::bad_alloc&) {
        fac_drop_nonempty(c->fac);
        return fail(c, BI_ERR_NOMEM, "bi_sourcewise_build_nonempty: out of host memory");
    }
}

int bi_sourcewise_drop_nonempty(bi_ctx* c) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    fac_drop_nonempty(c->fac);
    return BI_OK;
}

}  // extern "C"
