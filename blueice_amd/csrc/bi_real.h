// bi_real.h -- real-valued datasets: the store (bi_set_real_counts, bi_set_asimov_counts, bi_real_count_sets,
// bi_download_real_counts), bi_eval_real and bi_fit_batched_real (host half; the kernels are k_morph_real and k_real_expect,
// bi_k_real.h).
//
// The store c->real_counts [real_T][Bp] lies beside the context's ordinary data and is read by nothing else: every existing
// data path keeps scipy's poisson.logpmf semantics (a count that is no integer is -inf).  bi_eval_real is the descriptor batch
// of bi_items.h over the dense rows -- one work item per live point, the coefficient columns of PointDerivs::first_order, the
// chunked launch and k_finish -- with the half-deviance in slot 0 instead of the log-likelihood and the store's rows for the
// counts.  The points are screened by the box and rate tests alone; the dataset test of the other evaluations is against the
// integer store (c->T, which may be empty here: expected results need no observed data) and is replaced by a check of the
// whole dataset column.  bi_set_asimov_counts writes the value rows of bi_items.h, bi_expected_counts's, through k_real_expect.
#pragma once

namespace {

// a new store takes the place of the old one only when it is complete: on any refusal the previous one stays usable
void real_store_swap(bi_ctx* c, DevBuf& fresh, int64_t T) {
    dev_free(c->real_counts);
    c->real_counts = fresh;
    c->real_T = T;
    fresh = DevBuf{};
}

int real_eval(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* half_deviance,
              double* grad, int32_t* status) {
    const int S = c->S, d = c->d;
    const bool values_only = grad == nullptr;
    const int W = values_only ? 1 : 1 + d + S;
    if (W > kMaxG) return fail(c, BI_ERR_INVALID, "bi_eval_real: 1 + d + S = %d exceeds %d gradient columns (value-only calls have no such limit)", W, kMaxG);
    for (int64_t p = 0; dataset && p < P; ++p)
        if (dataset[p] < 0 || dataset[p] >= c->real_T)
            return fail(c, BI_ERR_INVALID, "bi_eval_real: dataset[%lld] = %lld outside the %lld real-valued sets", (long long)p,
                        (long long)dataset[p], (long long)c->real_T);
    HIP_TRY(c, hipSetDevice(c->device));
    const int G = W == 1 ? 1 : W <= 4 ? 4 : W <= 8 ? 8 : 16;
    const int de = (int)c->eff_axes.size();
    const int NS = (1 << de) * S;
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();

    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, nullptr, status, [&](int64_t p) {
        half_deviance[p] = inf;
        for (int j = 0; !values_only && j < d + S; ++j) grad[p * (d + S) + j] = qnan;
    }, false);
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;

    std::vector<int> axis_col((size_t)de);
    for (int i = 0; i < de; ++i) axis_col[(size_t)i] = 1 + c->eff_axes[(size_t)i];
    // the dense route, its counts offsets dataset * Bp into the real-valued store; no slot constants
    const ItemRoute rt = ItemRoute::dense(c);
    ItemBatch batch(c, live, G, G, W);
    batch.fill(rt, z, rate_scale, dataset, false, 1024, 0,
               [&](const PointDerivs& pd, double* col, int corner, int s) {
                   if (values_only) col[0] = pd.value(corner, s);      // (k_real_expect's a_k)
                   else pd.first_order(col, corner, s, axis_col.data(), 1 + d + s);
               },
               [](const PointDerivs&, double*, int64_t) {});
    int rc;
    if ((rc = batch.upload(c))) return rc;
    HessArgs a{};
    a.ps = rt.ps;
    a.counts = (const double*)c->real_counts.p;
    a.B = c->B;
    a.NS = NS;
    a.D = W - 1;
    a.chunks = (int)c->tile_chunks;
    const bool nt = rt.nt(n_items);
    rc = batch.run(c, a, "bi_eval_real", [&](const HessArgs& b, dim3 grid) {
        const int e = launch_morph_real(c, G, b, grid, nt);
        return e ? fail(c, e, "bi_eval_real: no kernel variant for %d columns", G) : BI_OK;
    });
    if (rc) return rc;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = live[(size_t)i];
        const double* h = batch.out(i);
        half_deviance[p] = h[0];
        for (int j = 0; !values_only && j < d + S; ++j) grad[p * (d + S) + j] = std::isfinite(h[0]) ? h[1 + j] : qnan;
    }
    return BI_OK;
}

// what every entry point of the real-valued store refuses, and `need_store`: the evaluations
int real_check(bi_ctx* c, const char* what, bool need_store) {
    int rc = gof_check(c, what, false);
    if (rc) return rc;
    if (need_store && (c->real_T < 1 || !c->real_counts.p))
        return fail(c, BI_ERR_STATE, "%s: no real-valued dataset is resident (bi_set_real_counts / bi_set_asimov_counts first)", what);
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_set_real_counts(bi_ctx* c, int64_t T, const double* counts) {
    int rc = real_check(c, "bi_set_real_counts", false);
    if (rc) return rc;
    if (T < 0) return fail(c, BI_ERR_INVALID, "bi_set_real_counts: T = %lld", (long long)T);
    HIP_TRY(c, hipSetDevice(c->device));
    if (T == 0 || !counts) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        dev_free(c->real_counts);
        c->real_T = 0;
        return BI_OK;
    }
    const int64_t B = c->B, Bp = c->Bp;
    for (int64_t t = 0; t < T; ++t)
        for (int64_t b = 0; b < B; ++b) {
            const double n = counts[t * B + b];
            if (!(n >= 0.0 && n < std::numeric_limits<double>::infinity()))
                return fail(c, BI_ERR_INVALID, "bi_set_real_counts: dataset %lld, bin %lld holds %g: every count must be finite and >= 0",
                            (long long)t, (long long)b, n);
        }
    std::vector<double> padded((size_t)(T * Bp), 0.0);
    for (int64_t t = 0; t < T; ++t) std::copy(counts + t * B, counts + (t + 1) * B, padded.begin() + (size_t)(t * Bp));
    DevBuf fresh;
    if ((rc = dev_alloc(c, fresh, padded.size() * sizeof(double)))) return rc;
    hipError_t e = hipMemcpyAsync(fresh.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        dev_free(fresh);
        return fail(c, BI_ERR_HIP, "bi_set_real_counts: %s", hipGetErrorString(e));
    }
    real_store_swap(c, fresh, T);
    return BI_OK;
}

int bi_set_asimov_counts(bi_ctx* c, int64_t H, const double* z, const double* rate_scale) {
    int rc = real_check(c, "bi_set_asimov_counts", false);
    if (rc) return rc;
    if (H < 1) return fail(c, BI_ERR_INVALID, "bi_set_asimov_counts: H = %lld (at least one truth)", (long long)H);
    if (c->d > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    const int S = c->S;
    const int de = (int)c->eff_axes.size();
    const int NS = (1 << de) * S;
    const int64_t Bp = c->Bp;
    HIP_TRY(c, hipSetDevice(c->device));
    // every truth is screened before anything changes
    std::vector<int32_t> bits((size_t)H);
    screen_points(c, H, z, rate_scale, nullptr, bits.data(), [](int64_t) {}, false);
    for (int64_t h = 0; h < H; ++h)
        if (bits[(size_t)h])
            return fail(c, BI_ERR_INVALID, "bi_set_asimov_counts: truth %lld %s", (long long)h,
                        bits[(size_t)h] == BI_ST_OUT_OF_BOUNDS ? "lies outside the anchor box" : "has unphysical rates");
    std::vector<int64_t> rowoff((size_t)H * NS);
    std::vector<double> coef((size_t)H * NS);
    PointDerivs pd(c, false);
    fill_value_rows(pd, nullptr, H, z, rate_scale, rowoff.data(), coef.data());
    ScratchBuf fresh, d_rowoff, d_coef, d_bad;
    std::vector<int64_t> bad((size_t)H, 0);
    if ((rc = dev_alloc(c, fresh, (size_t)(H * Bp) * sizeof(double))) || (rc = dev_upload(c, d_rowoff, rowoff)) ||
        (rc = dev_upload(c, d_coef, coef)) || (rc = dev_upload(c, d_bad, bad)))
        return rc;
    hipError_t e = hipMemsetAsync(fresh.p, 0, (size_t)(H * Bp) * sizeof(double), c->stream);
    c->last_point_pieces = 0;
    for (int64_t h0 = 0; h0 < H && e == hipSuccess; h0 += 65535) {
        const int64_t nh = std::min<int64_t>(65535, H - h0);
        RealExpectArgs a{};
        a.ps = (const double*)c->ps.p;
        a.rowoff = (const int64_t*)d_rowoff.p + h0 * NS;
        a.coef = (const double*)d_coef.p + h0 * NS;
        a.out = (double*)fresh.p + h0 * Bp;
        a.bad = (int64_t*)d_bad.p + h0;
        a.B = c->B; a.Bp = Bp; a.NS = NS;
        launch_real_expect(c, a, nh);
        ++c->last_point_pieces;
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), d_bad.p, (size_t)H * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_set_asimov_counts: %s", hipGetErrorString(e));
    for (int64_t h = 0; h < H; ++h)
        if (bad[(size_t)h])
            return fail(c, BI_ERR_INVALID, "bi_set_asimov_counts: the expectation of truth %lld is negative or nan in bin %lld: no dataset",
                        (long long)h, (long long)(bad[(size_t)h] - 1));
    DevBuf keep = fresh;                 // (out of the scope's hands: the store owns it from here)
    static_cast<DevBuf&>(fresh) = DevBuf{};
    real_store_swap(c, keep, H);
    return BI_OK;
}

int64_t bi_real_count_sets(bi_ctx* c) { return c ? c->real_T : 0; }

int bi_download_real_counts(bi_ctx* c, int64_t t, double* out) {
    int rc = real_check(c, "bi_download_real_counts", true);
    if (rc) return rc;
    if (t < 0 || t >= c->real_T || !out)
        return fail(c, BI_ERR_INVALID, "bi_download_real_counts: dataset %lld outside [0,%lld) or out is NULL", (long long)t, (long long)c->real_T);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, (const double*)c->real_counts.p + t * c->Bp, (size_t)c->B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

int bi_eval_real(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* half_deviance,
                 double* grad, int32_t* status) {
    int rc = real_check(c, "bi_eval_real", true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !half_deviance)) return fail(c, BI_ERR_INVALID, "bad P / output pointer");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    return real_eval(c, P, z, rate_scale, dataset, half_deviance, grad, status);
}

int bi_fit_batched_real(bi_ctx* c, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                        const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                        const double* hi, const int32_t* n_kinks, const double* kinks, double gtol, int max_iter,
                        const double* prior_mean, const double* prior_sigma, const double* prior_const, double* x_out,
                        double* f_out, int32_t* flags_out, int64_t* counters) {
    int rc = real_check(c, "bi_fit_batched_real", true);
    if (rc) return rc;
    return fit_batched(c, "bi_fit_batched_real", kFitReal, P, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks, gtol, max_iter,
                       prior_mean, prior_sigma, prior_const, x_out, f_out, flags_out, counters);
}

}  // extern "C"
