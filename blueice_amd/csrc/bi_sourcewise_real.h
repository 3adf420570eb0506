// bi_sourcewise_real.h -- real-valued datasets of a source-wise model: the store (bi_sourcewise_set_real_counts,
// bi_sourcewise_set_asimov_counts, bi_sourcewise_real_count_sets, bi_sourcewise_download_real_counts), bi_eval_sourcewise_real and
// bi_fit_batched_sourcewise_real (host half; the kernel is k_sourcewise_real, bi_k_sourcewise_real.h).
//
// The store c->fac.real_counts [real_T][Bp] lies beside the model's ordinary counts and is read by nothing else: every other data
// path of the source-wise model keeps scipy's poisson.logpmf semantics (a count that is no integer is -inf).  None of the calls
// here needs ordinary counts.  bi_eval_sourcewise_real is bi_eval_factored's host path -- FacBatch (bi_factored.h): screen, fill
// on host threads, one packed upload, run_item_chunks + k_finish, the gradient by FacBatch::gradient's chain rule -- with the
// half-deviance in slot 0, nothing subtracted from it, and the store's rows for the counts.  The points are screened by the box
// and rate tests alone; the dataset test of the other evaluations is against the ordinary counts (which may be absent here) and
// is replaced by a check of the whole dataset column, as in bi_eval_real.  An Asimov dataset is the row k_sourcewise_expect
// writes for its truth (sourcewise_expect_rows, bi_sourcewise.h), straight into the new store.
#pragma once

namespace {

// a new store takes the place of the old one only when it is complete: on any refusal the previous one stays usable
void sw_real_store_swap(bi_ctx* c, DevBuf& fresh, int64_t T) {
    dev_free(c->fac.real_counts);
    c->fac.real_counts = fresh;
    c->fac.real_T = T;
    fresh = DevBuf{};
}

// what every entry point of the store refuses, and `need_store`: the evaluations
int sw_real_check(bi_ctx* c, const char* who, bool need_store) {
    int rc = fac_check(c, who, false);
    if (rc) return rc;
    if (need_store && (c->fac.real_T < 1 || !c->fac.real_counts.p))
        return fail(c, BI_ERR_STATE, "%s: no real-valued dataset is resident (bi_sourcewise_set_real_counts / bi_sourcewise_set_asimov_counts first)",
                    who);
    return BI_OK;
}

int sourcewise_real_eval(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* half_deviance,
                         double* grad, int32_t* status) {
    const char* who = "bi_eval_sourcewise_real";
    for (int64_t p = 0; dataset && p < P; ++p)
        if (dataset[p] < 0 || dataset[p] >= c->fac.real_T)
            return fail(c, BI_ERR_INVALID, "%s: dataset[%lld] = %lld outside the %lld real-valued sets", who, (long long)p, (long long)dataset[p],
                        (long long)c->fac.real_T);
    const bool want_grad = grad != nullptr;
    FacBatch b(c, want_grad ? 1 : 0, false);        // (no dataset test in the screen: the column was checked above)
    const int d = b.d, S = b.S, NSL = factored_slots(b.SC, b.EM, want_grad);
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));

    b.screen(P, z, rate_scale, nullptr, status, [&](int64_t p) {
        half_deviance[p] = inf;
        for (int j = 0; want_grad && j < d + S; ++j) grad[p * (d + S) + j] = qnan;
    });
    const int64_t n_items = b.n_items;
    if (n_items == 0) return BI_OK;
    b.fill(z, rate_scale, nullptr);
    const size_t n = (size_t)n_items;
    // the items' counts rows: dataset * Bp into the real-valued store
    for (size_t i = 0; i < n; ++i) b.cnt_off[i] = (dataset ? dataset[b.live[i]] : 0) * b.m.Bp;
    std::vector<int64_t> perm(n * NSL);
    const std::vector<double> slot_lg(n * NSL, 0.0);        // nothing is subtracted from any sum
    for (size_t q = 0; q < perm.size(); ++q) perm[q] = (int64_t)q;
    int rc = b.upload({{perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}}, n * NSL);
    if (rc) return rc;
    const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1);
    const double* store = (const double*)c->fac.real_counts.p;
    rc = b.run(NSL, b.pu.dev<int64_t>(b.first_extra), b.pu.dev<double>(b.first_extra + 1), who, [&](const FactoredArgs& a, dim3 grid) {
        FactoredArgs r = a;
        r.counts = store;
        const int e = launch_sourcewise_real(c, b.SC, b.EM, want_grad, r, grid, nt);
        return e ? fail(c, e, "%s: no kernel variant for %d source slots with %d own axes", who, b.SC, b.EM) : BI_OK;
    });
    if (rc) return rc;

    const double* out = b.out();
    std::vector<double> gz((size_t)std::max(d, 1));
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = b.live[(size_t)i];
        const double* h = out + (size_t)i * NSL;
        half_deviance[p] = h[0];
        if (!want_grad || !std::isfinite(h[0])) continue;       // (the gradient stays nan)
        b.gradient(i, h, rate_scale, grad + p * (d + S), gz);
    }
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_sourcewise_set_real_counts(bi_ctx* c, int64_t T, const double* counts) {
    const char* who = "bi_sourcewise_set_real_counts";
    int rc = sw_real_check(c, who, false);
    if (rc) return rc;
    if (T < 0) return fail(c, BI_ERR_INVALID, "%s: T = %lld", who, (long long)T);
    HIP_TRY(c, hipSetDevice(c->device));
    bi_ctx::Factored& m = c->fac;
    if (T == 0 || !counts) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        dev_free(m.real_counts);
        m.real_T = 0;
        return BI_OK;
    }
    const int64_t B = m.B, Bp = m.Bp;
    for (int64_t t = 0; t < T; ++t)
        for (int64_t b = 0; b < B; ++b) {
            const double n = counts[t * B + b];
            if (!(n >= 0.0 && n < std::numeric_limits<double>::infinity()))
                return fail(c, BI_ERR_INVALID, "%s: dataset %lld, bin %lld holds %g: every count must be finite and >= 0", who, (long long)t,
                            (long long)b, n);
        }
    std::vector<double> padded((size_t)(T * Bp), 0.0);
    for (int64_t t = 0; t < T; ++t) std::copy(counts + t * B, counts + (t + 1) * B, padded.begin() + (size_t)(t * Bp));
    DevBuf fresh;
    if ((rc = dev_alloc(c, fresh, padded.size() * sizeof(double)))) return rc;
    hipError_t e = hipMemcpyAsync(fresh.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        dev_free(fresh);
        return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    sw_real_store_swap(c, fresh, T);
    return BI_OK;
}

int bi_sourcewise_set_asimov_counts(bi_ctx* c, int64_t H, const double* z, const double* rate_scale) {
    const char* who = "bi_sourcewise_set_asimov_counts";
    int rc = sw_real_check(c, who, false);
    if (rc) return rc;
    if (H < 1) return fail(c, BI_ERR_INVALID, "%s: H = %lld (at least one truth)", who, (long long)H);
    if (c->fac.d > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t B = c->fac.B, Bp = c->fac.Bp;
    // every truth is screened before anything changes
    FacBatch b(c, 0, false);
    std::vector<int32_t> st((size_t)H, 0);
    b.screen(H, z, rate_scale, nullptr, st.data(), [](int64_t) {});
    for (int64_t h = 0; h < H; ++h) {
        if (st[(size_t)h] & BI_ST_OUT_OF_BOUNDS) return fail(c, BI_ERR_INVALID, "%s (truth %lld): point is outside the anchor box", who, (long long)h);
        if (st[(size_t)h]) return fail(c, BI_ERR_INVALID, "%s (truth %lld): a rate is outside [0, inf)", who, (long long)h);
    }
    b.fill(z, rate_scale, nullptr);
    if ((rc = b.upload({}, 0))) return rc;
    DevBuf fresh;                                    // the old store stays until everything has succeeded
    if ((rc = dev_alloc(c, fresh, (size_t)H * (size_t)Bp * sizeof(double)))) return rc;
    // k_sourcewise_expect writes whole rows of stride Bp, the pad bins behind B included (zeros: the templates are zero there)
    for (int64_t h0 = 0; h0 < H && !rc; h0 += kSwLaunchItems, ++c->last_point_pieces)
        rc = sourcewise_expect_rows(c, b, h0, std::min(kSwLaunchItems, H - h0), false, (double*)fresh.p + h0 * Bp, false, who);
    hipError_t e = rc ? hipSuccess : hipGetLastError();
    // an expectation that is not finite is no dataset (the rates and templates are >= 0: it cannot be negative); the rows come to
    // the host in bounded pieces
    const int64_t piece = std::max<int64_t>(1, kSwExpectDoubles / Bp);
    std::vector<double> rows((size_t)(std::min(piece, H) * Bp));
    int64_t bad_h = -1, bad_b = -1;
    for (int64_t h0 = 0; h0 < H && !rc && e == hipSuccess && bad_h < 0; h0 += piece) {
        const int64_t nh = std::min(piece, H - h0);
        e = hipMemcpyAsync(rows.data(), (const double*)fresh.p + h0 * Bp, (size_t)(nh * Bp) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        for (int64_t h = 0; h < nh && e == hipSuccess && bad_h < 0; ++h)
            for (int64_t k = 0; k < B; ++k) {
                const double mu = rows[(size_t)(h * Bp + k)];
                if (!(mu >= 0.0 && mu < std::numeric_limits<double>::infinity())) { bad_h = h0 + h; bad_b = k; break; }
            }
    }
    if (rc || e != hipSuccess || bad_h >= 0) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(fresh);
        if (rc) return rc;
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        return fail(c, BI_ERR_INVALID, "%s (truth %lld): the expectation is not finite in bin %lld: no dataset", who, (long long)bad_h, (long long)bad_b);
    }
    sw_real_store_swap(c, fresh, H);
    return BI_OK;
}

int64_t bi_sourcewise_real_count_sets(bi_ctx* c) { return c ? c->fac.real_T : 0; }

int bi_sourcewise_download_real_counts(bi_ctx* c, int64_t t, double* out) {
    const char* who = "bi_sourcewise_download_real_counts";
    int rc = sw_real_check(c, who, true);
    if (rc) return rc;
    if (t < 0 || t >= c->fac.real_T || !out)
        return fail(c, BI_ERR_INVALID, "%s: dataset %lld outside [0,%lld) or out is NULL", who, (long long)t, (long long)c->fac.real_T);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, (const double*)c->fac.real_counts.p + t * c->fac.Bp, (size_t)c->fac.B * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

int bi_eval_sourcewise_real(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* half_deviance,
                            double* grad, int32_t* status) {
    const char* who = "bi_eval_sourcewise_real";
    int rc = sw_real_check(c, who, true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !half_deviance)) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointer", who);
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (P == 0) return BI_OK;
    return sourcewise_real_eval(c, P, z, rate_scale, dataset, half_deviance, grad, status);
}

int bi_fit_batched_sourcewise_real(bi_ctx* c, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                                   const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                                   const double* hi, const int32_t* n_kinks, const double* kinks, double gtol, int max_iter,
                                   const double* prior_mean, const double* prior_sigma, const double* prior_const, double* x_out,
                                   double* f_out, int32_t* flags_out, int64_t* counters) {
    int rc = sw_real_check(c, "bi_fit_batched_sourcewise_real", true);
    if (rc) return rc;
    return fit_batched(c, "bi_fit_batched_sourcewise_real", kFitSourcewiseReal, P, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi,
                       n_kinks, kinks, gtol, max_iter, prior_mean, prior_sigma, prior_const, x_out, f_out, flags_out, counters);
}

}  // extern "C"
