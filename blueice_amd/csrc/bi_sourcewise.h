// bi_sourcewise.h -- what a source-wise model needs beyond value, gradient and curvature (host half; the kernels are
// k_sourcewise_expect and k_sourcewise_gof, bi_k_sourcewise.h, and the dense toy kernel below): bi_sourcewise_expected_counts,
// bi_eval_sourcewise_gof, bi_sourcewise_generate_toys, bi_sourcewise_download_counts.  Screen, descriptors and upload are
// FacBatch's of order 0 (bi_factored.h); the goodness-of-fit sums go through FacBatch::run with two slots, the expectation is
// written by launches over sub-batches of points into a bounded device buffer.
//
// The toys are stream A of bi_generate_toys (one draw per bin, poisson_draw_pair of bi_k_misc.h) with mu_b the expectation
// k_sourcewise_expect writes, and they replace the store's counts as T dense datasets: the store has no non-empty-bin form, and
// every kernel that reads it streams dense rows.
#pragma once

namespace {

constexpr int64_t kSwLaunchItems = 32768;                  // items (points, truths, toys) per launch: gridDim.y stays below 65 536
constexpr int64_t kSwExpectDoubles = (int64_t)1 << 23;     // expectations in flight per launch of bi_sourcewise_expected_counts (64 MiB)

// One thread per (toy, bin pair): blockIdx.y = toy of the launch, toy0 + blockIdx.y its number in the seed's ensemble, truth[.] the
// row of mu / p0 ([H][Bp]) it is drawn at (uniform over a block: a scalar load).  Both counts leave in one 16-byte store; the pad
// bins behind B are written as 0 (poisson_draw_pair gives 0 for a bin >= B).  128 VGPRs, and the 388 bytes of stack that the
// out-of-line poisson_ptrs brings to k_toy_count as well (profiles/sourcewise_toys_kernel_resources.txt); nothing spills.
__global__ __launch_bounds__(kThreads) void k_sourcewise_toys(const double* __restrict__ mu, const double* __restrict__ p0, int64_t Bp,
                                                              int64_t B, uint64_t seed, int64_t toy0, const int32_t* __restrict__ truth,
                                                              double* __restrict__ counts) {
    const int64_t b = 2 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (b >= Bp) return;
    const int64_t t = blockIdx.y;
    const int64_t h = truth[t];
    double n0, n1;
    poisson_draw_pair(mu + h * Bp, p0 + h * Bp, B, seed, toy0 + t, b, n0, n1);
    *reinterpret_cast<double2*>(counts + t * Bp + b) = make_double2(n0, n1);
}

// the expectation rows of items [i0, i0 + ni) of a filled and uploaded batch -> d_out [ni][R][Bp] (device)
int sourcewise_expect_rows(bi_ctx* c, const FacBatch& b, int64_t i0, int64_t ni, bool per_source, double* d_out, bool nt, const char* who) {
    SourcewiseExpectArgs a{};
    a.f = b.args();
    b.point_at(a.f, i0);
    a.out = d_out;
    a.Bp = b.m.Bp;
    a.R = per_source ? b.S : 1;
    const int e = launch_sourcewise_expect(c, b.SC, b.EM, per_source, a, ni, nt);
    return e ? fail(c, e, "%s: no kernel variant for %d source slots with %d own axes", who, b.SC, b.EM) : BI_OK;
}

}  // namespace

extern "C" {

int bi_sourcewise_expected_counts(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int per_source, double* out) {
    const char* who = "bi_sourcewise_expected_counts";
    int rc = fac_check(c, who, false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !out)) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointer", who);
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (P == 0) return BI_OK;
    FacBatch b(c, 0, false);
    const int64_t B = b.m.B, Bp = b.m.Bp, R = per_source ? b.S : 1, per_item = R * Bp;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    // the screen of every evaluation less its dataset test (the expectation does not depend on the data); no status is reported
    b.screen(P, z, rate_scale, nullptr, nullptr, [&](int64_t p) { std::fill(out + p * R * B, out + (p + 1) * R * B, qnan); });
    const int64_t n_items = b.n_items;
    if (n_items == 0) return BI_OK;
    b.fill(z, rate_scale, nullptr);
    if ((rc = b.upload({}, 0))) return rc;
    const int64_t chunk = std::max<int64_t>(1, std::min(std::min(n_items, kSwLaunchItems), kSwExpectDoubles / per_item));
    ScratchBuf d_out;
    if ((rc = dev_alloc(c, d_out, (size_t)(chunk * per_item) * sizeof(double)))) return rc;
    const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1);
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        if ((rc = sourcewise_expect_rows(c, b, i0, ni, per_source != 0, (double*)d_out.p, nt, who))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        ++c->last_point_pieces;
        // rows of stride Bp -> the caller's rows of stride B; runs of consecutive live points are consecutive in `out` too.  The
        // copies synchronise: d_out is reused by the next sub-batch
        hipError_t e = hipGetLastError();
        for (int64_t i = i0; i < i0 + ni && e == hipSuccess;) {
            int64_t j = i + 1;
            while (j < i0 + ni && b.live[(size_t)j] == b.live[(size_t)j - 1] + 1) ++j;
            e = hipMemcpy2DAsync(out + b.live[(size_t)i] * R * B, (size_t)B * sizeof(double), (const double*)d_out.p + (i - i0) * per_item,
                                 (size_t)Bp * sizeof(double), (size_t)B * sizeof(double), (size_t)((j - i) * R), hipMemcpyDeviceToHost, c->stream);
            i = j;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        else (void)hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return BI_OK;
}

int bi_eval_sourcewise_gof(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* half_deviance,
                           double* pearson, int32_t* status) {
    const char* who = "bi_eval_sourcewise_gof";
    int rc = fac_check(c, who, true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!half_deviance || !pearson))) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointers", who);
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (P == 0) return BI_OK;
    constexpr int NSL = 2;
    FacBatch b(c, 0);
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    b.screen(P, z, rate_scale, dataset, status, [&](int64_t p) { half_deviance[p] = pearson[p] = inf; });
    const int64_t n_items = b.n_items;
    if (n_items == 0) return BI_OK;
    b.fill(z, rate_scale, dataset);
    const size_t n = (size_t)n_items;
    std::vector<int64_t> perm(n * NSL);
    const std::vector<double> slot_lg(n * NSL, 0.0);        // nothing is subtracted from either sum
    for (size_t q = 0; q < perm.size(); ++q) perm[q] = (int64_t)q;
    if ((rc = b.upload({{perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}}, n * NSL))) return rc;
    const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1);
    rc = b.run(NSL, b.pu.dev<int64_t>(b.first_extra), b.pu.dev<double>(b.first_extra + 1), who, [&](const FactoredArgs& a, dim3 grid) {
        const int e = launch_sourcewise_gof(c, b.SC, b.EM, a, grid, nt);
        return e ? fail(c, e, "%s: no kernel variant for %d source slots with %d own axes", who, b.SC, b.EM) : BI_OK;
    });
    if (rc) return rc;
    // ll = -inf at the point (an event where nothing is expected, a count that is no count) is +inf in BOTH statistics, ll = nan
    // nan in both: whichever of the two sums met the bin first decides for the pair (as bi_eval_gof)
    const double* res = b.out();
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = b.live[(size_t)i];
        double hd = res[(size_t)i * NSL], pe = res[(size_t)i * NSL + 1];
        if (hd != hd || pe != pe) hd = pe = qnan;
        else if (hd == inf || pe == inf) hd = pe = inf;
        half_deviance[p] = hd;
        pearson[p] = pe;
    }
    return BI_OK;
}

int bi_sourcewise_generate_toys(bi_ctx* c, int64_t H, const double* z, const double* rate_scale, const int64_t* n_toys, uint64_t seed) {
    const char* who = "bi_sourcewise_generate_toys";
    int rc = fac_check(c, who, false);
    if (rc) return rc;
    if (H == 0) return BI_OK;
    if (H < 0 || !n_toys) return fail(c, BI_ERR_INVALID, "%s: need H >= 0 truth points and their numbers of toys", who);
    int64_t T = 0;
    for (int64_t h = 0; h < H; ++h) {
        if (n_toys[h] < 0) return fail(c, BI_ERR_INVALID, "%s: n_toys[%lld] = %lld is negative", who, (long long)h, (long long)n_toys[h]);
        if (n_toys[h] > INT32_MAX - T) return fail(c, BI_ERR_INVALID, "%s: a call draws fewer than 2^31 toys", who);
        T += n_toys[h];
    }
    if (T < 1) return fail(c, BI_ERR_INVALID, "%s: need T >= 1 toys", who);
    if (c->fac.d > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    HIP_TRY(c, hipSetDevice(c->device));
    bi_ctx::Factored& m = c->fac;
    const int64_t B = m.B, Bp = m.Bp;
    // every truth is validated before the store changes
    FacBatch b(c, 0, false);
    std::vector<int32_t> st((size_t)H, 0);
    b.screen(H, z, rate_scale, nullptr, st.data(), [](int64_t) {});
    for (int64_t h = 0; h < H; ++h) {
        if (st[(size_t)h] & BI_ST_OUT_OF_BOUNDS) return fail(c, BI_ERR_INVALID, "%s (truth %lld): point is outside the anchor box", who, (long long)h);
        if (st[(size_t)h]) return fail(c, BI_ERR_INVALID, "%s (truth %lld): a rate is outside [0, inf)", who, (long long)h);
    }
    b.fill(z, rate_scale, nullptr);
    if ((rc = b.upload({}, 0))) return rc;
    DevBuf fresh;                                    // the old counts stay until everything has succeeded
    if ((rc = dev_alloc(c, fresh, (size_t)T * (size_t)Bp * sizeof(double)))) return rc;
    std::vector<int32_t> truth((size_t)T);
    for (int64_t h = 0, t = 0; h < H; ++h)
        for (int64_t j = 0; j < n_toys[h]; ++j, ++t) truth[(size_t)t] = (int32_t)h;
    ScratchBuf d_mu, d_p0, d_truth;
    std::vector<double> lgsum;
    if ((rc = dev_alloc(c, d_mu, (size_t)(H * Bp) * sizeof(double))) || (rc = dev_alloc(c, d_p0, (size_t)(H * Bp) * sizeof(double))) ||
        (rc = dev_upload(c, d_truth, truth))) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(fresh);
        return rc;
    }
    for (int64_t h0 = 0; h0 < H && !rc; h0 += kSwLaunchItems, ++c->last_point_pieces)
        rc = sourcewise_expect_rows(c, b, h0, std::min(kSwLaunchItems, H - h0), false, (double*)d_mu.p + h0 * Bp, false, who);
    hipError_t e = hipSuccess;
    if (!rc) {
        {
            EventScope ev(c);
            hipLaunchKernelGGL(k_exp_neg, dim3((unsigned)((H * Bp + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_mu.p, H * Bp,
                               (double*)d_p0.p);
        }
        EventScope ev(c);
        for (int64_t t0 = 0; t0 < T; t0 += kSwLaunchItems) {
            const int64_t nt = std::min(kSwLaunchItems, T - t0);
            hipLaunchKernelGGL(k_sourcewise_toys, dim3((unsigned)(Bp / kTile), (unsigned)nt), dim3(kThreads), 0, c->stream, (const double*)d_mu.p,
                               (const double*)d_p0.p, Bp, B, seed, c->toy_offset + t0, (const int32_t*)d_truth.p + t0, (double*)fresh.p + t0 * Bp);
        }
        e = hipGetLastError();
    }
    // sum_b lgamma(n + 1) per toy, as bi_factored_set_counts computes it (synchronises the stream on every path)
    if (!rc) rc = fac_counts_lgsum(c, who, (const double*)fresh.p, T, e, lgsum);
    else (void)hipStreamSynchronize(c->stream);
    if (rc) {
        dev_free(fresh);
        return rc;
    }
    dev_free(m.counts);
    m.counts = fresh;
    m.T = T;
    m.h_lgsum.swap(lgsum);
    fac_drop_nonempty(m);           // (lists of the previous counts)
    return fac_sync_lgsum(c, who);
}

int bi_sourcewise_download_counts(bi_ctx* c, int64_t t, double* out) {
    const char* who = "bi_sourcewise_download_counts";
    int rc = fac_check(c, who, true);
    if (rc) return rc;
    if (t < 0 || t >= c->fac.T || !out)
        return fail(c, BI_ERR_INVALID, "%s: dataset %lld outside [0,%lld) or out is NULL", who, (long long)t, (long long)c->fac.T);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, (const double*)c->fac.counts.p + t * c->fac.Bp, (size_t)c->fac.B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

}  // extern "C"
