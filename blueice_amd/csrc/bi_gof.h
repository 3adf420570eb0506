// bi_gof.h -- bi_eval_gof and bi_expected_counts (host half; the kernels are k_morph_gof and k_morph_expect, bi_k_gof.h).
//
// bi_eval_gof: one work item per live point with ONE coefficient column over the NS = 2^d_eff * S corner rows of its cell,
// a_k = w_c(z) mus_s(z) rs_s, and two result slots, the half-deviance and Pearson's chi2 of the item's dataset.  An empty bin
// adds mu_b to both sums, so in the non-empty-bin form the empty bins of dataset t enter through the row totals over them:
//     both slots += sum_k a_k Tz[t, row_k]
// (as the slot constant -that: k_finish subtracts).  The route, the screen, the descriptor batch and its chunked launch and
// finish are bi_items.h's; the two identical slot constants are written here.  bi_expected_counts: the value rows and the
// download of bi_items.h around k_morph_expect.
#pragma once

namespace {

// the refusals the two entry points share; need_data: bi_eval_gof
int gof_check(bi_ctx* c, const char* what, bool need_data) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->bb_source >= 0)
        return fail(c, BI_ERR_INVALID, "%s: not defined with Beeston-Barlow (bb_source = %d): the expectation depends on the data", what, c->bb_source);
    if (c->unbinned) return fail(c, BI_ERR_INVALID, "%s: the context holds an unbinned likelihood, which has no bins", what);
    return need_data ? check_ready(c, true) : BI_OK;
}

}  // namespace

extern "C" {

int bi_eval_gof(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* half_deviance,
                double* pearson, int32_t* status) {
    int rc = gof_check(c, "bi_eval_gof", true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!half_deviance || !pearson))) return fail(c, BI_ERR_INVALID, "bad P / output pointers");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    const int S = c->S;
    const int de = (int)c->eff_axes.size();
    const int NS = (1 << de) * S, NSL = 2;
    HIP_TRY(c, hipSetDevice(c->device));
    const ItemRoute rt(c);
    if (!rt.has_counts()) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();

    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, dataset, status, [&](int64_t p) {
        half_deviance[p] = pearson[p] = inf;
    });
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;
    // one column a_k; on the compacted route slot 0 gathers the expectation summed over the dataset's empty bins, which both
    // statistics are reduced by the negative of
    ItemBatch batch(c, live, 1, NSL, NSL);
    batch.fill(rt, z, rate_scale, dataset, false, 1024, 1,
               [](const PointDerivs& pd, double* col, int corner, int s) { col[0] = pd.value(corner, s); },
               [](const PointDerivs&, double* lg, int64_t) { lg[0] = lg[1] = -lg[0]; });
    if ((rc = batch.upload(c))) return rc;
    HessArgs a{};
    a.ps = rt.ps;
    a.counts = rt.counts;
    a.B = c->B;
    a.NS = NS;
    a.chunks = (int)c->tile_chunks;
    const bool nt = rt.nt(n_items);
    rc = batch.run(c, a, "bi_eval_gof", [&](const HessArgs& b, dim3 grid) {
        launch_morph_gof(c, b, grid, nt);
        return BI_OK;
    });
    if (rc) return rc;
    // ll = -inf at the point (an event where nothing is expected, a count that is no count) is +inf in BOTH statistics, ll = nan
    // (a negative or nan expectation) nan in both: whichever of the two sums met the bin first decides for the pair
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = live[(size_t)i];
        double hd = batch.out(i)[0], pe = batch.out(i)[1];
        if (hd != hd || pe != pe) hd = pe = qnan;
        else if (hd == inf || pe == inf) hd = pe = inf;
        half_deviance[p] = hd;
        pearson[p] = pe;
    }
    return BI_OK;
}

int bi_expected_counts(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int per_source, double* out) {
    int rc = gof_check(c, "bi_expected_counts", false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !out)) return fail(c, BI_ERR_INVALID, "bad P / output pointer");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    const int S = c->S;
    const int de = (int)c->eff_axes.size();
    const int NS = (1 << de) * S, R = per_source ? S : 1;
    const int64_t B = c->B, per_item = (int64_t)R * B;
    HIP_TRY(c, hipSetDevice(c->device));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    // the screen of every evaluation less its dataset test (the expectation does not depend on the data); no status is reported
    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, nullptr, nullptr,
                                                    [&](int64_t p) { std::fill(out + p * per_item, out + (p + 1) * per_item, qnan); }, false);
    const int64_t n_items = (int64_t)live.size();
    c->last_point_pieces = 0;
    if (n_items == 0) return BI_OK;
    // chunks of points: the device buffer holds at most ~64 MB of expectations (and a launch at most 65 535 items)
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_items, 32768), ((int64_t)1 << 23) / per_item));
    ScratchBuf d_out;
    if ((rc = dev_alloc(c, d_out, (size_t)(chunk * per_item) * sizeof(double)))) return rc;
    std::vector<int64_t> rowoff((size_t)chunk * NS);
    std::vector<double> coef((size_t)chunk * NS);
    PointDerivs pd(c, false);
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        fill_value_rows(pd, &live[(size_t)i0], ni, z, rate_scale, rowoff.data(), coef.data());
        PackedUpload pu;
        if ((rc = packed_upload(c, {{rowoff.data(), (size_t)ni * NS * sizeof(int64_t)}, {coef.data(), (size_t)ni * NS * sizeof(double)}}, 0, pu)))
            return rc;
        ExpectArgs a{};
        a.ps = (const double*)c->ps.p;
        a.rowoff = pu.dev<int64_t>(0);
        a.coef = pu.dev<double>(1);
        a.out = (double*)d_out.p;
        a.B = B; a.NS = NS; a.S = S; a.R = R;
        launch_morph_expect(c, a, ni);
        ++c->last_point_pieces;
        // (the staging block of packed_upload and d_out are reused by the next chunk: the download synchronises)
        const hipError_t e = download_live_runs(c, &live[(size_t)i0], ni, (const double*)d_out.p, per_item, out, hipGetLastError());
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_expected_counts: %s", hipGetErrorString(e));
    }
    return BI_OK;
}

}  // extern "C"
