// bi_gof.h -- bi_eval_gof and bi_expected_counts (host half; the kernels are k_morph_gof and k_morph_expect, bi_k_gof.h).
//
// bi_eval_gof: one work item per live point with ONE coefficient column over the NS = 2^d_eff * S corner rows of its cell,
// a_k = w_c(z) mus_s(z) rs_s, and two result slots, the half-deviance and Pearson's chi2 of the item's dataset.  The route
// (dense rows with or without nontemporal loads, or the compacted non-empty bins) is bi_eval_hess's.  An empty bin adds mu_b
// to both sums, so in the non-empty-bin form the empty bins of dataset t enter through the row totals over them:
//     both slots += sum_k a_k Tz[t, row_k]
// (as the slot constant -that: k_finish subtracts).  The screen, the descriptors' upload, the chunked launch and k_finish are
// the steps bi_eval_grad and bi_eval_hess share (bi_grad.h).
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
    const int S = c->S, d = c->d;
    const int de = (int)c->eff_axes.size();
    const int nc = 1 << de, NS = nc * S, NSL = 2;
    HIP_TRY(c, hipSetDevice(c->device));
    bool any_neg = false;
    for (int q = 0; q < S; ++q) any_neg |= (c->allow_neg[(size_t)q] != 0);
    const bool sparse = c->sparse && c->compact_ready && c->ps_nonneg && !any_neg;
    if (!sparse && !c->dense_counts) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    const int64_t n_rows = c->A * S;
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();

    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, dataset, status, [&](int64_t p) {
        half_deviance[p] = pearson[p] = inf;
    });
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;
    std::vector<int64_t> rowoff((size_t)n_items * NS), cnt_off((size_t)n_items), perm((size_t)n_items * NSL);
    std::vector<double> coef((size_t)n_items * NS), slot_lg((size_t)n_items * NSL, 0.0);
    std::vector<int32_t> tiles((size_t)n_items);
    parallel_for(n_items, 1024, [&](int64_t lo, int64_t hi) {
        PointDerivs pd(c, false);
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = live[(size_t)i];
            const int64_t ds = dataset ? dataset[p] : 0;
            pd.at(z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr);
            const int64_t row_stride = sparse ? c->h_c_np[(size_t)ds] : c->Bp;
            const int64_t row_base = sparse ? c->h_c_off[(size_t)ds] : 0;
            const size_t ro = (size_t)i * NS, po = (size_t)i * NSL;
            double empty = 0.0;                   // the expectation summed over the dataset's empty bins
            int k = 0;
            for (int corner = 0; corner < nc; ++corner)
                for (int s = 0; s < S; ++s, ++k) {
                    const int64_t row = (pd.g.cell_anchor + pd.corner_off[(size_t)corner]) * S + s;
                    rowoff[ro + k] = row_base + row * row_stride;
                    const double a = pd.g.w[(size_t)corner] * pd.r[(size_t)s];
                    coef[ro + k] = a;
                    if (sparse) empty += a * c->h_Tz[(size_t)(ds * n_rows + row)];
                }
            for (int j = 0; j < NSL; ++j) {
                slot_lg[po + j] = -empty;
                perm[po + j] = (int64_t)po + j;
            }
            cnt_off[(size_t)i] = sparse ? c->h_cnt_off[(size_t)ds] : ds * c->Bp;
            tiles[(size_t)i] = (int32_t)(row_stride / kTile);
        }
    });
    int max_tiles = 1;
    for (int32_t t : tiles) max_tiles = std::max(max_tiles, (int)t);
    PackedUpload pu;
    if ((rc = packed_upload(c, {{rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)},
                                {cnt_off.data(), cnt_off.size() * sizeof(int64_t)}, {tiles.data(), tiles.size() * sizeof(int32_t)},
                                {perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}},
                            (size_t)n_items * NSL * sizeof(double), pu)))
        return rc;
    double* h_out = (double*)pu.host_out();
    HessArgs a{};
    a.ps = sparse ? (const double*)c->ps_c.p : (const double*)c->ps.p;
    a.counts = sparse ? (const double*)c->cnt_c.p : (const double*)c->counts.p;
    a.B = c->B;
    a.NS = NS;
    a.chunks = (int)c->tile_chunks;
    const bool nt = !sparse && (c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1));
    rc = run_item_chunks(c, n_items, max_tiles, NSL, pu.dev<int64_t>(4), pu.dev<double>(5), h_out, nullptr, "bi_eval_gof",
                         [&](int64_t i0, dim3 grid, double* partial, unsigned* pflags) {
                             HessArgs b = a;
                             b.rowoff = pu.dev<int64_t>(0) + i0 * NS;
                             b.coef = pu.dev<double>(1) + i0 * NS;
                             b.item_cnt = pu.dev<int64_t>(2) + i0;
                             b.item_tiles = pu.dev<int32_t>(3) + i0;
                             b.partial = partial;
                             b.pflags = pflags;
                             launch_morph_gof(c, b, grid, nt);
                             return BI_OK;
                         });
    if (rc) return rc;
    // ll = -inf at the point (an event where nothing is expected, a count that is no count) is +inf in BOTH statistics, ll = nan
    // (a negative or nan expectation) nan in both: whichever of the two sums met the bin first decides for the pair
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = live[(size_t)i];
        double hd = h_out[(size_t)i * NSL], pe = h_out[(size_t)i * NSL + 1];
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
    const int S = c->S, d = c->d;
    const int de = (int)c->eff_axes.size();
    const int nc = 1 << de, NS = nc * S, R = per_source ? S : 1;
    const int64_t B = c->B, per_item = (int64_t)R * B;
    HIP_TRY(c, hipSetDevice(c->device));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    // the screen of every evaluation (screen_point) less its dataset test: the expectation does not depend on the data
    std::vector<int64_t> live;
    {
        PointGeom g;
        std::vector<double> r((size_t)S);
        for (int64_t p = 0; p < P; ++p) {
            std::fill(out + p * per_item, out + (p + 1) * per_item, qnan);
            if (!point_geometry(c, z ? z + p * d : nullptr, g)) continue;
            interp_mus(c, g, r.data());
            for (int s = 0; rate_scale && s < S; ++s) r[(size_t)s] *= rate_scale[p * S + s];
            if (rates_physical(c, r.data())) live.push_back(p);
        }
    }
    const int64_t n_items = (int64_t)live.size();
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
        for (int64_t i = 0; i < ni; ++i) {
            const int64_t p = live[(size_t)(i0 + i)];
            pd.at(z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr);
            int k = 0;
            for (int corner = 0; corner < nc; ++corner)
                for (int s = 0; s < S; ++s, ++k) {
                    rowoff[(size_t)(i * NS + k)] = ((pd.g.cell_anchor + pd.corner_off[(size_t)corner]) * S + s) * c->Bp;
                    coef[(size_t)(i * NS + k)] = pd.g.w[(size_t)corner] * pd.r[(size_t)s];
                }
        }
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
        hipError_t e = hipGetLastError();
        // runs of consecutive live points are consecutive in `out` too: one copy each
        for (int64_t i = 0; i < ni && e == hipSuccess;) {
            int64_t j = i + 1;
            while (j < ni && live[(size_t)(i0 + j)] == live[(size_t)(i0 + j - 1)] + 1) ++j;
            e = hipMemcpyAsync(out + live[(size_t)(i0 + i)] * per_item, (const double*)d_out.p + i * per_item,
                               (size_t)((j - i) * per_item) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
            i = j;
        }
        // (the staging block of packed_upload and d_out are reused by the next chunk)
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        else (void)hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_expected_counts: %s", hipGetErrorString(e));
    }
    return BI_OK;
}

}  // extern "C"
