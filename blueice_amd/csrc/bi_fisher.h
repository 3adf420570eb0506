// bi_fisher.h -- bi_eval_fisher: the expected (Fisher) information of P points (host half; the kernel is k_morph_fisher,
// bi_k_fisher.h).
//
//     I_qr(theta) = sum_b d_q mu_b d_r mu_b / mu_b        theta = (z of the effective axes, rate_scale)
//
// needs no data and no store: one work item per live point over the dense rows, the G = 1 + D padded first-order columns of
// PointDerivs::first_order (column 0 -> mu_b, 1 + i -> d mu_b / d z of effective axis i, 1 + d_eff + s -> d mu_b / d rate_scale_s:
// the first-order columns of bi_eval_hess), no slot constants.  The screen (box and rate tests alone), the descriptor batch,
// its chunked launch and k_finish are bi_items.h's.  An item's result slots: [0] sum_b mu_b, [1 + q] the number of bins with
// mu_b == 0 and d_q mu_b != 0, [G + q (q + 1) / 2 + r] the Gram pair q >= r; the host scatters the pairs symmetrically into the
// full parameter order (rows and columns of single-anchor axes stay zero).
#pragma once

namespace {

// (G, DM) kernel variant of D first-order columns: G the smallest of {4, 8, 16} that holds 1 + D, DM the smallest that holds
// D; false when 1 + D exceeds kMaxG
bool fisher_variant(int D, int& G, int& DM) {
    if (D < 0 || 1 + D > kMaxG) return false;
    G = 1 + D <= 4 ? 4 : 1 + D <= 8 ? 8 : 16;
    DM = D <= 4 ? 4 : D <= 8 ? 8 : 16;
    return true;
}

}  // namespace

extern "C" {

int bi_fisher_variant(int D, int* G, int* DM) {
    int g = 0, dm = 0;
    if (!fisher_variant(D, g, dm)) return BI_ERR_INVALID;
    if (G) *G = g;
    if (DM) *DM = dm;
    return BI_OK;
}

int bi_eval_fisher(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, double* info, double* total, int64_t* unbounded,
                   int32_t* status) {
    int rc = gof_check(c, "bi_eval_fisher", false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !info)) return fail(c, BI_ERR_INVALID, "bad P / output pointer");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    const int S = c->S, d = c->d;
    const int de = (int)c->eff_axes.size();
    const int D = de + S, F = d + S;
    int G, DM;
    if (!fisher_variant(D, G, DM))
        return fail(c, BI_ERR_INVALID, "bi_eval_fisher: 1 + d_eff + S = %d exceeds %d coefficient columns", 1 + D, kMaxG);
    const int NSL = G + DM * (DM + 1) / 2;             // result slots per item: the columns, then the Gram pairs
    const int NS = (1 << de) * S;
    HIP_TRY(c, hipSetDevice(c->device));
    const double qnan = std::numeric_limits<double>::quiet_NaN();

    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, nullptr, status, [&](int64_t p) {
        for (int j = 0; j < F * F; ++j) info[p * F * F + j] = qnan;
        if (total) total[p] = qnan;
        for (int j = 0; unbounded && j < F; ++j) unbounded[p * F + j] = 0;
    }, false);
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;

    // full parameter index of first-order index q
    std::vector<int> full((size_t)D), axis_col((size_t)de);
    for (int q = 0; q < D; ++q) full[(size_t)q] = q < de ? c->eff_axes[(size_t)q] : d + (q - de);
    for (int i = 0; i < de; ++i) axis_col[(size_t)i] = 1 + i;
    // the dense route (no counts are read: the items' counts offsets are never used); no slot constants
    const ItemRoute rt = ItemRoute::dense(c);
    ItemBatch batch(c, live, G, NSL, NSL);
    batch.fill(rt, z, rate_scale, nullptr, false, 1024, 0,
               [&](const PointDerivs& pd, double* col, int corner, int s) { pd.first_order(col, corner, s, axis_col.data(), 1 + de + s); },
               [](const PointDerivs&, double*, int64_t) {});
    if ((rc = batch.upload(c))) return rc;
    HessArgs a{};
    a.ps = rt.ps;
    a.counts = nullptr;
    a.B = c->B;
    a.NS = NS;
    a.D = D;
    a.chunks = (int)c->tile_chunks;
    const bool nt = rt.nt(n_items);
    rc = batch.run(c, a, "bi_eval_fisher", [&](const HessArgs& b, dim3 grid) {
        const int e = launch_morph_fisher(c, G, DM, b, grid, nt);
        return e ? fail(c, e, "bi_eval_fisher: no kernel variant for G = %d, DM = %d", G, DM) : BI_OK;
    });
    if (rc) return rc;
    parallel_for(n_items, 2048, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = live[(size_t)i];
            const double* h = batch.out(i);
            double* ip = info + p * F * F;
            if (total) total[p] = h[0];
            for (int q = 0; unbounded && q < D; ++q) unbounded[p * F + full[(size_t)q]] = (int64_t)h[1 + q];
            if (!(h[0] >= 0.0)) continue;        // a negative or nan expectation in some bin: the matrix stays nan
            for (int j = 0; j < F * F; ++j) ip[j] = 0.0;
            for (int q = 0; q < D; ++q)
                for (int r = 0; r <= q; ++r) {
                    const double v = h[G + q * (q + 1) / 2 + r];
                    ip[full[(size_t)q] * F + full[(size_t)r]] = v;
                    ip[full[(size_t)r] * F + full[(size_t)q]] = v;
                }
        }
    });
    return BI_OK;
}

}  // extern "C"
