// bi_hess.h -- bi_eval_hess: value, gradient and Hessian of P points (host half; the kernel is k_morph_hess, bi_k_hess.h).
//
// Per point the host builds Gc = 1 + D + D2 coefficient columns over the NS = 2^d_eff * S corner rows of its cell, row k =
// (corner c, source s), a_k = w_c(z) mus_s(z) rs_s:
//   column 0                 a_k                                                            -> mu_b
//   first order, axis i      d_i w_c mus_s rs_s + w_c d_i mus_s rs_s                          -> d_i mu_b
//   first order, rate t      delta_st w_c mus_s                                               -> d_t mu_b
//   second order, axes i<=j  rs_s (d_ij w_c mus_s + d_i w_c d_j mus_s + d_j w_c d_i mus_s + w_c d_ij mus_s)
//                            (d_ii w_c = d_ii mus_s = 0: the diagonal keeps 2 d_i w_c d_i mus_s)
//   second order, axis i, t  delta_st (d_i w_c mus_s + w_c d_i mus_s)
// (rate-rate second derivatives are 0).  The kernel reduces every column with the per-bin weight n / mu - 1 (1 / lambda for
// events) and the Gram sums of the first-order columns with n / mu^2 (1 / lambda^2); the empty bins of the non-empty-bin
// form enter through the row totals over them (h_Tz), the unbinned -sum_s mu_s through the slot constants.  The route, the
// screen, the corner derivatives and first-order columns, the descriptor batch and its chunked launch and finish are
// bi_items.h's; the second-order columns and their unbinned constants are written here.
#pragma once

namespace {

// (G, DM) kernel variant of Gc coefficient columns and D first-order columns; false when none fits without scratch
bool hess_variant(int Gc, int D, int& G, int& DM) {
    G = Gc <= 8 ? 8 : Gc <= 16 ? 16 : Gc <= 32 ? 32 : 64;
    DM = D <= 4 ? 4 : D <= 8 ? 8 : 16;
    if (G >= 32 && DM < 8) DM = 8;
    if (Gc > 64 || D > 16) return false;
    return !(G == 64 && DM == 16);          // (200 accumulators per thread: spills)
}

}  // namespace

extern "C" {

int bi_eval_hess(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                 double* grad, double* hess, int32_t* status) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!ll || !grad || !hess))) return fail(c, BI_ERR_INVALID, "bad P / output pointers");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    if (c->bb_source >= 0) return fail(c, BI_ERR_INVALID, "bi_eval_hess: no analytic Hessian with Beeston-Barlow (bb_source = %d)", c->bb_source);
    const bool unb = c->unbinned;
    if (unb && !c->ps_finite)
        return fail(c, BI_ERR_INVALID, "bi_eval_hess: the unbinned pdfs are not all finite (the nan-skipping sum over sources has no analytic Hessian)");
    const int S = c->S, d = c->d;
    const int de = (int)c->eff_axes.size();
    const int D = de + S, NZZ = de * (de + 1) / 2, Gc = 1 + D + NZZ + de * S, NP = D * (D + 1) / 2;
    int G, DM;
    if (!hess_variant(Gc, D, G, DM))
        return fail(c, BI_ERR_INVALID, "bi_eval_hess: %d coefficient columns and %d first-order parameters have no kernel variant "
                                       "(at most 64 columns and 16 first-order parameters, not both above 32 and 8)", Gc, D);
    const int NSL = G + DM * (DM + 1) / 2;             // result slots per item: the columns, then the Gram pairs
    const int F = d + S;
    HIP_TRY(c, hipSetDevice(c->device));
    const int NS = (1 << de) * S;
    const ItemRoute rt(c);
    if (!rt.has_counts()) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    const double ninf = -std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();

    // column of the second-order pair (q >= r, first-order indices: < de an effective axis, else rate q - de); -1 = zero
    std::vector<int> col2((size_t)NP, -1);
    {
        int k = 1 + D;
        for (int ii = 0; ii < de; ++ii)
            for (int jj = ii; jj < de; ++jj) col2[(size_t)(jj * (jj + 1) / 2 + ii)] = k++;
        for (int ii = 0; ii < de; ++ii)
            for (int t = 0; t < S; ++t) col2[(size_t)((de + t) * (de + t + 1) / 2 + ii)] = k++;
    }
    // full parameter index of first-order index q
    std::vector<int> full((size_t)D);
    for (int q = 0; q < D; ++q) full[(size_t)q] = q < de ? c->eff_axes[(size_t)q] : d + (q - de);

    // the points that are evaluated at all, then the descriptors of the live ones (as bi_eval_grad)
    if (dataset && multi_set(c)) return refuse_sets(c, "bi_eval_hess with a dataset column");
    if (unb) dataset = nullptr;        // (one dataset; several event sets: set 0, whose columns B counts)
    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = ninf;
        for (int j = 0; j < F; ++j) grad[p * F + j] = qnan;
        for (int j = 0; j < F * F; ++j) hess[p * F * F + j] = qnan;
    });
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;
    std::vector<int> axis_col((size_t)de);
    for (int ii = 0; ii < de; ++ii) axis_col[(size_t)ii] = 1 + ii;
    ItemBatch batch(c, live, G, NSL, NSL);
    batch.fill(rt, z, rate_scale, dataset, true, 512, Gc,
               [&](const PointDerivs& pd, double* col, int corner, int s) {
                   const double* rs = pd.rs;
                   const double w = pd.g.w[(size_t)corner];
                   const double* dwc = &pd.dw[(size_t)corner * de];
                   pd.first_order(col, corner, s, axis_col.data(), 1 + de + s);
                   int q = 1 + D;
                   for (int ii = 0; ii < de; ++ii)
                       for (int jj = ii; jj < de; ++jj, ++q) {
                           const double a_i = pd.dmus[(size_t)ii * S + s], a_j = pd.dmus[(size_t)jj * S + s];
                           if (ii == jj) col[q] = rs[s] * (2.0 * dwc[ii] * a_i);
                           else {
                               const int pz = jj * (jj + 1) / 2 + ii;
                               col[q] = rs[s] * (pd.d2w[(size_t)corner * NZZ + pz] * pd.mus[(size_t)s] + dwc[ii] * a_j + dwc[jj] * a_i +
                                                 w * pd.d2mus[(size_t)pz * S + s]);
                           }
                       }
                   for (int ii = 0; ii < de; ++ii, q += S) col[q + s] = dwc[ii] * pd.mus[(size_t)s] + w * pd.dmus[(size_t)ii * S + s];
               },
               [&](const PointDerivs& pd, double* lg, int64_t ds) {
                   if (!unb) {
                       lg[0] += c->h_lgsum[(size_t)ds];
                       return;
                   }
                   pd.first_order_unbinned(lg, axis_col.data(), 1 + de);
                   int q = 1 + D;                   // the second-order columns' constants
                   for (int ii = 0; ii < de; ++ii) {
                       for (int jj = ii; jj < de; ++jj, ++q)
                           if (jj != ii)
                               for (int s = 0; s < S; ++s) lg[q] += pd.d2mus[(size_t)(jj * (jj + 1) / 2 + ii) * S + s] * pd.rs[s];
                   }
                   for (int ii = 0; ii < de; ++ii)
                       for (int t = 0; t < S; ++t, ++q) lg[q] = pd.dmus[(size_t)ii * S + t];
               });
    if ((rc = batch.upload(c))) return rc;
    HessArgs a{};
    a.ps = rt.ps;
    a.counts = rt.counts;
    a.B = c->B;
    a.outlier = c->outlier;
    a.NS = NS;
    a.D = D;
    a.chunks = (int)c->tile_chunks;
    const bool nt = !unb && rt.nt(n_items);
    rc = batch.run(c, a, "bi_eval_hess", [&](const HessArgs& b, dim3 grid) {
        const int e = launch_morph_hess(c, G, DM, b, grid, nt);
        return e ? fail(c, e, "bi_eval_hess: no kernel variant for G = %d, DM = %d", G, DM) : BI_OK;
    });
    if (rc) return rc;
    parallel_for(n_items, 2048, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = live[(size_t)i];
            const double* h = batch.out(i);
            ll[p] = h[0];
            double* gp = grad + p * F;
            double* hp = hess + p * F * F;
            for (int j = 0; j < F; ++j) gp[j] = 0.0;
            for (int q = 0; q < D; ++q) gp[full[(size_t)q]] = h[1 + q];
            if (!std::isfinite(ll[p])) {        // H stays nan; the gradient is bi_eval_grad's (nan for the unbinned likelihood)
                if (unb) for (int j = 0; j < F; ++j) gp[j] = qnan;
                continue;
            }
            for (int j = 0; j < F * F; ++j) hp[j] = 0.0;
            for (int q = 0; q < D; ++q) {
                for (int r = 0; r <= q; ++r) {
                    const int pr = q * (q + 1) / 2 + r;
                    const double v = h[G + pr] + (col2[(size_t)pr] >= 0 ? h[col2[(size_t)pr]] : 0.0);
                    hp[full[(size_t)q] * F + full[(size_t)r]] = v;
                    hp[full[(size_t)r] * F + full[(size_t)q]] = v;
                }
            }
        }
    });
    return BI_OK;
}

}  // extern "C"
