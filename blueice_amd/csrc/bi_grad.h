// bi_grad.h -- the entry points of bi_eval_grad: per point the coefficient COLUMNS of the value and of its derivatives over the
// corner rows of its cell, one work item per point (k_morph_reduce<G, false, NT, 1 / 3>; with Beeston-Barlow
// k_morph_bbgrad, bi_k_bbgrad.h), k_finish for the sums.  The route, the screen, the descriptor batch and its chunked
// launch-and-finish tail are bi_items.h's; what is the gradient's own: the first-order columns, the unbinned slot constants,
// launches over mixed event sets, and the Beeston-Barlow layout of three row groups (eval_grad_bb).  Large batches of plain
// binned likelihoods are planned on the device instead (bi_planning_device.h, bi_grad_mfma.h).
#pragma once

namespace {

// Beeston-Barlow models: per point the U rows (corner, source != bb) carry all 1 + d + S columns, the P and A rows (corner,
// bb source / Monte-Carlo counts) the value and shape columns; aux holds {p_cal, N} and its derivatives
int eval_grad_bb(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                 double* grad, int32_t* status) {
    const int S = c->S, d = c->d, bbs = c->bb_source;
    const int W = 1 + d + S;
    const int de = (int)c->eff_axes.size();
    const int nc = 1 << de;
    const int n0 = nc * (S - 1), n1 = nc, n2 = nc, NS = n0 + n1 + n2;
    const int G = W <= 8 ? 8 : 16;
    const int DZ = 1 + d <= 4 ? 4 : 8;
    if (W > 16 || 1 + d > 8) return fail(c, BI_ERR_INVALID, "Beeston-Barlow gradient needs 1 + d + S <= 16 and d <= 7 (got d = %d, S = %d)", d, S);
    if (!c->dense_counts) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    const double ninf = -std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const int64_t coef_per_item = (int64_t)n0 * G + (int64_t)(n1 + n2) * DZ;

    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = ninf;
        for (int j = 0; j < d + S; ++j) grad[p * (d + S) + j] = qnan;
    });
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;
    std::vector<int> axis_col((size_t)de);
    for (int i = 0; i < de; ++i) axis_col[(size_t)i] = 1 + c->eff_axes[(size_t)i];
    std::vector<int64_t> rowoff((size_t)n_items * NS), cnt_off((size_t)n_items), perm((size_t)n_items * G, -1);
    std::vector<double> coef((size_t)(n_items * coef_per_item), 0.0), aux((size_t)n_items * G * 2, 0.0), slot_lg((size_t)n_items * G, 0.0);
    std::vector<PointGeom> geoms((size_t)n_items);
    std::vector<double> rates_all((size_t)n_items * S);
    parallel_for(n_items, 1024, [&](int64_t lo, int64_t hi) {
        PointDerivs pd(c, false);
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = live[(size_t)i];
            pd.at(z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr);
            const PointGeom& g = pd.g;
            const size_t ro = (size_t)i * NS, po = (size_t)i * G;
            double* cU = &coef[(size_t)(i * coef_per_item)];
            double* cP = cU + (size_t)n0 * G;
            double* cA = cP + (size_t)n1 * DZ;
            int k = 0;
            double Ntot = 0.0;
            for (int corner = 0; corner < nc; ++corner) {
                const int64_t a = g.cell_anchor + pd.corner_off[(size_t)corner];
                const double w = g.w[(size_t)corner];
                for (int s = 0; s < S; ++s) {
                    if (s == bbs) continue;
                    rowoff[ro + k] = (a * S + s) * c->Bp;
                    pd.first_order(cU + (size_t)k * G, corner, s, axis_col.data(), 1 + d + s);
                    ++k;
                }
                rowoff[ro + n0 + corner] = (a * S + bbs) * c->Bp;
                rowoff[ro + n0 + n1 + corner] = a * c->Bp;
                cP[(size_t)corner * DZ] = w;
                cA[(size_t)corner * DZ] = w;
                for (int ii = 0; ii < de; ++ii) {
                    cP[(size_t)corner * DZ + axis_col[(size_t)ii]] = pd.dw[(size_t)corner * de + ii];
                    cA[(size_t)corner * DZ + axis_col[(size_t)ii]] = pd.dw[(size_t)corner * de + ii];
                }
                const double term = c->h_nm_tot[(size_t)a] * w;
                Ntot = Ntot + term;
            }
            double* ax_ = &aux[po * 2];
            ax_[0] = 0.0; ax_[1] = Ntot;                      // p_cal is set below, once N is final (bb_exact)
            for (int ii = 0; ii < de; ++ii) {
                double dN = 0.0;
                for (int corner = 0; corner < nc; ++corner)
                    dN += pd.dw[(size_t)corner * de + ii] * c->h_nm_tot[(size_t)(g.cell_anchor + pd.corner_off[(size_t)corner])];
                ax_[axis_col[(size_t)ii] * 2 + 0] = pd.dmus[(size_t)ii * S + bbs] * pd.rs[bbs];
                ax_[axis_col[(size_t)ii] * 2 + 1] = dN;
            }
            ax_[(1 + d + bbs) * 2 + 0] = pd.mus[(size_t)bbs];
            const int64_t ds = dataset ? dataset[p] : 0;
            slot_lg[po] = c->h_lgsum[(size_t)ds];
            for (int q = 0; q < W; ++q) perm[po + q] = i * W + q;
            cnt_off[(size_t)i] = ds * c->Bp;
            geoms[(size_t)i] = g;
            std::copy(pd.r.begin(), pd.r.end(), rates_all.begin() + (size_t)i * S);
        }
    });
    int rc;
    // N(z) in numpy's summation order where some bin can have U_b == 0 (as the value path does: same bits, same asserts)
    for (int64_t i = 0; i < n_items; ++i) {
        double& N = aux[(size_t)i * G * 2 + 1];
        const double* r = &rates_all[(size_t)i * S];
        if (c->bb_exact == 1 || (c->bb_exact == 2 && bb_zero_u_possible(c, geoms[(size_t)i], r))) {
            if ((rc = bb_exact_total(c, geoms[(size_t)i], &N))) return rc;
        }
        aux[(size_t)i * G * 2 + 0] = r[bbs] / N;
    }
    PackedUpload pu;
    const size_t out_bytes = (size_t)n_items * W * sizeof(double) + (size_t)n_items * W * sizeof(int32_t) + 64;
    if ((rc = packed_upload(c, {{rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)},
                                {aux.data(), aux.size() * sizeof(double)}, {cnt_off.data(), cnt_off.size() * sizeof(int64_t)},
                                {perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}},
                            out_bytes, pu)))
        return rc;
    double* h_out = (double*)pu.host_out();
    int32_t* h_st = (int32_t*)((char*)pu.host_out() + ((size_t)n_items * W * sizeof(double) + 63) / 64 * 64);
    memset(h_st, 0, (size_t)n_items * W * sizeof(int32_t));
    LaunchArgs a{};
    a.ps = (const double*)c->ps.p;
    a.nm = (const double*)c->nm.p;
    a.counts = (const double*)c->counts.p;
    a.B = c->B; a.Bp = c->Bp; a.n0 = n0; a.n1 = n1; a.n2 = n2; a.n_tiles = n_tiles_of(c); a.chunks = (int)c->tile_chunks;
    const bool huge = (int64_t)sizeof(double) * (NS + 1) * c->Bp > ((int64_t)1 << 30);
    const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && (n_items == 1 || huge));
    rc = run_item_chunks(c, n_items, a.n_tiles, G, pu.dev<int64_t>(4), pu.dev<double>(5), h_out, h_st, "bi_eval_grad (Beeston-Barlow)",
                         [&](int64_t i0, dim3 grid, double* partial, unsigned* pflags) {
                             LaunchArgs b = a;
                             b.rowoff = pu.dev<int64_t>(0) + i0 * NS;
                             b.coef = pu.dev<double>(1) + i0 * coef_per_item;
                             b.aux = pu.dev<double>(2) + i0 * G * 2;
                             b.item_cnt = pu.dev<int64_t>(3) + i0;
                             b.partial = partial;
                             b.pflags = pflags;
                             const int e = launch_morph_bbgrad(c, G, DZ, b, grid, nt);
                             return e ? fail(c, e, "no Beeston-Barlow gradient kernel for %d x %d columns", G, DZ) : BI_OK;
                         });
    if (rc) return rc;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = live[(size_t)i];
        ll[p] = h_out[(size_t)i * W];
        for (int j = 0; j < d + S; ++j) grad[p * (d + S) + j] = h_out[(size_t)i * W + 1 + j];
        if (status) status[p] |= h_st[(size_t)i * W];          // the Beeston-Barlow assertion bits ride on the value slot
    }
    return BI_OK;
}

}  // namespace

static int eval_grad_points(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                            double* grad, int32_t* status, bool values_only);

extern "C" {

int bi_eval_grad(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                 double* grad, int32_t* status) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!ll || !grad))) return fail(c, BI_ERR_INVALID, "bad P / output pointers");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    if (c->bb_source >= 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        return eval_grad_bb(c, P, z, rate_scale, dataset, ll, grad, status);
    }
    return eval_grad_points(c, P, z, rate_scale, dataset, ll, grad, status, false);
}

}  // extern "C"

// bi_eval_grad without Beeston-Barlow.  values_only (unbinned contexts with several event sets, bi_eval): the same
// descriptors with the value column alone, grad is not touched.
static int eval_grad_points(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                            double* grad, int32_t* status, bool values_only) {
    int rc;
    const int S = c->S, d = c->d;
    const int W = values_only ? 1 : 1 + d + S;
    if (W > kMaxG) return fail(c, BI_ERR_INVALID, "1 + d + S = %d exceeds %d gradient columns", W, kMaxG);
    HIP_TRY(c, hipSetDevice(c->device));
    const int G = values_only ? 1 : std::max(2, pick_class(W, kMaxG));
    const int de = (int)c->eff_axes.size();
    const int NS = (1 << de) * S;
    // (one dataset -- or several event sets side by side on the event axis: set t is columns [first_t, first_t + N_t))
    const ItemRoute rt(c, true);
    const bool unb = rt.unb, sparse = rt.compact, sets = rt.by_set;
    if (!rt.has_counts()) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    const double ninf = -std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();

    // large batches: the descriptors are built on the device (k_grad_fill), one work item per point
    if (!unb && c->device_plan_min > 0 && P >= c->device_plan_min && de <= 6 && P <= ((int64_t)1 << 26)) {
        // one dataset, up to 32 streams: grouped by grid cell, two matrix products per 16-bin block (k_grad_mfma)
        if (c->grad_mfma && P >= c->grad_mfma_min && c->scan_mfma && c->ps_finite && NS <= 32 && (!dataset || c->T == 1))
            return eval_grad_mfma(c, P, z, rate_scale, dataset, sparse, ll, grad, status);
        return eval_grad_device(c, P, z, rate_scale, dataset, sparse, G, ll, grad, status);
    }

    // Host half, per point and independent: the screen decides which points are evaluated at all (the reference's early
    // exits), then the descriptor arrays of the live ones are filled.  Both run on a few host threads for large batches --
    // the batched profile-fit engine calls this once per optimiser iteration over every running problem, and at ~1.7 us
    // per point single-threaded the host half was six times the kernels' time at 10^5 points.
    if (unb && !sets) dataset = nullptr;
    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = ninf;
        for (int j = 0; !values_only && j < d + S; ++j) grad[p * (d + S) + j] = qnan;
    });
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;
    std::vector<int> axis_col((size_t)de);
    for (int i = 0; i < de; ++i) axis_col[(size_t)i] = 1 + c->eff_axes[(size_t)i];
    ItemBatch batch(c, live, G, G, W);
    batch.fill(rt, z, rate_scale, dataset, false, 1024, W,
               [&](const PointDerivs& pd, double* col, int corner, int s) {
                   if (values_only) col[0] = pd.value(corner, s);
                   else pd.first_order(col, corner, s, axis_col.data(), 1 + d + s);
               },
               [&](const PointDerivs& pd, double* lg, int64_t ds) {
                   if (unb && values_only) lg[0] = pd.rate_sum();
                   else if (unb) pd.first_order_unbinned(lg, axis_col.data(), 1 + d);
                   else lg[0] += c->h_lgsum[(size_t)ds];
               });
    // several event sets: a launch whose items all name ONE set runs the ordinary kernels over that set's columns (the row
    // offsets start at first_t, B = N_t; their counts offset is 0 as for every unbinned launch); items with different sets
    // take k_morph_sets, every item over its own segment, whose length travels in the counts-offset array
    bool mixed = false;
    int64_t ds0 = 0;
    if (sets) {
        ds0 = dataset ? dataset[live[0]] : 0;
        for (int64_t i = 1; dataset && i < n_items && !mixed; ++i) mixed = dataset[live[(size_t)i]] != ds0;
        if (mixed) ++c->n_set_launches;
        else std::fill(batch.cnt_off.begin(), batch.cnt_off.end(), (int64_t)0);
    }
    if ((rc = batch.upload(c))) return rc;
    LaunchArgs a{};
    a.ps = rt.ps;
    a.counts = rt.counts;
    a.B = c->B; a.Bp = c->Bp; a.n0 = NS; a.n_tiles = batch.max_tiles; a.chunks = (int)c->tile_chunks;
    a.outlier = c->outlier;
    a.nan_S = (unb && !c->ps_finite) ? c->S : 0;
    if (sets) a.B = c->set_n[(size_t)ds0];             // (one set: its events; several: k_morph_sets takes every item's own)
    const bool nt = rt.nt(n_items);
    rc = batch.run(c, a, "bi_eval_grad", [&](const LaunchArgs& b, dim3 grid) {
        if (mixed) launch_morph_sets(c, G, b, grid);
        else if (values_only) launch_morph_g(c, 1, b, grid, false, nt);
        else launch_morph_grad(c, G, b, grid, nt);
        if (!mixed) { c->last_morph_nbx = grid.x; c->last_morph_items = grid.y; c->last_morph_fused = 0; }
        return BI_OK;
    });
    if (rc) return rc;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = live[(size_t)i];
        const double* h = batch.out(i);
        ll[p] = h[0];
        for (int j = 0; !values_only && j < d + S; ++j) grad[p * (d + S) + j] = (unb && !std::isfinite(ll[p])) ? qnan : h[1 + j];
    }
    return BI_OK;
}
