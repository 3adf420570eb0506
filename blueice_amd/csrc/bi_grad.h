// bi_grad.h -- host half of bi_eval_grad: per point the coefficient COLUMNS of the value and of its derivatives over the
// corner rows of its cell, one work item per point (k_morph_reduce<G, false, NT, 1 / 3>; with Beeston-Barlow
// k_morph_bbgrad, bi_k_bbgrad.h), k_finish for the sums.  The steps shared with bi_eval_hess (bi_hess.h): the screen of the
// points, the corner-weight derivatives, the first-order columns, the chunked launch-and-finish tail.  Large batches of
// plain binned likelihoods are planned on the device instead (bi_planning_device.h, bi_grad_mfma.h).
#pragma once

namespace {

// screen_point over P points on a few host threads, reset(p) first (the caller's defaults for point p's outputs); status
// [P] (nullable) gets every point's bit.  -> the points that pass, in order.
template <class F>
std::vector<int64_t> screen_points(const bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                                   int32_t* status, F reset) {
    std::vector<int32_t> st((size_t)P);
    parallel_for(P, 2048, [&](int64_t lo, int64_t hi) {
        PointGeom g;
        std::vector<double> r((size_t)c->S);
        for (int64_t p = lo; p < hi; ++p) {
            reset(p);
            st[(size_t)p] = screen_point(c, z ? z + p * c->d : nullptr, rate_scale ? rate_scale + p * c->S : nullptr,
                                         dataset ? dataset[p] : 0, g, r.data());
        }
    });
    std::vector<int64_t> live;
    live.reserve((size_t)P);
    for (int64_t p = 0; p < P; ++p) {
        if (status) status[p] = st[(size_t)p];
        if (!st[(size_t)p]) live.push_back(p);
    }
    return live;
}

// One live point's rates and their derivatives over the effective axes i, j (one per host thread, reused point after point):
//   mus [S], r [S]     interpolated rates, r = mus rs
//   dw [nc][de]        d w_c / d z_i = (+-1 / delta_i) prod_{j != i} w^(j)
//   dmus [de][S]       d mus_s / d z_i = sum_c d w_c / d z_i mus_c,s
//   d2w [nc][npz]      (second order only) d2 w_c / d z_i d z_j, both factors differentiated (0 for i = j); pair i <= j at
//                      j (j + 1) / 2 + i
//   d2mus [npz][S]     sum_c d2 w_c / d z_i d z_j mus_c,s
struct PointDerivs {
    const bi_ctx* c;
    int de, nc, S, npz;
    bool second;
    std::vector<int64_t> corner_off;              // [nc] anchor offset of every corner
    PointGeom g;
    const double* rs = nullptr;                   // the point's rate scales (ones when the call has none)
    std::vector<double> ones, mus, r, dw, dmus, d2w, d2mus;

    PointDerivs(const bi_ctx* ctx, bool second_order)
        : c(ctx), de((int)ctx->eff_axes.size()), nc(1 << de), S(ctx->S), npz(de * (de + 1) / 2), second(second_order),
          corner_off((size_t)nc), ones((size_t)S, 1.0), mus((size_t)S), r((size_t)S), dw((size_t)nc * de), dmus((size_t)de * S),
          d2w(second ? (size_t)nc * npz : 0), d2mus(second ? (size_t)npz * S : 0) {
        for (int k = 0; k < nc; ++k) corner_off[(size_t)k] = corner_offset(c, k);
    }

    double mus_at(int corner, int s) const { return c->h_mus[(size_t)((g.cell_anchor + corner_off[(size_t)corner]) * S + s)]; }

    // the point at z (a live one: inside the anchor box) with rate scales rate_scale (nullable)
    void at(const double* z, const double* rate_scale) {
        point_geometry(c, z, g);
        interp_mus(c, g, mus.data());
        rs = rate_scale ? rate_scale : ones.data();
        for (int s = 0; s < S; ++s) r[(size_t)s] = mus[(size_t)s] * rs[s];
        auto factor = [&](int corner, int j, bool diff) {
            const bool up = (corner >> (de - 1 - j)) & 1;
            const int ax = c->eff_axes[(size_t)j];
            if (diff) return (up ? 1.0 : -1.0) * g.inv_delta[ax];
            return up ? g.t[ax] : (1 - g.t[ax]);
        };
        for (int corner = 0; corner < nc; ++corner)
            for (int i = 0; i < de; ++i) {
                double v = factor(corner, i, true);
                for (int j = 0; j < de; ++j)
                    if (j != i) v *= factor(corner, j, false);
                dw[(size_t)corner * de + i] = v;
            }
        for (int i = 0; i < de; ++i)
            for (int s = 0; s < S; ++s) {
                double v = 0.0;
                for (int corner = 0; corner < nc; ++corner) v += dw[(size_t)corner * de + i] * mus_at(corner, s);
                dmus[(size_t)i * S + s] = v;
            }
        if (!second) return;
        for (int corner = 0; corner < nc; ++corner)
            for (int i = 0; i < de; ++i)
                for (int j = i; j < de; ++j) {
                    double v = 0.0;
                    if (j != i) {
                        v = 1.0;
                        for (int k = 0; k < de; ++k) v *= factor(corner, k, k == i || k == j);
                    }
                    d2w[(size_t)corner * npz + (j * (j + 1) / 2 + i)] = v;
                }
        for (int pz = 0; pz < npz; ++pz)
            for (int s = 0; s < S; ++s) {
                double v = 0.0;
                for (int corner = 0; corner < nc; ++corner) v += d2w[(size_t)corner * npz + pz] * mus_at(corner, s);
                d2mus[(size_t)pz * S + s] = v;
            }
    }

    // the first-order columns of descriptor row (corner, s): col[0] = w_c r_s; col[axis_col[i]] = d_i w_c r_s + w_c d_i mus_s rs_s,
    // the total derivative (through the weights and through mus(z)); col[rate_col] = w_c mus_s
    void first_order(double* col, int corner, int s, const int* axis_col, int rate_col) const {
        const double w = g.w[(size_t)corner];
        col[0] = w * r[(size_t)s];
        for (int i = 0; i < de; ++i) col[axis_col[i]] = dw[(size_t)corner * de + i] * r[(size_t)s] + w * dmus[(size_t)i * S + s] * rs[s];
        col[rate_col] = w * mus[(size_t)s];
    }

    // the unbinned likelihood's slot constants of the same columns: -sum_s mu_s and its derivatives (likelihood.py:690), what
    // the kernel's sums over the events are reduced by
    void first_order_unbinned(double* lg, const int* axis_col, int rate_col0) const {
        double rsum = 0.0;
        for (int s = 0; s < S; ++s) rsum += r[(size_t)s];
        lg[0] = rsum;
        for (int i = 0; i < de; ++i) {
            double v = 0.0;
            for (int s = 0; s < S; ++s) v += dmus[(size_t)i * S + s] * rs[s];
            lg[axis_col[i]] = v;
        }
        for (int s = 0; s < S; ++s) lg[rate_col0 + s] = mus[(size_t)s];
    }
};

// The tail of the one-item-per-point paths: n_items work items of nsl result slots, on nbx blocks each (at most max_tiles;
// about four blocks per CU slot in all).  Per chunk of at most 65 535 items (gridDim.y), launch(i0, grid, partial, pflags)
// points its kernel's arguments at items i0 ... and launches it on the grid; the kernel assigns every (item, block, slot)
// of partial / pflags, so the chunks, in order on one stream, share one chunk's buffers.  k_finish then adds the partials up
// into out[perm] - slot_lg (status |= their flag bits when given).  Synchronises the stream.
template <class L>
int run_item_chunks(bi_ctx* c, int64_t n_items, int max_tiles, int nsl, const int64_t* perm, const double* slot_lg, double* out,
                    int32_t* status, const char* what, L launch) {
    const int64_t slots = (int64_t)c->prop.multiProcessorCount * c->blocks_per_cu;
    const int nbx = (int)std::min<int64_t>(max_tiles, n_items == 1 ? slots : std::max<int64_t>(1, (4 * slots + n_items - 1) / n_items));
    const int64_t chunk = 65535, part_items = std::min(chunk, n_items);
    ScratchBuf d_part, d_flag;
    int rc;
    if ((rc = dev_alloc(c, d_part, (size_t)part_items * nbx * nsl * sizeof(double))) ||
        (rc = dev_alloc(c, d_flag, (size_t)part_items * nbx * nsl * sizeof(unsigned)))) return rc;
    hipError_t e = hipSuccess;
    for (int64_t i0 = 0; i0 < n_items && e == hipSuccess; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        if ((rc = launch(i0, dim3((unsigned)nbx, (unsigned)ni), (double*)d_part.p, (unsigned*)d_flag.p))) return rc;
        launch_finish(c, (const double*)d_part.p, (const unsigned*)d_flag.p, nbx, nsl, ni * nsl, perm + i0 * nsl, slot_lg + i0 * nsl,
                      out, status);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return BI_OK;
}

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
    const int nc = 1 << de, NS = nc * S;
    bool any_neg = false;
    for (int q = 0; q < S; ++q) any_neg |= (c->allow_neg[(size_t)q] != 0);
    const bool unb = c->unbinned;       // extended unbinned likelihood: the rows are pdf values at the events, no counts
    const bool sparse = !unb && c->sparse && c->compact_ready && c->ps_nonneg && !any_neg;
    if (!unb && !sparse && !c->dense_counts) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    const int64_t n_rows = c->A * S;
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
    // (one dataset -- or several event sets side by side on the event axis: set t is columns [first_t, first_t + N_t))
    const bool sets = multi_set(c);
    if (unb && !sets) dataset = nullptr;
    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = ninf;
        for (int j = 0; !values_only && j < d + S; ++j) grad[p * (d + S) + j] = qnan;
    });
    const int64_t n_items = (int64_t)live.size();
    if (n_items == 0) return BI_OK;
    std::vector<int> axis_col((size_t)de);
    for (int i = 0; i < de; ++i) axis_col[(size_t)i] = 1 + c->eff_axes[(size_t)i];
    std::vector<int64_t> rowoff((size_t)n_items * NS), cnt_off((size_t)n_items), perm((size_t)n_items * G, -1);
    std::vector<double> coef((size_t)n_items * NS * G, 0.0), slot_lg((size_t)n_items * G, 0.0);
    std::vector<int32_t> tiles((size_t)n_items);
    parallel_for(n_items, 1024, [&](int64_t lo, int64_t hi) {
        PointDerivs pd(c, false);
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = live[(size_t)i];
            const int64_t ds = dataset ? dataset[p] : 0;
            pd.at(z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr);
            const int64_t row_stride = sparse ? c->h_c_np[(size_t)ds] : c->Bp;
            const int64_t row_base = sparse ? c->h_c_off[(size_t)ds] : (sets ? c->set_first[(size_t)ds] : 0);
            const size_t ro = (size_t)i * NS, co = (size_t)i * NS * G, po = (size_t)i * G;
            int k = 0;
            for (int corner = 0; corner < nc; ++corner)
                for (int s = 0; s < S; ++s, ++k) {
                    const int64_t row = (pd.g.cell_anchor + pd.corner_off[(size_t)corner]) * S + s;
                    rowoff[ro + k] = row_base + row * row_stride;
                    double* col = &coef[co + (size_t)k * G];
                    if (values_only) col[0] = pd.g.w[(size_t)corner] * pd.r[(size_t)s];      // (first_order's column 0)
                    else pd.first_order(col, corner, s, axis_col.data(), 1 + d + s);
                    if (sparse) {
                        const double tz = c->h_Tz[(size_t)(ds * n_rows + row)];
                        for (int q = 0; q < W; ++q) slot_lg[po + q] += col[q] * tz;
                    }
                }
            if (unb && values_only) {
                double rsum = 0.0;
                for (int s = 0; s < S; ++s) rsum += pd.r[(size_t)s];
                slot_lg[po] = rsum;
            } else if (unb)
                pd.first_order_unbinned(&slot_lg[po], axis_col.data(), 1 + d);
            else
                slot_lg[po] += c->h_lgsum[(size_t)ds];
            for (int q = 0; q < W; ++q) perm[po + q] = i * W + q;
            // (several event sets: the item's tiles cover its own segment, and k_morph_sets takes the segment's length here)
            cnt_off[(size_t)i] = sets ? c->set_n[(size_t)ds] : unb ? 0 : (sparse ? c->h_cnt_off[(size_t)ds] : ds * c->Bp);
            tiles[(size_t)i] = sets ? (int32_t)std::max<int64_t>(1, (c->set_n[(size_t)ds] + kTile - 1) / kTile) : (int32_t)(row_stride / kTile);
        }
    });
    int max_tiles = 1;
    for (int32_t t : tiles) max_tiles = std::max(max_tiles, (int)t);
    // several event sets: a launch whose items all name ONE set runs the ordinary kernels over that set's columns (the row
    // offsets start at first_t, B = N_t; their counts offset is 0 as for every unbinned launch); items with different sets
    // take k_morph_sets, every item over its own segment, whose length travels in the counts-offset array
    bool mixed = false;
    int64_t ds0 = 0;
    if (sets) {
        ds0 = dataset ? dataset[live[0]] : 0;
        for (int64_t i = 1; dataset && i < n_items && !mixed; ++i) mixed = dataset[live[(size_t)i]] != ds0;
        if (mixed) ++c->n_set_launches;
        else std::fill(cnt_off.begin(), cnt_off.end(), (int64_t)0);
    }
    // descriptors: one packed copy; results: k_finish writes them straight into pinned host memory
    PackedUpload pu;
    if ((rc = packed_upload(c, {{rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)},
                                {cnt_off.data(), cnt_off.size() * sizeof(int64_t)}, {tiles.data(), tiles.size() * sizeof(int32_t)},
                                {perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}},
                            (size_t)n_items * W * sizeof(double), pu)))
        return rc;
    double* h_out = (double*)pu.host_out();
    LaunchArgs a{};
    a.ps = sparse ? (const double*)c->ps_c.p : (const double*)c->ps.p;
    a.counts = sparse ? (const double*)c->cnt_c.p : (const double*)c->counts.p;
    a.B = c->B; a.Bp = c->Bp; a.n0 = NS; a.n_tiles = max_tiles; a.chunks = (int)c->tile_chunks;
    a.outlier = c->outlier;
    a.nan_S = (unb && !c->ps_finite) ? c->S : 0;
    if (unb) a.counts = (const double*)c->ps.p;        // (never read in this mode: any valid device address)
    if (sets) a.B = c->set_n[(size_t)ds0];             // (one set: its events; several: k_morph_sets takes every item's own)
    const bool nt = !sparse && (c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1));
    rc = run_item_chunks(c, n_items, max_tiles, G, pu.dev<int64_t>(4), pu.dev<double>(5), h_out, nullptr, "bi_eval_grad",
                         [&](int64_t i0, dim3 grid, double* partial, unsigned* pflags) {
                             LaunchArgs b = a;
                             b.rowoff = pu.dev<int64_t>(0) + i0 * NS;
                             b.coef = pu.dev<double>(1) + i0 * NS * G;
                             b.item_cnt = pu.dev<int64_t>(2) + i0;
                             b.item_tiles = pu.dev<int32_t>(3) + i0;
                             b.partial = partial;
                             b.pflags = pflags;
                             if (mixed) launch_morph_sets(c, G, b, grid);
                             else if (values_only) launch_morph_g(c, 1, b, grid, false, nt);
                             else launch_morph_grad(c, G, b, grid, nt);
                             if (!mixed) { c->last_morph_nbx = grid.x; c->last_morph_items = grid.y; c->last_morph_fused = 0; }
                             return BI_OK;
                         });
    if (rc) return rc;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = live[(size_t)i];
        ll[p] = h_out[(size_t)i * W];
        for (int j = 0; !values_only && j < d + S; ++j)
            grad[p * (d + S) + j] = (unb && !std::isfinite(ll[p])) ? qnan : h_out[(size_t)i * W + 1 + j];
    }
    return BI_OK;
}
