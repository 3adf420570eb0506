// bi_factored.h -- source-wise binned models: one anchor grid per source (host half; the kernel is k_morph_factored,
// bi_k_factored.h).  bi_factored_begin / _set_anchor / _end, bi_factored_set_counts, bi_eval_factored, bi_fit_batched_factored.
//
// The grid model of this library is one tensor product of all d shape axes: a point reads S 2^d rows and the tensor holds
// prod n_i anchor models.  Here source s has rows over the e_s axes IT owns only, p_s [n_{O_s[0]}] .. [B] in C order, and a
// point reads sum_s 2^e_s rows; the expectation is mu_b = sum_s r_s tau_s,b with tau_s the multilinear interpolation of source
// s over its own axes and r_s = M_s(z) rs_s.  That is the per-source interpolation of the reference's
// source_wise_interpolation, for binned Poisson likelihoods.
//
// The store (bi_ctx::fac) lies beside the grid model and is read by nothing else: a context that holds only a source-wise
// model has model_ready == false, so every other entry point refuses it with its usual BI_ERR_STATE.
//
// Limits: d <= 32 axes, S <= 8 sources, e_s <= 3 own axes (a source that responds to more belongs on the full grid).  The
// geometry arrays here are sized by those, not by kMaxDim (PointGeom).  Out of scope, refused where they can be asked for:
// sources that may go negative (template entries must be finite and >= 0; rates outside [0, inf) are BI_ST_UNPHYSICAL),
// Beeston-Barlow.  Unbinned data are a second form of the data, the event store of bi_sourcewise_events.h: while it exists
// factored_eval, and through it the native fit, run on it (FacBatch with events = true) and every other source-wise entry point
// refuses (fac_check).  The counts are dense doubles [T][Bp]: the caller's (bi_factored_set_counts) or toys drawn
// on the device (bi_sourcewise_generate_toys, bi_sourcewise.h, which also holds the expectation and goodness-of-fit layers).
// Beside them, when asked for, the non-empty-bin form of the same counts (bi_sourcewise_build_nonempty, bi_sourcewise_nonempty.h:
// per dataset its list of bins with events and a compacted copy of the rows over it), on which factored_eval, and through it the
// native fit, then run (FacBatch with nonempty = true; fac_nonempty_on).
// Coarse views of the expectation and of these counts: bi_sourcewise_coarse.h, with a coarse binning of the store's own
// (bi_ctx::sw_coarse), which bi_factored_begin releases.
//
// bi_eval_factored is the per-item host path of bi_items.h with descriptors of its own (FacBatch, which the curvature calls of
// bi_factored_curv.h share): screen, fill on host threads, one packed upload, run_item_chunks + k_finish.  The blocks per item
// depend on the rows' length alone (not on the batch), so a point's sums are added in the same order whatever batch it is
// evaluated in.  The loops over staged points that make their work items on the device instead (k_sourcewise_plan over the device
// copy of the geometry, fac_upload_geometry / fac_sync_lgsum below): bi_sourcewise_plan.h.
#pragma once

namespace {

constexpr int kFacBlocks = 1024;                       // blocks per item at most: one per tile for rows up to 512 K bins
constexpr int64_t kFacPartialDoubles = (int64_t)1 << 23;   // partial sums in flight per run_item_chunks call (64 MiB)

struct FacGeom {
    int k[kFacMaxDim];
    double t[kFacMaxDim], inv_delta[kFacMaxDim];
};

// the box test of all d axes (owned or not), then cell and fraction per axis: find_cell's convention (bi_geometry.h)
bool fac_geometry(const bi_ctx::Factored& m, const double* z, FacGeom& g) {
    for (int i = 0; i < m.d; ++i) {
        const auto& gr = m.grid[(size_t)i];
        if (!(gr.front() <= z[i] && z[i] <= gr.back())) return false;
    }
    for (int i = 0; i < m.d; ++i) {
        const auto& gr = m.grid[(size_t)i];
        find_cell(gr, z[i], g.k[i], g.t[i]);
        g.inv_delta[i] = gr.size() > 1 ? 1.0 / (gr[(size_t)g.k[i] + 1] - gr[(size_t)g.k[i]]) : 0.0;
    }
    return true;
}

// One source at one point: its corner rows, w_c, d w_c / d (own axis j), the rate M_s(z) and its slopes; with order 2 also the
// mixed second derivatives d2 w_c / d (own axes j < k) and d2M of them, pair (j, k) at k (k - 1) / 2 + j (the morph is
// multilinear: d_jj = 0).  Corner c: bit of the first own axis most significant; w_c the product of t or 1 - t in own-axis order
// from 1.0; M_s left to right from 0.0 (interp_mus); the slopes as PointDerivs forms them.
struct FacSource {
    int e, nc;
    int64_t row[1 << kFacMaxOwn];
    double w[1 << kFacMaxOwn], dw[1 << kFacMaxOwn][kFacMaxOwn], d2w[1 << kFacMaxOwn][kFacMaxOwn];
    double M, dM[kFacMaxOwn], d2M[kFacMaxOwn];

    // order: 0 the weights and M alone, 1 with the slopes, 2 with the second derivatives
    void at(const bi_ctx::Factored& m, int s, const FacGeom& g, int order) {
        const bool slopes = order >= 1;
        e = m.n_own[(size_t)s];
        nc = 1 << e;
        const int* ax = &m.own[(size_t)s * kFacMaxOwn];
        const int64_t* st = &m.own_stride[(size_t)s * kFacMaxOwn];
        int64_t base = m.row_first[(size_t)s];
        for (int j = 0; j < e; ++j) base += (int64_t)g.k[ax[j]] * st[j];
        auto factor = [&](int c, int j, bool diff) {
            const bool up = (c >> (e - 1 - j)) & 1;
            if (diff) return (up ? 1.0 : -1.0) * g.inv_delta[ax[j]];
            return up ? g.t[ax[j]] : (1 - g.t[ax[j]]);
        };
        for (int c = 0; c < nc; ++c) {
            int64_t r = base;
            double wc = 1.0;
            for (int j = 0; j < e; ++j) {
                if ((c >> (e - 1 - j)) & 1) r += st[j];
                wc = wc * factor(c, j, false);
            }
            row[c] = r;
            w[c] = wc;
            for (int i = 0; slopes && i < e; ++i) {
                double v = factor(c, i, true);
                for (int j = 0; j < e; ++j)
                    if (j != i) v *= factor(c, j, false);
                dw[c][i] = v;
            }
            for (int k = 1; order >= 2 && k < e; ++k)
                for (int i = 0; i < k; ++i) {
                    double v = 1.0;
                    for (int j = 0; j < e; ++j) v *= factor(c, j, j == i || j == k);
                    d2w[c][k * (k - 1) / 2 + i] = v;
                }
        }
        double v = 0.0;
        for (int c = 0; c < nc; ++c) {
            const double term = m.h_mus[(size_t)row[c]] * w[c];
            v = v + term;
        }
        M = v;
        for (int i = 0; slopes && i < e; ++i) {
            double dv = 0.0;
            for (int c = 0; c < nc; ++c) dv += dw[c][i] * m.h_mus[(size_t)row[c]];
            dM[i] = dv;
        }
        for (int x = 0; order >= 2 && x < e * (e - 1) / 2; ++x) {
            double dv = 0.0;
            for (int c = 0; c < nc; ++c) dv += d2w[c][x] * m.h_mus[(size_t)row[c]];
            d2M[x] = dv;
        }
    }
};

// the early exits of one point, in screen_point's order: dataset (where the call reads data), anchor box (every axis), rates
int32_t fac_screen(const bi_ctx::Factored& m, const double* z, const double* rs, int64_t ds, bool dataset_test, FacGeom& g) {
    if (dataset_test && (ds < 0 || ds >= (m.ev_ready ? m.ev_T : m.T))) return BI_ST_BAD_DATASET;
    if (!fac_geometry(m, z, g)) return BI_ST_OUT_OF_BOUNDS;
    const double inf = std::numeric_limits<double>::infinity();
    FacSource fs;
    for (int s = 0; s < m.S; ++s) {
        fs.at(m, s, g, 0);
        const double r = rs ? fs.M * rs[s] : fs.M;
        if (!(r >= 0 && r < inf)) return BI_ST_UNPHYSICAL;
    }
    return 0;
}

// events_ok: the call serves the event store (bi_sourcewise_events.h) -- bi_eval_factored, the native fit and the store's own
// entry points; while a store exists every other source-wise call is refused, and those read it instead of the counts
int fac_check(bi_ctx* c, const char* who, bool need_counts, bool events_ok = false) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    if (!c->fac.ready) return fail(c, BI_ERR_STATE, "%s: no source-wise model uploaded (bi_factored_begin ... bi_factored_end first)", who);
    if (c->fac.ev_ready || c->fac.ev_open) {
        if (!events_ok)
            return fail(c, BI_ERR_STATE, "%s: the context holds an event store (it is an unbinned source-wise likelihood): "
                        "bi_sourcewise_drop_events first", who);
        if (need_counts && !c->fac.ev_ready)
            return fail(c, BI_ERR_STATE, "%s: the event store is still being filled (bi_sourcewise_events_end first)", who);
        return BI_OK;
    }
    if (need_counts && (c->fac.T < 1 || !c->fac.counts.p))
        return fail(c, BI_ERR_STATE, "%s: no counts uploaded (bi_factored_set_counts first)", who);
    return BI_OK;
}

// The non-empty-bin form (bi_sourcewise_nonempty.h) belongs to the counts and the model it was built from: whatever replaces
// either releases it (bi_factored_begin, bi_factored_set_counts, bi_sourcewise_generate_toys), and bi_sourcewise_drop_nonempty.
void fac_drop_nonempty(bi_ctx::Factored& m) {
    m.ne_ready = false;
    m.ne_bytes = 0;
    m.ne_max_nbx = 1;
    m.ne_off.clear(); m.ne_np.clear(); m.ne_cnt_off.clear();
    dev_free(m.ne_ps); dev_free(m.ne_cnt); dev_free(m.ne_tab);
}
// The event store (bi_sourcewise_events.h) belongs to the model: bi_factored_begin and bi_sourcewise_drop_events release it.
void fac_drop_events(bi_ctx::Factored& m) {
    m.ev_ready = m.ev_open = false;
    m.ev_T = m.ev_cols = m.ev_bytes = 0;
    m.ev_outlier = 0.0;
    m.ev_first.clear(); m.ev_n.clear(); m.ev_row_set.clear();
    dev_free(m.ev_ps);
    dev_free(m.ev_tab);
    m.ev_max_nbx = 1;
    dev_free(m.sim_coords); dev_free(m.sim_source);      // (the events a simulated store was scored from)
    m.sim_k = 0;
    m.sim_n = -1;
}
// do bi_eval_factored (and with it the native fit), bi_eval_sourcewise_planned and bi_sample_stretch_sourcewise run on it
bool fac_nonempty_on(const bi_ctx* c) { return c->fac.ne_ready && c->sourcewise_form == 1; }

// sum_b lgamma(n + 1) of the T dense datasets counts [T][Bp] (device) -> lgsum [T], once per upload or generator call: the kernels
// of the grid model's counts (finish_counts).  e: the error state of what the caller queued before; synchronises the stream.
int fac_counts_lgsum(bi_ctx* c, const char* who, const double* counts, int64_t T, hipError_t e, std::vector<double>& lgsum) {
    const int64_t B = c->fac.B, Bp = c->fac.Bp;
    const int nblk = (int)std::min<int64_t>(256, (B + kThreads - 1) / kThreads);
    const int64_t chunk = 32768;
    ScratchBuf part, lg;
    lgsum.assign((size_t)T, 0.0);
    int rc;
    if ((rc = dev_alloc(c, part, (size_t)std::min(T, chunk) * nblk * sizeof(double))) || (rc = dev_alloc(c, lg, (size_t)T * sizeof(double)))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    for (int64_t t0 = 0; t0 < T && e == hipSuccess; t0 += chunk) {
        const int64_t nt = std::min(chunk, T - t0);
        hipLaunchKernelGGL(k_counts_lgamma, dim3(nblk, (unsigned)nt), dim3(kThreads), 0, c->stream, counts + t0 * Bp, B, Bp, (double*)part.p, nblk);
        hipLaunchKernelGGL(k_rows_sum, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, (const double*)part.p, nblk,
                           (double*)lg.p + t0, nt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(lgsum.data(), lg.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return BI_OK;
}

// The device planner's copy (k_sourcewise_plan, bi_sourcewise_plan.h) of what fac_geometry and FacSource::at read, one slab:
// anchors, anchor_off [d + 1], n_own [S], own [S][3], own_stride [S][3], row_first [S], h_mus [rows], h_rowsum [rows] at
// geom_off[0 .. 8).
// Waits for the copy (the staging block is the context's).
int fac_upload_geometry(bi_ctx* c) {
    bi_ctx::Factored& m = c->fac;
    std::vector<double> anchors;
    std::vector<int32_t> anchor_off(1, 0), n_own(m.n_own.begin(), m.n_own.end()), own(m.own.begin(), m.own.end());
    for (const auto& g : m.grid) {
        anchors.insert(anchors.end(), g.begin(), g.end());
        anchor_off.push_back((int32_t)anchors.size());
    }
    HIP_TRY(c, hipSetDevice(c->device));
    PackedUpload pu;
    int rc = packed_upload(c, {{anchors.data(), anchors.size() * sizeof(double)}, {anchor_off.data(), anchor_off.size() * sizeof(int32_t)},
                               {n_own.data(), n_own.size() * sizeof(int32_t)}, {own.data(), own.size() * sizeof(int32_t)},
                               {m.own_stride.data(), m.own_stride.size() * sizeof(int64_t)}, {m.row_first.data(), (size_t)m.S * sizeof(int64_t)},
                               {m.h_mus.data(), m.h_mus.size() * sizeof(double)}, {m.h_rowsum.data(), m.h_rowsum.size() * sizeof(double)}},
                           0, pu, &m.geom);
    if (rc) return rc;
    for (size_t q = 0; q < 8; ++q) m.geom_off[q] = pu.off[q];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

// ... and of h_lgsum, wherever that changes: a planned evaluation after new counts or toys must not subtract the old sums
int fac_sync_lgsum(bi_ctx* c, const char* who) {
    bi_ctx::Factored& m = c->fac;
    int rc = dev_upload(c, m.lgsum_dev, m.h_lgsum);
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);      // (h_lgsum is pageable and may be swapped again)
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return BI_OK;
}

// What bi_eval_factored, bi_eval_sourcewise_hess and bi_eval_sourcewise_fisher share: the screen of the P points, the descriptors
// of the live ones (filled on host threads), their one packed upload, and the launch of a kernel over them in sub-batches.
//   order 0 / 1    value / with the gradient's columns (k_morph_factored)
//   order 2        with the second-order columns chi and d2M (k_factored_curv, observed form)
//   order 3        no data: the first-order columns and the chain coefficients of the unbounded counts (k_factored_curv, Fisher form)
struct FacBatch {
    bi_ctx* c;
    const bi_ctx::Factored& m;
    int order, d, S, SC, EM, W, NX, WC, NR;
    std::vector<int64_t> live;
    int64_t n_items = 0;
    std::vector<int64_t> rowoff, cnt_off;
    std::vector<double> coef, rates, chain;
    std::vector<double> hM, hdM, hd2M;          // [n][S], [n][S][kFacMaxOwn] (order >= 1), [n][S][kFacMaxOwn] (order 2): the chain rule's
    PackedUpload pu;
    size_t first_extra = 0;                     // index of the caller's first own part in pu

    bool dataset_test;                          // the screen tests the dataset index (calls that read counts)
    mutable int64_t pieces = 0;                 // run_item_chunks' chunks over every run() so far: last_point_pieces
    // the non-empty-bin form (order 0 / 1, bi_sourcewise_nonempty.h): the descriptors point into the dataset's compacted copy
    bool nonempty;
    std::vector<int32_t> tiles;                 // [n] tiles of the item's dataset's list
    std::vector<double> lam_sum;                // [n] sum_s lambda_s, sources ascending from 0.0
    std::vector<double> hN, hdN;                // [n][S] N_s = sum_c w_c R_{s,c}; [n][S][kFacMaxOwn] d_j N_s (order 1)
    // the event store (order 0 / 1 / 2, bi_sourcewise_events.h): the descriptors point at the item's event set's columns; `tiles`
    // are the set's, lam_sum is sum_s r_s (sources ascending from 0.0), cnt_off holds the set's number of events; at order 2 the
    // d2w columns and hd2M as for the counts (bi_eval_sourcewise_events_hess)
    bool events;

    FacBatch(bi_ctx* ctx, int order_, bool reads_counts = true, bool nonempty_ = false)
        : c(ctx), m(ctx->fac), order(order_), d(m.d), S(m.S), SC(S <= 2 ? 2 : S <= 4 ? 4 : 8), EM(std::max(1, m.max_own)), W(1 + EM),
          NX(order_ == 2 ? EM * (EM - 1) / 2 : 0), WC(W + NX), NR(m.n_rows_point), dataset_test(order_ != 3 && reads_counts),
          nonempty(nonempty_ && order_ <= 1 && reads_counts && !ctx->fac.ev_ready),
          events(ctx->fac.ev_ready && order_ <= 2 && reads_counts) {
        c->last_point_pieces = 0;               // (a call with no live item launches nothing)
    }

    // reset(p) writes the caller's defaults of point p; status [P] (nullable) gets every point's bits
    template <class F>
    void screen(int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, int32_t* status, F reset) {
        std::vector<int32_t> st((size_t)P);
        parallel_for(P, 2048, [&](int64_t lo, int64_t hi) {
            FacGeom g;
            for (int64_t p = lo; p < hi; ++p) {
                reset(p);
                st[(size_t)p] = fac_screen(m, z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr, dataset ? dataset[p] : 0,
                                           dataset_test, g);
            }
        });
        live.reserve((size_t)P);
        for (int64_t p = 0; p < P; ++p) {
            if (status) status[p] = st[(size_t)p];
            if (!st[(size_t)p]) live.push_back(p);
        }
        n_items = (int64_t)live.size();
    }

    // the descriptors of the live points, and what the chain rule needs of them on the host: M_s, its slopes and second differences
    void fill(const double* z, const double* rate_scale, const int64_t* dataset) {
        const size_t n = (size_t)n_items;
        const int so = order == 0 ? 0 : order == 2 ? 2 : 1;      // what FacSource::at computes (the Fisher form: first order)
        rowoff.assign(n * NR, 0);
        cnt_off.assign(n, 0);
        coef.assign(n * NR * WC, 0.0);
        rates.assign(n * SC, 0.0);
        if (order == 3) chain.assign(n * SC * W, 0.0);
        if (order >= 1) { hM.resize(n * S); hdM.resize(n * S * kFacMaxOwn); }
        if (order == 2) hd2M.resize(n * S * kFacMaxOwn);
        if (events) {
            tiles.assign(n, 1);
            lam_sum.assign(n, 0.0);
        }
        if (nonempty) {
            tiles.assign(n, 1);
            lam_sum.assign(n, 0.0);
            hN.assign(n * S, 0.0);
            if (order >= 1) hdN.assign(n * S * kFacMaxOwn, 0.0);
        }
        parallel_for(n_items, 1024, [&](int64_t lo, int64_t hi) {
            FacGeom g;
            FacSource fs;
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t p = live[(size_t)i];
                const int64_t ds = dataset ? dataset[p] : 0;
                fac_geometry(m, z ? z + p * d : nullptr, g);
                // the rows of the item: the dense tensor's, or those of its dataset's compacted copy
                const int64_t row_base = events ? m.ev_first[(size_t)ds] : nonempty ? m.ne_off[(size_t)ds] : 0;
                const int64_t row_stride = events ? m.ev_cols : nonempty ? m.ne_np[(size_t)ds] : m.Bp;
                double lam = 0.0;
                int k = 0;
                for (int s = 0; s < S; ++s) {
                    fs.at(m, s, g, so);
                    const double rs = rate_scale ? rate_scale[p * S + s] : 1.0;
                    if (nonempty) {
                        // N_s = sum_c w_c R_{s,c} and its slopes, one fma per corner from 0.0; lambda_s = r_s N_s, sources ascending
                        double N = 0.0;
                        for (int cnr = 0; cnr < fs.nc; ++cnr) N = std::fma(fs.w[cnr], m.h_rowsum[(size_t)fs.row[cnr]], N);
                        hN[(size_t)i * S + s] = N;
                        for (int j = 0; order >= 1 && j < fs.e; ++j) {
                            double dN = 0.0;
                            for (int cnr = 0; cnr < fs.nc; ++cnr) dN = std::fma(fs.dw[cnr][j], m.h_rowsum[(size_t)fs.row[cnr]], dN);
                            hdN[((size_t)i * S + s) * kFacMaxOwn + j] = dN;
                        }
                        const double r = rate_scale ? fs.M * rate_scale[p * S + s] : fs.M;
                        const double lambda = r * N;
                        lam = lam + lambda;
                    }
                    for (int cnr = 0; cnr < fs.nc; ++cnr, ++k) {
                        rowoff[(size_t)i * NR + k] = row_base + fs.row[cnr] * row_stride;
                        double* q = &coef[((size_t)i * NR + k) * WC];
                        q[0] = fs.w[cnr];
                        for (int j = 0; order >= 1 && j < fs.e; ++j) q[1 + j] = fs.dw[cnr][j];
                        for (int x = 0; order == 2 && x < fs.e * (fs.e - 1) / 2; ++x) q[W + x] = fs.d2w[cnr][x];
                    }
                    rates[(size_t)i * SC + s] = rate_scale ? fs.M * rate_scale[p * S + s] : fs.M;
                    if (events) lam = lam + rates[(size_t)i * SC + s];
                    if (order >= 1) {
                        hM[(size_t)i * S + s] = fs.M;
                        for (int j = 0; j < fs.e; ++j) hdM[((size_t)i * S + s) * kFacMaxOwn + j] = fs.dM[j];
                    }
                    for (int x = 0; order == 2 && x < fs.e * (fs.e - 1) / 2; ++x) hd2M[((size_t)i * S + s) * kFacMaxOwn + x] = fs.d2M[x];
                    if (order == 3) {
                        double* q = &chain[((size_t)i * SC + s) * W];
                        q[0] = fs.M;
                        for (int j = 0; j < fs.e; ++j) q[1 + j] = rs * fs.dM[j];
                    }
                }
                cnt_off[(size_t)i] = events ? m.ev_n[(size_t)ds] : nonempty ? m.ne_cnt_off[(size_t)ds] : dataset_test ? ds * m.Bp : 0;
                if (events) {
                    const int64_t n_ev = m.ev_n[(size_t)ds];
                    tiles[(size_t)i] = (int32_t)std::max<int64_t>(1, (n_ev + kTile - 1) / kTile);
                    lam_sum[(size_t)i] = lam;
                }
                if (nonempty) {
                    tiles[(size_t)i] = (int32_t)(m.ne_np[(size_t)ds] / kTile);
                    lam_sum[(size_t)i] = lam;
                }
            }
        });
    }

    // one packed copy of the descriptors and of the caller's `extra` parts (pu.dev(first_extra + k)); out_doubles results behind them
    int upload(std::vector<std::pair<const void*, size_t>> extra, size_t out_doubles) {
        std::vector<std::pair<const void*, size_t>> parts = {
            {rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)},
            {rates.data(), rates.size() * sizeof(double)}, {cnt_off.data(), cnt_off.size() * sizeof(int64_t)},
            {chain.data(), chain.size() * sizeof(double)}, {tiles.data(), tiles.size() * sizeof(int32_t)}};
        first_extra = parts.size();
        parts.insert(parts.end(), extra.begin(), extra.end());
        return packed_upload(c, parts, out_doubles * sizeof(double), pu);
    }
    const double* out() const { return (const double*)pu.host_out(); }

    // what every launch over this batch shares: the model, the tile geometry, the sources' own axes
    FactoredArgs args() const {
        FactoredArgs a{};
        a.ps = (const double*)m.ps.p;
        a.counts = (const double*)m.counts.p;
        a.n_tiles = (int)(m.Bp / kTile);
        a.NR = NR;
        a.chunks = (int)c->tile_chunks;
        a.lead = 0u;
        bool seen[kFacMaxDim] = {};
        for (int s = 0; s < 8; ++s) {
            a.e[s] = s < S ? m.n_own[(size_t)s] : -1;
            for (int j = 0; j < kFacMaxOwn; ++j) {
                const int ax = (s < S && j < m.n_own[(size_t)s]) ? m.own[(size_t)s * kFacMaxOwn + j] : -1;
                a.ax[s][j] = (signed char)ax;
                if (ax >= 0 && !seen[ax]) {
                    seen[ax] = true;
                    a.lead |= 1u << (s * 3 + j);
                }
            }
        }
        return a;
    }
    // ... and the descriptors of the items from `at` on
    void point_at(FactoredArgs& b, int64_t at) const {
        b.rowoff = pu.dev<int64_t>(0) + at * NR;
        b.coef = pu.dev<double>(1) + at * NR * WC;
        b.rates = pu.dev<double>(2) + at * SC;
        b.item_cnt = pu.dev<int64_t>(3) + at;
        b.chain = pu.dev<double>(4) + at * SC * W;
    }

    // One kernel over the live points: nsl result slots per item, perm / slot_lg [n][nsl] (device) where a slot's sum goes and
    // what k_finish subtracts from it.  The blocks of an item depend on the rows' length alone; sub-batches keep the partial
    // sums of one run_item_chunks call within kFacPartialDoubles.  launch(args, grid) -> error code.  last_point_pieces counts
    // the chunks of every sub-batch of every run() of this batch (the curvature calls run once per Gram panel);
    // last_morph_nbx / last_morph_items / last_morph_fused (= 0) describe the grid of the most recent launch, as bi_grad.h's do.
    template <class L>
    int run(int nsl, const int64_t* perm, const double* slot_lg, const char* what, L launch) const {
        const FactoredArgs a = args();
        const int nbx = std::min(a.n_tiles, kFacBlocks);
        const int64_t per_call = std::max<int64_t>(1, kFacPartialDoubles / ((int64_t)nbx * nsl));
        for (int64_t j0 = 0; j0 < n_items; j0 += per_call) {
            const int64_t nj = std::min(per_call, n_items - j0);
            const int rc = run_item_chunks(c, nj, a.n_tiles, nsl, perm + j0 * nsl, slot_lg + j0 * nsl, (double*)pu.host_out(), nullptr, what,
                                           [&](int64_t i0, dim3 grid, double* partial, unsigned* pflags) {
                                               FactoredArgs b = a;
                                               point_at(b, j0 + i0);
                                               b.partial = partial;
                                               b.pflags = pflags;
                                               c->last_morph_nbx = grid.x; c->last_morph_items = grid.y; c->last_morph_fused = 0;
                                               return launch(b, grid);
                                           },
                                           nbx);
            if (rc) return rc;
            pieces += c->last_point_pieces;
            c->last_point_pieces = pieces;
        }
        return BI_OK;
    }

    // run() over per-item lists: Args is SourcewiseNonemptyArgs (k_sourcewise_nonempty over the items' compacted copies) or
    // SourcewiseEventsArgs (k_sourcewise_events over the items' event sets), `a` holds what is the same for every item and
    // item_at(b, at) points b at what part 3 of the upload means to the kernel (the item's counts, or its number of events).  An
    // item's blocks are min(its tiles, kFacBlocks) -- its own list alone decides; the grid's x is the largest of them over the
    // batch (the other blocks post +0.0), which sizes the partial buffers and the sub-batches and changes no bit of any item.
    template <class Args, class At, class L>
    int run_lists(Args a, At item_at, int nsl, const int64_t* perm, const double* slot_lg, const char* what, L launch) const {
        a.NR = NR;
        a.chunks = (int)c->tile_chunks;
        a.max_blocks = kFacBlocks;
        for (int s = 0; s < 8; ++s) a.e[s] = s < S ? m.n_own[(size_t)s] : -1;
        int nbx = 1;
        for (int32_t t : tiles) nbx = std::max(nbx, std::min((int)t, kFacBlocks));
        const int64_t per_call = std::max<int64_t>(1, kFacPartialDoubles / ((int64_t)nbx * nsl));
        for (int64_t j0 = 0; j0 < n_items; j0 += per_call) {
            const int64_t nj = std::min(per_call, n_items - j0);
            const int rc = run_item_chunks(c, nj, nbx, nsl, perm + j0 * nsl, slot_lg + j0 * nsl, (double*)pu.host_out(), nullptr, what,
                                           [&](int64_t i0, dim3 grid, double* partial, unsigned* pflags) {
                                               Args b = a;
                                               const int64_t at = j0 + i0;
                                               b.rowoff = pu.dev<int64_t>(0) + at * NR;
                                               b.coef = pu.dev<double>(1) + at * NR * WC;
                                               b.rates = pu.dev<double>(2) + at * SC;
                                               item_at(b, at);
                                               b.item_tiles = pu.dev<int32_t>(5) + at;
                                               b.partial = partial;
                                               b.pflags = pflags;
                                               c->last_morph_nbx = grid.x; c->last_morph_items = grid.y; c->last_morph_fused = 0;
                                               return launch(b, grid);
                                           },
                                           nbx);
            if (rc) return rc;
            pieces += c->last_point_pieces;
            c->last_point_pieces = pieces;
        }
        return BI_OK;
    }
    // ... on the non-empty-bin form
    template <class L>
    int run_nonempty(int nsl, const int64_t* perm, const double* slot_lg, const char* what, L launch) const {
        SourcewiseNonemptyArgs a{};
        a.ps = (const double*)m.ne_ps.p;
        a.counts = (const double*)m.ne_cnt.p;
        return run_lists(a, [&](SourcewiseNonemptyArgs& b, int64_t at) { b.item_cnt = pu.dev<int64_t>(3) + at; }, nsl, perm, slot_lg, what, launch);
    }
    // ... on the event store
    template <class L>
    int run_events(int nsl, const int64_t* perm, const double* slot_lg, const char* what, L launch) const {
        SourcewiseEventsArgs a{};
        a.ps = (const double*)m.ev_ps.p;
        a.outlier = m.ev_outlier;
        return run_lists(a, [&](SourcewiseEventsArgs& b, int64_t at) { b.item_n = pu.dev<int64_t>(3) + at; }, nsl, perm, slot_lg, what, launch);
    }

    // the chain rule of item i's gradient sums h (the slots of k_morph_factored<.., GRAD>) to gp [d + S]: sources ascending, own
    // axes ascending within a source; gz [max(d, 1)] is the caller's scratch
    void gradient(int64_t i, const double* h, const double* rate_scale, double* gp, std::vector<double>& gz) const {
        const int64_t p = live[(size_t)i];
        std::fill(gz.begin(), gz.end(), 0.0);
        for (int s = 0; s < S; ++s) {
            const double M = hM[(size_t)i * S + s], G = h[1 + s];
            const double rs = rate_scale ? rate_scale[p * S + s] : 1.0;
            gp[d + s] = M * G;
            for (int j = 0; j < m.n_own[(size_t)s]; ++j) {
                const int ax = m.own[(size_t)s * kFacMaxOwn + j];
                const double U = h[1 + SC + s * EM + j], dM = hdM[((size_t)i * S + s) * kFacMaxOwn + j];
                gz[(size_t)ax] = gz[(size_t)ax] + rs * (M * U + dM * G);
            }
        }
        for (int i2 = 0; i2 < d; ++i2) gp[i2] = gz[(size_t)i2];
    }
};

int factored_eval(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll, double* grad,
                  int32_t* status) {
    const bool want_grad = grad != nullptr;
    const bool ne = fac_nonempty_on(c);         // the non-empty-bin form (bi_sourcewise_nonempty.h), where it is built and chosen
    const bool evs = c->fac.ev_ready;           // the event store (bi_sourcewise_events.h): the unbinned likelihood
    FacBatch b(c, want_grad ? 1 : 0, true, ne);
    const int d = b.d, S = b.S, NSL = factored_slots(b.SC, b.EM, want_grad);
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));

    b.screen(P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = -inf;
        for (int j = 0; want_grad && j < d + S; ++j) grad[p * (d + S) + j] = qnan;
    });
    const int64_t n_items = b.n_items;
    if (n_items == 0) return BI_OK;
    b.fill(z, rate_scale, dataset);
    const size_t n = (size_t)n_items;
    std::vector<int64_t> perm(n * NSL);
    std::vector<double> slot_lg(n * NSL, 0.0);
    for (size_t q = 0; q < perm.size(); ++q) perm[q] = (int64_t)q;
    for (size_t i = 0; i < n; ++i) {
        if (evs) { slot_lg[i * NSL] = b.lam_sum[i]; continue; }     // (sum_s r_s: there is no lgamma over events)
        const double lg = b.m.h_lgsum[(size_t)(dataset ? dataset[b.live[i]] : 0)];
        slot_lg[i * NSL] = ne ? b.lam_sum[i] + lg : lg;         // (k_finish subtracts sum_s lambda_s + lgsum: one number per item)
    }
    int rc = b.upload({{perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}}, n * NSL);
    if (rc) return rc;
    const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1);
    if (evs)
        rc = b.run_events(NSL, b.pu.dev<int64_t>(b.first_extra), b.pu.dev<double>(b.first_extra + 1), "bi_eval_factored",
                          [&](const SourcewiseEventsArgs& a, dim3 grid) {
                              const int e = launch_sourcewise_events(c, b.SC, b.EM, want_grad, a, grid);
                              return e ? fail(c, e, "bi_eval_factored: no kernel variant for %d source slots with %d own axes", b.SC, b.EM) : BI_OK;
                          });
    else if (ne)
        rc = b.run_nonempty(NSL, b.pu.dev<int64_t>(b.first_extra), b.pu.dev<double>(b.first_extra + 1), "bi_eval_factored",
                            [&](const SourcewiseNonemptyArgs& a, dim3 grid) {
                                const int e = launch_sourcewise_nonempty(c, b.SC, b.EM, want_grad, a, grid);
                                return e ? fail(c, e, "bi_eval_factored: no kernel variant for %d source slots with %d own axes", b.SC, b.EM) : BI_OK;
                            });
    else
        rc = b.run(NSL, b.pu.dev<int64_t>(b.first_extra), b.pu.dev<double>(b.first_extra + 1), "bi_eval_factored",
                   [&](const FactoredArgs& a, dim3 grid) {
                       const int e = launch_morph_factored(c, b.SC, b.EM, want_grad, a, grid, nt);
                       return e ? fail(c, e, "bi_eval_factored: no kernel variant for %d source slots with %d own axes", b.SC, b.EM) : BI_OK;
                   });
    if (rc) return rc;

    const double* out = b.out();
    std::vector<double> gz((size_t)std::max(d, 1)), h_ne((size_t)NSL);
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = b.live[(size_t)i];
        const double* h = out + (size_t)i * NSL;
        ll[p] = h[0];
        if (!want_grad || !std::isfinite(h[0])) continue;
        if (evs) {
            // sum_e g tau_s - 1: a pdf integrates to 1 exactly, and its integral has no slope, so the ups slots stand as they are
            std::copy(h, h + NSL, h_ne.begin());
            for (int s = 0; s < S; ++s) h_ne[(size_t)(1 + s)] = h[1 + s] - 1.0;
            h = h_ne.data();
        } else if (ne) {
            // the sums over the listed bins less the rows' totals: sum_Z g tau_s - N_s and sum_Z g ups_s,j - d_j N_s are what the
            // dense kernel's slots hold (sum_b f tau_s, sum_b f ups_s,j); then the same chain rule
            std::copy(h, h + NSL, h_ne.begin());
            for (int s = 0; s < S; ++s) {
                h_ne[(size_t)(1 + s)] = h[1 + s] - b.hN[(size_t)i * S + s];
                for (int j = 0; j < b.m.n_own[(size_t)s]; ++j)
                    h_ne[(size_t)(1 + b.SC + s * b.EM + j)] = h[1 + b.SC + s * b.EM + j] - b.hdN[((size_t)i * S + s) * kFacMaxOwn + j];
            }
            h = h_ne.data();
        }
        b.gradient(i, h, rate_scale, grad + p * (d + S), gz);
    }
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_factored_begin(bi_ctx* c, int d, const int32_t* n_anchor, const double* anchor_z, int S, int64_t B, const int32_t* n_own,
                      const int32_t* own_axes) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    if (d < 0 || d > kFacMaxDim) return fail(c, BI_ERR_INVALID, "bi_factored_begin: d=%d outside [0,%d]", d, kFacMaxDim);
    if (S < 1 || S > kFacMaxSources) return fail(c, BI_ERR_INVALID, "bi_factored_begin: S=%d outside [1,%d]", S, kFacMaxSources);
    if (B < 1) return fail(c, BI_ERR_INVALID, "bi_factored_begin: B=%lld (at least one bin)", (long long)B);
    if (d > 0 && (!n_anchor || !anchor_z)) return fail(c, BI_ERR_INVALID, "bi_factored_begin: anchor arrays are NULL");
    if (!n_own) return fail(c, BI_ERR_INVALID, "bi_factored_begin: n_own is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bi_ctx::Factored& m = c->fac;
    m.ready = m.open = false;
    dev_free(m.counts);
    m.T = 0;
    m.h_lgsum.clear();
    dev_free(m.geom);           // (the device planner's copies: the next bi_factored_end and set_counts upload them again)
    dev_free(m.lgsum_dev);
    dev_free(m.real_counts);    // (rows of the previous model's padded length)
    m.real_T = 0;
    release_coarse(c->sw_coarse);   // (groups of the previous model's bins)
    fac_drop_nonempty(m);           // (compacted copies of the previous model's rows)
    fac_drop_events(m);             // (events scored at the previous model's anchors)
    m.d = d; m.S = S; m.B = B;
    m.Bp = std::max<int64_t>(kTile, (B + kTile - 1) / kTile * kTile);
    m.grid.assign((size_t)d, {});
    const double* zp = anchor_z;
    for (int i = 0; i < d; ++i) {
        if (n_anchor[i] < 1) return fail(c, BI_ERR_INVALID, "bi_factored_begin: axis %d has %d anchors", i, n_anchor[i]);
        m.grid[(size_t)i].assign(zp, zp + n_anchor[i]);
        for (int j = 1; j < n_anchor[i]; ++j)
            if (!(zp[j] > zp[j - 1])) return fail(c, BI_ERR_INVALID, "bi_factored_begin: anchor z values of axis %d are not strictly ascending", i);
        zp += n_anchor[i];
    }
    m.n_own.assign((size_t)S, 0);
    m.own.assign((size_t)S * kFacMaxOwn, 0);
    m.own_stride.assign((size_t)S * kFacMaxOwn, 0);
    m.row_first.assign((size_t)S + 1, 0);
    m.n_rows_point = 0;
    m.max_own = 0;
    const int32_t* op = own_axes;
    for (int s = 0; s < S; ++s) {
        const int e = n_own[s];
        if (e < 0 || e > kFacMaxOwn)
            return fail(c, BI_ERR_INVALID, "bi_factored_begin: source %d owns %d axes, outside [0,%d] (more belongs on the full grid)", s, e, kFacMaxOwn);
        if (e > 0 && !own_axes) return fail(c, BI_ERR_INVALID, "bi_factored_begin: own_axes is NULL");
        int64_t rows = 1;
        for (int j = 0; j < e; ++j) {
            const int ax = op[j];
            if (ax < 0 || ax >= d) return fail(c, BI_ERR_INVALID, "bi_factored_begin: source %d owns axis %d, outside [0,%d)", s, ax, d);
            if (j > 0 && ax <= op[j - 1]) return fail(c, BI_ERR_INVALID, "bi_factored_begin: the axes of source %d are not strictly ascending", s);
            if (m.grid[(size_t)ax].size() < 2)
                return fail(c, BI_ERR_INVALID, "bi_factored_begin: source %d owns axis %d, which has a single anchor", s, ax);
            m.own[(size_t)s * kFacMaxOwn + j] = ax;
            rows *= (int64_t)m.grid[(size_t)ax].size();
        }
        int64_t stride = 1;
        for (int j = e - 1; j >= 0; --j) {
            m.own_stride[(size_t)s * kFacMaxOwn + j] = stride;
            stride *= (int64_t)m.grid[(size_t)m.own[(size_t)s * kFacMaxOwn + j]].size();
        }
        m.n_own[(size_t)s] = e;
        m.row_first[(size_t)s + 1] = m.row_first[(size_t)s] + rows;
        m.n_rows_point += 1 << e;
        m.max_own = std::max(m.max_own, e);
        op += e;
    }
    const int64_t rows = m.row_first[(size_t)S];
    m.h_mus.assign((size_t)rows, 0.0);
    m.h_rowsum.assign((size_t)rows, 0.0);
    m.row_set.assign((size_t)rows, 0);
    dev_free(m.ps);
    int rc = dev_alloc(c, m.ps, (size_t)rows * m.Bp * sizeof(double));
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(m.ps.p, 0, (size_t)rows * m.Bp * sizeof(double), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    m.open = true;
    return BI_OK;
}

int bi_factored_set_anchor(bi_ctx* c, int s, int64_t local_index, const double* ps_row, double mu) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    bi_ctx::Factored& m = c->fac;
    if (!m.open) return fail(c, BI_ERR_STATE, "bi_factored_set_anchor: bi_factored_begin first");
    if (s < 0 || s >= m.S) return fail(c, BI_ERR_INVALID, "bi_factored_set_anchor: source %d outside [0,%d)", s, m.S);
    const int64_t rows = m.row_first[(size_t)s + 1] - m.row_first[(size_t)s];
    if (local_index < 0 || local_index >= rows)
        return fail(c, BI_ERR_INVALID, "bi_factored_set_anchor: anchor %lld of source %d outside [0,%lld)", (long long)local_index, s, (long long)rows);
    if (!ps_row) return fail(c, BI_ERR_INVALID, "bi_factored_set_anchor: ps_row is NULL");
    const int64_t r = m.row_first[(size_t)s] + local_index;
    if (m.row_set[(size_t)r])
        return fail(c, BI_ERR_INVALID, "bi_factored_set_anchor: anchor %lld of source %d was set before (each anchor exactly once)", (long long)local_index, s);
    for (int64_t b = 0; b < m.B; ++b)
        if (!(ps_row[b] >= 0.0 && ps_row[b] < std::numeric_limits<double>::infinity()))
            return fail(c, BI_ERR_INVALID, "bi_factored_set_anchor: source %d, anchor %lld, bin %lld holds %g: template entries must be finite and >= 0 "
                        "(sources that may go negative are out of scope of source-wise models)", s, (long long)local_index, (long long)b, ps_row[b]);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync((double*)m.ps.p + (size_t)r * m.Bp, ps_row, (size_t)m.B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // the host buffer is borrowed only for the duration of the call
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    m.h_mus[(size_t)r] = mu;
    long double total = 0.0L;       // R_{s,c}: the row's total over all bins, rounded once (the non-empty-bin form's lambda_s)
    for (int64_t b = 0; b < m.B; ++b) total += (long double)ps_row[b];
    m.h_rowsum[(size_t)r] = (double)total;
    m.row_set[(size_t)r] = 1;
    return BI_OK;
}

int bi_factored_end(bi_ctx* c) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    bi_ctx::Factored& m = c->fac;
    if (!m.open) return fail(c, BI_ERR_STATE, "bi_factored_end: bi_factored_begin first");
    for (int s = 0; s < m.S; ++s)
        for (int64_t r = m.row_first[(size_t)s]; r < m.row_first[(size_t)s + 1]; ++r)
            if (!m.row_set[(size_t)r])
                return fail(c, BI_ERR_STATE, "bi_factored_end: anchor %lld of source %d was never set", (long long)(r - m.row_first[(size_t)s]), s);
    int rc = fac_upload_geometry(c);
    if (rc) return rc;
    m.open = false;
    m.ready = true;
    return BI_OK;
}

int bi_factored_set_counts(bi_ctx* c, int64_t T, const double* counts) {
    int rc = fac_check(c, "bi_factored_set_counts", false);
    if (rc) return rc;
    bi_ctx::Factored& m = c->fac;
    if (T < 1 || !counts) return fail(c, BI_ERR_INVALID, "bi_factored_set_counts: T = %lld (at least one dataset) or counts is NULL", (long long)T);
    const int64_t B = m.B, Bp = m.Bp;
    for (int64_t t = 0; t < T; ++t)
        for (int64_t b = 0; b < B; ++b) {
            const double n = counts[t * B + b];
            if (!(n >= 0.0 && n < std::numeric_limits<double>::infinity()))
                return fail(c, BI_ERR_INVALID, "bi_factored_set_counts: dataset %lld, bin %lld holds %g: every count must be finite and >= 0",
                            (long long)t, (long long)b, n);
        }
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<double> padded((size_t)(T * Bp), 0.0);
    for (int64_t t = 0; t < T; ++t) std::copy(counts + t * B, counts + (t + 1) * B, padded.begin() + (size_t)(t * Bp));
    DevBuf fresh;
    if ((rc = dev_alloc(c, fresh, padded.size() * sizeof(double)))) return rc;
    hipError_t e = hipMemcpyAsync(fresh.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
    std::vector<double> lgsum;
    if ((rc = fac_counts_lgsum(c, "bi_factored_set_counts", (const double*)fresh.p, T, e, lgsum))) {
        dev_free(fresh);
        return rc;
    }
    dev_free(m.counts);
    m.counts = fresh;
    m.T = T;
    m.h_lgsum.swap(lgsum);
    fac_drop_nonempty(m);           // (lists of the previous counts)
    return fac_sync_lgsum(c, "bi_factored_set_counts");
}

int bi_eval_factored(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll, double* grad,
                     int32_t* status) {
    int rc = fac_check(c, "bi_eval_factored", true, true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !ll)) return fail(c, BI_ERR_INVALID, "bi_eval_factored: bad P / output pointer");
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "bi_eval_factored: z is NULL");
    if (P == 0) return BI_OK;
    return factored_eval(c, P, z, rate_scale, dataset, ll, grad, status);
}

int bi_fit_batched_factored(bi_ctx* c, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                            const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                            const double* hi, const int32_t* n_kinks, const double* kinks, double gtol, int max_iter,
                            const double* prior_mean, const double* prior_sigma, const double* prior_const, double* x_out,
                            double* f_out, int32_t* flags_out, int64_t* counters) {
    int rc = fac_check(c, "bi_fit_batched_factored", true, true);
    if (rc) return rc;
    return fit_batched(c, "bi_fit_batched_factored", kFitFactored, P, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks,
                       gtol, max_iter, prior_mean, prior_sigma, prior_const, x_out, f_out, flags_out, counters);
}

}  // extern "C"
