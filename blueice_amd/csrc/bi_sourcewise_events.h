// bi_sourcewise_events.h -- source-wise models: the event store, with which the context is an UNBINNED source-wise likelihood
// (host half; the kernel is k_sourcewise_events, bi_k_sourcewise_events.h).  bi_sourcewise_events_begin / _set_row / _end,
// bi_sourcewise_score_events, bi_sourcewise_drop_events, bi_sourcewise_event_set_counts, bi_sourcewise_download_event_set, and
// bi_eval_sourcewise_events_hess (value, gradient and analytic Hessian over the store; kernel k_sourcewise_events_curv,
// bi_k_sourcewise_events_curv.h).
//
// The reference's source_wise_interpolation keeps, per source, the pdf values of the events at the anchors of the parameters
// that source responds to only.  The store is that: a second form of the data beside the dense counts, [rows][columns] with
// rows = sum_s prod_{i in O_s} n_i the model's rows.  It holds T event sets side by side: set t at the columns
// [first_t, first_t + N_t), first_t a multiple of kTile (so: even), every set padded to whole tiles and to at least one; the
// padding holds zeros and is masked by index in the kernel.  Events keep the caller's order: the order fixes the bits.
//
// The extended unbinned likelihood of a point is then the non-empty-bin form's with the events as the list, n = 1, no lgamma and
// N_s = 1 (a pdf integrates to one, and that integral has no slope):
//     ll = sum_e log lam_e - sum_s r_s,     lam_e = sum_s r_s tau_s,e   (nan sources left out; the outlier clamp on lam_e)
//     d ll / d rs_s = M_s (sum_e g tau_s - 1)
//     d ll / d z_i  = sum_{s: i in O_s} rs_s [M_s sum_e g ups_s,i + d_i M_s (sum_e g tau_s - 1)]
// (factored_eval, bi_factored.h: the subtraction of 1 on the host, then FacBatch::gradient unchanged).
//
// Two ways to fill it: rows scored on the host, each uploaded exactly once (_begin / _set_row / _end), or the model's rows taken
// as density histograms over the analysis space and looked up on the device with bi_score_events' two methods and kernels
// (k_score_locate, k_score_rows: every stored value has the bits bi_score_events gives for that row -- but for 'linear' lookups
// in TWO analysis dimensions, where scipy's RegularGridInterpolator takes a routine of its own that associates the products
// differently: there the store follows scipy, k_score_rows<2, true>, so that device- and host-scored stores agree bit for bit, and
// differs from bi_score_events' tensor by a rounding; events_score_columns, which takes the coordinates where they lie in HBM, so that
// bi_sourcewise_simulate_event_toys, bi_sourcewise_sim.h, scores the events it drew through the same launches).  Both need a finished
// source-wise model for the geometry and the rates; the first does not read the model's rows.
// While a store exists bi_eval_factored and bi_fit_batched_factored evaluate it (`dataset` indexes the event sets) and every
// other source-wise entry point refuses with BI_ERR_STATE (fac_check).  compact_budget bounds its bytes.
#pragma once

namespace {

// the layout of T sets of n[t] events: first [T], the columns of all; BI_ERR_INVALID beyond compact_budget (nothing is built)
int events_layout(bi_ctx* c, const char* who, int64_t T, const int64_t* n_events, std::vector<int64_t>& first, int64_t& cols) {
    if (T < 1 || !n_events) return fail(c, BI_ERR_INVALID, "%s: need T >= 1 event sets and their numbers of events", who);
    first.assign((size_t)T, 0);
    cols = 0;
    for (int64_t t = 0; t < T; ++t) {
        if (n_events[t] < 0) return fail(c, BI_ERR_INVALID, "%s: event set %lld has a negative number of events", who, (long long)t);
        first[(size_t)t] = cols;
        cols += std::max<int64_t>(kTile, (n_events[t] + kTile - 1) / kTile * kTile);
    }
    const int64_t rows = c->fac.row_first[(size_t)c->fac.S];
    const int64_t bytes = rows * cols * (int64_t)sizeof(double);
    if (bytes > c->compact_budget)
        return fail(c, BI_ERR_INVALID, "%s: the event store of %lld sets (%lld columns, %lld rows) takes %lld bytes, more than compact_budget = %lld: "
                    "nothing is built", who, (long long)T, (long long)cols, (long long)rows, (long long)bytes, (long long)c->compact_budget);
    return BI_OK;
}

// a fresh zeroed store of that layout on the context (the previous one is released); ev_open, not ev_ready
int events_create(bi_ctx* c, const char* who, int64_t T, const int64_t* n_events, double outlier) {
    bi_ctx::Factored& m = c->fac;
    if (!(outlier >= 0.0 && outlier < std::numeric_limits<double>::infinity()))
        return fail(c, BI_ERR_INVALID, "%s: outlier_likelihood = %g outside [0, inf)", who, outlier);
    std::vector<int64_t> first;
    int64_t cols = 0;
    int rc = events_layout(c, who, T, n_events, first, cols);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    fac_drop_events(m);
    const int64_t rows = m.row_first[(size_t)m.S];
    const size_t bytes = (size_t)rows * (size_t)cols * sizeof(double);
    if ((rc = dev_alloc(c, m.ev_ps, bytes))) return rc;
    hipError_t e = hipMemsetAsync(m.ev_ps.p, 0, bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        fac_drop_events(m);
        return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    m.ev_T = T;
    m.ev_cols = cols;
    m.ev_bytes = (int64_t)bytes;
    m.ev_outlier = outlier;
    m.ev_first = first;
    m.ev_n.assign(n_events, n_events + T);
    m.ev_row_set.assign((size_t)rows, 0);
    m.ev_open = true;
    return BI_OK;
}

// The lookup of the store's columns: coords_dev [k][cols] in HBM in the store's padded layout (whatever the padding columns hold:
// the lookup stays inside every row, and they are set to zero behind it) -> every row of the fresh store of events_create.
// clip: 'linear' lookups clip the coordinates here (events drawn on the device arrive unclipped; a caller's are clipped already).
// Waits for the stream; after a device error the context holds no store.
int events_score_columns(bi_ctx* c, const char* who, int method, int k, const AxisWalk& ax, const double* grid, const double* coords_dev, int clip) {
    bi_ctx::Factored& m = c->fac;
    const int64_t cols = m.ev_cols, rows = m.row_first[(size_t)m.S], T = m.ev_T;
    std::vector<int64_t> pads;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t end = t + 1 < T ? m.ev_first[(size_t)t + 1] : cols;
        for (int64_t col = m.ev_first[(size_t)t] + m.ev_n[(size_t)t]; col < end; ++col) pads.push_back(col);
    }
    ScoreArgs a{};
    a.k = k;
    a.method = method;
    a.clip = clip;
    ax.put(a.n_grid, a.grid_off, a.stride);
    ScratchBuf d_grid, d_base, d_t, d_pad;
    int rc;
    if ((rc = dev_alloc(c, d_grid, (size_t)ax.flat * sizeof(double))) || (rc = dev_alloc(c, d_base, (size_t)cols * sizeof(int64_t))) ||
        (method == 1 && (rc = dev_alloc(c, d_t, (size_t)cols * k * sizeof(double)))) || (!pads.empty() && (rc = dev_upload(c, d_pad, pads)))) {
        (void)hipStreamSynchronize(c->stream);
        fac_drop_events(m);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(d_grid.p, grid, (size_t)ax.flat * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_score_locate, dim3((unsigned)((cols + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, coords_dev, cols, a,
                           (const double*)d_grid.p, (int64_t*)d_base.p, (double*)d_t.p);
        const int per_block = kThreads * score_events_per_thread(method == 0 ? 0 : k);
        const unsigned bx = (unsigned)((cols + per_block - 1) / per_block);
#define BI_ROWS(...)                                                                                                            \
    hipLaunchKernelGGL((k_score_rows<__VA_ARGS__>), dim3(bx, (unsigned)std::min<int64_t>(rows, 65535)), dim3(kThreads), 0, c->stream,       \
                       (const int64_t*)d_base.p, (const double*)d_t.p, cols, a, (const double*)m.ps.p, m.Bp, (int)rows, (double*)m.ev_ps.p, \
                       cols, (const int32_t*)nullptr)
        switch (method == 0 ? 0 : k) {
            case 0: BI_ROWS(0); break; case 1: BI_ROWS(1); break; case 3: BI_ROWS(3); break;
            case 2: BI_ROWS(2, true); break;    // scipy's own routine for two-dimensional fields: see k_score_rows
            case 4: BI_ROWS(4); break; case 5: BI_ROWS(5); break; case 6: BI_ROWS(6); break; case 7: BI_ROWS(7); break;
            default: BI_ROWS(8); break;
        }
#undef BI_ROWS
        if (!pads.empty()) {
            const int64_t n_fill = rows * (int64_t)pads.size();
            hipLaunchKernelGGL(k_fill_columns, dim3((unsigned)((n_fill + 255) / 256)), dim3(256), 0, c->stream, (double*)m.ev_ps.p, cols, rows,
                               (const int64_t*)d_pad.p, (int64_t)pads.size(), 0.0);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // the grid and the host blocks are borrowed for the call only
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        fac_drop_events(m);
        return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return BI_OK;
}

// The store is complete: the device planner's table of the sets (ev_first, ev_n: k_sourcewise_plan's event variant,
// bi_sourcewise_plan.h) and the most blocks an item of any set takes, then ev_ready.  Waits for the copy; on an error the store
// stays as it was (open).
int events_finish(bi_ctx* c, const char* who) {
    bi_ctx::Factored& m = c->fac;
    std::vector<int64_t> tab(m.ev_first);
    tab.insert(tab.end(), m.ev_n.begin(), m.ev_n.end());
    int64_t max_tiles = 1;
    for (int64_t n : m.ev_n) max_tiles = std::max(max_tiles, (n + kTile - 1) / kTile);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = dev_upload(c, m.ev_tab, tab);
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);      // (tab is pageable and leaves with the scope)
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    m.ev_max_nbx = (int)std::min<int64_t>(max_tiles, kFacBlocks);
    m.ev_open = false;
    m.ev_ready = true;
    return BI_OK;
}
// ... of the fresh store of events_create, every row filled by the scoring kernels; after an error the context holds no store
int events_close(bi_ctx* c, const char* who) {
    std::fill(c->fac.ev_row_set.begin(), c->fac.ev_row_set.end(), 1);
    const int rc = events_finish(c, who);
    if (rc) fac_drop_events(c->fac);
    return rc;
}

int sourcewise_score_events(bi_ctx* c, int method, int k, const int32_t* n_grid, const double* grid, int64_t T, const int64_t* offsets,
                            const double* coords, double outlier) {
    const char* who = "bi_sourcewise_score_events";
    bi_ctx::Factored& m = c->fac;
    if (method != 0 && method != 1) return fail(c, BI_ERR_INVALID, "%s: method must be 0 (piecewise) or 1 (linear)", who);
    AxisWalk ax;
    int rc = walk_axes(c, k, n_grid, grid, 2, method == 1, kGridWords, ax);
    if (rc) return rc;
    if (ax.bins != m.B)
        return fail(c, BI_ERR_INVALID, "%s: the grid describes %lld bins, the model's rows have %lld", who, (long long)ax.bins, (long long)m.B);
    if (T < 1 || !offsets) return fail(c, BI_ERR_INVALID, "%s: need T >= 1 event sets and their offsets", who);
    if (offsets[0] != 0) return fail(c, BI_ERR_INVALID, "%s: offsets[0] must be 0", who);
    std::vector<int64_t> n((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        if (offsets[t + 1] < offsets[t]) return fail(c, BI_ERR_INVALID, "%s: offsets are not ascending at set %lld", who, (long long)t);
        n[(size_t)t] = offsets[t + 1] - offsets[t];
    }
    const int64_t N = offsets[T];
    if (N > 0 && !coords) return fail(c, BI_ERR_INVALID, "%s: coords is NULL", who);
    if ((rc = events_create(c, who, T, n.data(), outlier))) return rc;
    const int64_t cols = m.ev_cols;
    if (N > 0) {
        // the caller's events at their columns; a padding column is looked up at the first grid value of every axis (inside every
        // row) and set to zero behind the lookup
        std::vector<double> padded((size_t)cols * k);
        for (int i = 0; i < k; ++i) {
            double* row = padded.data() + (size_t)i * cols;
            std::fill(row, row + cols, grid[ax.off[i]]);
            for (int64_t t = 0; t < T; ++t)
                std::copy(coords + (size_t)i * N + offsets[t], coords + (size_t)i * N + offsets[t + 1], row + m.ev_first[(size_t)t]);
        }
        ScratchBuf d_ev;
        if ((rc = dev_alloc(c, d_ev, (size_t)cols * k * sizeof(double)))) {
            (void)hipStreamSynchronize(c->stream);
            fac_drop_events(m);
            return rc;
        }
        const hipError_t e = hipMemcpyAsync(d_ev.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            fac_drop_events(m);
            return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        }
        // (the caller's events are clipped already: bi_score_events' contract)
        if ((rc = events_score_columns(c, who, method, k, ax, grid, (const double*)d_ev.p, 0))) return rc;
    }
    return events_close(c, who);
}

}  // namespace

extern "C" {

int bi_sourcewise_events_begin(bi_ctx* c, int64_t T, const int64_t* n_events, double outlier_likelihood) {
    int rc = fac_check(c, "bi_sourcewise_events_begin", false, true);
    if (rc) return rc;
    return events_create(c, "bi_sourcewise_events_begin", T, n_events, outlier_likelihood);
}

int bi_sourcewise_events_set_row(bi_ctx* c, int s, int64_t local_index, const double* values) {
    const char* who = "bi_sourcewise_events_set_row";
    int rc = fac_check(c, who, false, true);
    if (rc) return rc;
    bi_ctx::Factored& m = c->fac;
    if (!m.ev_open) return fail(c, BI_ERR_STATE, "%s: bi_sourcewise_events_begin first", who);
    if (s < 0 || s >= m.S) return fail(c, BI_ERR_INVALID, "%s: source %d outside [0,%d)", who, s, m.S);
    const int64_t rows = m.row_first[(size_t)s + 1] - m.row_first[(size_t)s];
    if (local_index < 0 || local_index >= rows)
        return fail(c, BI_ERR_INVALID, "%s: anchor %lld of source %d outside [0,%lld)", who, (long long)local_index, s, (long long)rows);
    const int64_t r = m.row_first[(size_t)s] + local_index;
    if (m.ev_row_set[(size_t)r])
        return fail(c, BI_ERR_INVALID, "%s: anchor %lld of source %d was set before (each row exactly once)", who, (long long)local_index, s);
    int64_t N = 0;
    for (int64_t n : m.ev_n) N += n;
    if (N > 0 && !values) return fail(c, BI_ERR_INVALID, "%s: values is NULL", who);
    for (int64_t e = 0; e < N; ++e)
        if (std::isinf(values[e]))
            return fail(c, BI_ERR_INVALID, "%s: source %d, anchor %lld, event %lld holds %g: values must be finite or nan", who, s,
                        (long long)local_index, (long long)e, values[e]);
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t at = 0;
    for (int64_t t = 0; t < m.ev_T; ++t) {
        const int64_t n = m.ev_n[(size_t)t];
        if (n > 0)
            HIP_TRY(c, hipMemcpyAsync((double*)m.ev_ps.p + (size_t)r * m.ev_cols + m.ev_first[(size_t)t], values + at, (size_t)n * sizeof(double),
                                      hipMemcpyHostToDevice, c->stream));
        at += n;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));       // the host buffer is borrowed only for the duration of the call
    m.ev_row_set[(size_t)r] = 1;
    return BI_OK;
}

int bi_sourcewise_events_end(bi_ctx* c) {
    const char* who = "bi_sourcewise_events_end";
    int rc = fac_check(c, who, false, true);
    if (rc) return rc;
    bi_ctx::Factored& m = c->fac;
    if (!m.ev_open) return fail(c, BI_ERR_STATE, "%s: bi_sourcewise_events_begin first", who);
    for (int s = 0; s < m.S; ++s)
        for (int64_t r = m.row_first[(size_t)s]; r < m.row_first[(size_t)s + 1]; ++r)
            if (!m.ev_row_set[(size_t)r])
                return fail(c, BI_ERR_STATE, "%s: anchor %lld of source %d was never set", who, (long long)(r - m.row_first[(size_t)s]), s);
    return events_finish(c, who);
}

int bi_sourcewise_score_events(bi_ctx* c, int method, int k, const int32_t* n_grid, const double* grid, int64_t T, const int64_t* offsets,
                               const double* coords, double outlier_likelihood) {
    int rc = fac_check(c, "bi_sourcewise_score_events", false, true);
    if (rc) return rc;
    try {
        return sourcewise_score_events(c, method, k, n_grid, grid, T, offsets, coords, outlier_likelihood);
    } catch (const std::bad_alloc&) {
        fac_drop_events(c->fac);
        return fail(c, BI_ERR_NOMEM, "bi_sourcewise_score_events: out of host memory");
    }
}

int bi_sourcewise_drop_events(bi_ctx* c) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    fac_drop_events(c->fac);
    return BI_OK;
}

int bi_sourcewise_event_set_counts(bi_ctx* c, int64_t* counts) {
    if (!c || !counts) return BI_ERR_INVALID;
    if (!c->fac.ev_ready) return fail(c, BI_ERR_STATE, "bi_sourcewise_event_set_counts: the context holds no event store");
    std::copy(c->fac.ev_n.begin(), c->fac.ev_n.end(), counts);
    return BI_OK;
}

int bi_sourcewise_download_event_set(bi_ctx* c, int64_t t, double* out) {
    if (!c) return BI_ERR_INVALID;
    const bi_ctx::Factored& m = c->fac;
    if (!m.ev_ready) return fail(c, BI_ERR_STATE, "bi_sourcewise_download_event_set: the context holds no event store");
    if (t < 0 || t >= m.ev_T) return fail(c, BI_ERR_INVALID, "bi_sourcewise_download_event_set: event set %lld outside [0, %lld)", (long long)t, (long long)m.ev_T);
    const int64_t n = m.ev_n[(size_t)t];
    if (n == 0) return BI_OK;
    if (!out) return fail(c, BI_ERR_INVALID, "bi_sourcewise_download_event_set: out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)n * sizeof(double), (const double*)m.ev_ps.p + m.ev_first[(size_t)t], (size_t)m.ev_cols * sizeof(double),
                                (size_t)n * sizeof(double), (size_t)m.row_first[(size_t)m.S], hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

// bi_eval_sourcewise_hess (bi_factored_curv.h) on the event store: the same batch, panels and second-order host loop
// (fac_curv_hessian), k_sourcewise_events_curv for k_factored_curv.  The linear sums of the event likelihood are L_tau_s =
// sum_e g tau_s - 1 (a pdf integrates to one: sum_s r_s has the second derivatives d_j M_s, rs_s d_jk M_s and nothing else),
// L_ups and L_chi as the kernel gives them; slot 0 less sum_s r_s through k_finish, as factored_eval does for events.
int bi_eval_sourcewise_events_hess(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                                   double* grad, double* hess, int32_t* status) {
    int rc = fac_check(c, "bi_eval_sourcewise_events_hess", true, true);
    if (rc) return rc;
    if (!c->fac.ev_ready)
        return fail(c, BI_ERR_STATE, "bi_eval_sourcewise_events_hess: the context holds no event store (bi_sourcewise_events_begin ... _end or "
                    "bi_sourcewise_score_events first; the Hessian against counts is bi_eval_sourcewise_hess)");
    if (P < 0 || (P > 0 && (!ll || !grad || !hess))) return fail(c, BI_ERR_INVALID, "bi_eval_sourcewise_events_hess: bad P / output pointer");
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "bi_eval_sourcewise_events_hess: z is NULL");
    if (P == 0) return BI_OK;
    FacBatch b(c, 2);
    const int d = b.d, S = b.S, F = d + S, K = b.SC * b.W;
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    b.screen(P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = -inf;
        for (int j = 0; j < F; ++j) grad[p * F + j] = qnan;
        for (int j = 0; j < F * F; ++j) hess[p * F * F + j] = qnan;
    });
    if (b.n_items == 0) return BI_OK;
    b.fill(z, rate_scale, dataset);
    FacCurvPlan plan(b, false);
    for (int64_t i = 0; i < b.n_items; ++i) plan.lg0[(size_t)(i * plan.nsl[0])] = b.lam_sum[(size_t)i];     // (sum_s r_s: no lgamma over events)
    if ((rc = plan.run(c, b, false, "bi_eval_sourcewise_events_hess"))) return rc;

    const double* out = b.out();
    parallel_for(b.n_items, 256, [&](int64_t lo, int64_t hi) {
        std::vector<double> gz((size_t)std::max(d, 1)), L((size_t)plan.NL);
        std::vector<long double> C((size_t)F * K), T((size_t)F * K), H((size_t)F * F);
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = b.live[(size_t)i];
            const double* h = out + (size_t)i * plan.NTOT;
            ll[p] = h[0];
            if (!std::isfinite(h[0])) continue;             // gradient and Hessian stay nan
            std::copy(h, h + plan.NL, L.begin());
            for (int s = 0; s < S; ++s) L[(size_t)(1 + s)] = h[1 + s] - 1.0;
            b.gradient(i, L.data(), rate_scale, grad + p * F, gz);
            fac_curv_hessian(b, i, L.data(), h + plan.NL, rate_scale, C, T, H, hess + p * F * F);
        }
    });
    return BI_OK;
}

}  // extern "C"
