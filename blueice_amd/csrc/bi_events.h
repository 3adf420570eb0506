// bi_events.h -- the event-level host path of the main translation unit (blueice_hip.hip includes it): scoring events at every
// anchor model (bi_score_events, bi_score_event_sets), drawing event-level toys (bi_simulate_events, bi_simulate_event_toys)
// and the event sets a context holds side by side.  What these entry points share exists once here: the walk over the axes of
// a binned space or lookup grid (also bi_set_analysis_space and bi_histogram_events), the rates at a parameter point (also
// bi_generate_toys), the simulators' way to device-resident pmf rows, and the lookup grid that scores what they drew.
// The kernels are in bi_k_misc.h.
#pragma once

namespace {

// ---- one walk over the axes ------------------------------------------------------------------------------------------------

// what an entry point calls its axes in bi_last_error
struct AxisWords {
    const char* with;       // "need 1..8 axes with ..."
    const char* few;        // an axis with too few values (format: the axis)
    const char* values;     // "... of axis 1 are not strictly ascending"
};
constexpr AxisWords kSpaceWords{"edges", "axis %d needs at least two edges", "bin edges"};
constexpr AxisWords kHistWords{"edges, and a counts buffer", "axis %d needs at least two edges", "bin edges"};
constexpr AxisWords kGridWords{"grid values", "axis %d needs at least two grid values", "grid values"};
constexpr AxisWords kSimWords{"bin edges", "axis %d has too few bin edges", "bin edges"};

struct AxisWalk {
    int k = 0;
    int flat = 0;                     // values of all axes together
    int64_t bins = 1;
    int n[kMaxDim] = {}, off[kMaxDim] = {};
    int64_t stride[kMaxDim] = {};     // bins (C order) per step along the axis
    // into the argument struct of a kernel (HistArgs, ScoreArgs, SimArgs: they stay as the kernels declare them)
    void put(int* n_out, int* off_out, int64_t* stride_out = nullptr) const {
        for (int i = 0; i < k; ++i) {
            n_out[i] = n[i];
            off_out[i] = off[i];
            if (stride_out) stride_out[i] = stride[i];
        }
    }
};

// values: the n[i] strictly ascending values of axis i, back to back.  min_n: the values every axis needs; centres: an axis of
// n values has n bins (the bin centres of a 'linear' lookup), not n - 1 (edges)
int walk_axes(bi_ctx* c, int k, const int32_t* n, const double* values, int min_n, bool centres, const AxisWords& w, AxisWalk& a) {
    if (k < 1 || k > kMaxDim || !n || !values) return fail(c, BI_ERR_INVALID, "need 1..%d axes with %s", kMaxDim, w.with);
    a = AxisWalk{};
    a.k = k;
    for (int i = 0; i < k; ++i) {
        if (n[i] < min_n) return fail(c, BI_ERR_INVALID, w.few, i);
        const double* x = values + a.flat;
        for (int j = 1; j < n[i]; ++j)
            if (!(x[j] > x[j - 1])) return fail(c, BI_ERR_INVALID, "%s of axis %d are not strictly ascending", w.values, i);
        a.n[i] = n[i];
        a.off[i] = a.flat;
        a.flat += n[i];
    }
    for (int i = k - 1; i >= 0; --i) {
        a.stride[i] = a.bins;
        a.bins *= centres ? n[i] : n[i] - 1;
    }
    return BI_OK;
}

// ---- rates at a point --------------------------------------------------------------------------------------------------------

// expected events per source of model `m` at (z, rate_scale) -- the scalar half of likelihood.py:355-393 -- which a generator
// needs in [0, inf); the message goes to `c`: "<where> point is outside the anchor box", "<what> needs rates in [0, inf)"
int rates_at(bi_ctx* c, const bi_ctx* m, const double* z, const double* rate_scale, const char* where, const char* what, PointGeom& g,
             std::vector<double>& r) {
    if (!point_geometry(m, z, g)) return fail(c, BI_ERR_INVALID, "%s point is outside the anchor box", where);
    r.assign((size_t)m->S, 0.0);
    interp_mus(m, g, r.data());
    if (rate_scale) for (int s = 0; s < m->S; ++s) r[(size_t)s] *= rate_scale[s];
    for (int s = 0; s < m->S; ++s)
        if (!(r[(size_t)s] >= 0.0 && r[(size_t)s] < std::numeric_limits<double>::infinity()))
            return fail(c, BI_ERR_INVALID, "%s needs rates in [0, inf)", what);
    return BI_OK;
}

// ---- scoring -------------------------------------------------------------------------------------------------------------------

// coords: host [k][N], or coords_dev: the same block already in HBM (bi_simulate_events)
// pad_cols (several event sets: the padding columns between them, which get 1.0 in every row): the events keep their order
int score_events_impl(bi_ctx* tp, bi_ctx* c, int method, int k, const int32_t* n_grid, const double* grid, int64_t N,
                      const double* coords, const double* coords_dev, double outlier_likelihood,
                      const std::vector<int64_t>* pad_cols = nullptr) {
    if (!c) return BI_ERR_INVALID;
    if (!tp || tp == c) return fail(c, BI_ERR_INVALID, "need a templates context different from the target");
    if (c->pending || tp->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding: call bi_eval_end first");
    if (!tp->model_ready) return fail(c, BI_ERR_STATE, "the templates context holds no model");
    if (tp->device != c->device) return fail(c, BI_ERR_INVALID, "templates and target live on different devices");
    if (tp->bb_source >= 0) return fail(c, BI_ERR_INVALID, "Beeston-Barlow applies to binned likelihoods only");
    if (method != 0 && method != 1) return fail(c, BI_ERR_INVALID, "method must be 0 (piecewise) or 1 (linear)");
    AxisWalk ax;
    int rc = walk_axes(c, k, n_grid, grid, 2, method == 1, kGridWords, ax);
    if (rc) return rc;
    if (N < 0 || (N > 0 && !coords && !coords_dev)) return fail(c, BI_ERR_INVALID, "bad N / coords");
    if (ax.bins != tp->B) return fail(c, BI_ERR_INVALID, "the grid describes %lld bins, the templates have %lld", (long long)ax.bins, (long long)tp->B);
    ScoreArgs a{};
    a.k = k;
    a.method = method;
    a.clip = coords_dev ? 1 : 0;          // events simulated on the device arrive unclipped; a caller's events are clipped already
    ax.put(a.n_grid, a.grid_off, a.stride);
    // the target becomes a model on the same anchor grid with one "bin" per event
    std::vector<int32_t> na(tp->n_anchor.begin(), tp->n_anchor.end());
    std::vector<double> az;
    for (int i = 0; i < tp->d; ++i) az.insert(az.end(), tp->grid[(size_t)i].begin(), tp->grid[(size_t)i].end());
    if ((rc = bi_model_begin(c, tp->d, na.data(), az.data(), tp->S, N, -1))) return rc;
    if (N > 0) {
        ScratchBuf d_ev, d_grid, d_base, d_t, d_keys, d_iota, d_tmp, d_pad;
        // events ordered by cell (see k_score_rows): from a few thousand events on, and while 32-bit positions do
        // (not with several event sets: a set is a range of columns)
        const bool sorted = !pad_cols && c->score_sorted && N >= 4096 && N < ((int64_t)1 << 31);
        if (pad_cols && !pad_cols->empty() && (rc = dev_upload(c, d_pad, *pad_cols))) return rc;
        size_t sort_bytes = 0;
        if (sorted) (void)prim_sort_pairs(nullptr, sort_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (const int32_t*)nullptr,
                                                    (int32_t*)nullptr, (size_t)N, 0u, 64u, c->stream);
        if ((!coords_dev && (rc = dev_alloc(c, d_ev, (size_t)N * k * sizeof(double)))) || (rc = dev_alloc(c, d_grid, (size_t)ax.flat * sizeof(double))) ||
            (rc = dev_alloc(c, d_base, (size_t)N * sizeof(int64_t))) || (method == 1 && (rc = dev_alloc(c, d_t, (size_t)N * k * sizeof(double)))) ||
            (sorted && ((rc = dev_alloc(c, d_keys, (size_t)N * sizeof(int64_t))) || (rc = dev_alloc(c, d_iota, (size_t)N * sizeof(int32_t))) ||
                        (rc = dev_alloc(c, d_tmp, std::max<size_t>(sort_bytes, 256))) || (rc = dev_alloc(c, c->ev_perm, (size_t)N * sizeof(int32_t))))))
            return rc;
        hipError_t e = coords_dev ? hipSuccess : hipMemcpyAsync(d_ev.p, coords, (size_t)N * k * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_grid.p, grid, (size_t)ax.flat * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tp->stream);            // whatever filled the templates is complete
        if (e == hipSuccess) {
            // every event's cell and weights once, then the gathers row by row: the row is the slow dimension of the grid, so
            // the chip works on one or two 8 MB histograms at a time (see k_score_rows)
            const int n_rows = (int)(tp->A * tp->S);
            hipLaunchKernelGGL(k_score_locate, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                               coords_dev ? coords_dev : (const double*)d_ev.p, N, a, (const double*)d_grid.p, (int64_t*)d_base.p, (double*)d_t.p);
            const int64_t* base_used = (const int64_t*)d_base.p;
            if (sorted) {
                hipLaunchKernelGGL(k_iota32, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, (int32_t*)d_iota.p, N);
                size_t tb = d_tmp.bytes;
                // (the cell index needs ceil(log2 B) bits: fewer radix passes than 64)
                unsigned bits = 1;
                while (bits < 63 && ((int64_t)1 << bits) < tp->B) ++bits;
                e = prim_sort_pairs(d_tmp.p, tb, (const int64_t*)d_base.p, (int64_t*)d_keys.p, (const int32_t*)d_iota.p,
                                              (int32_t*)c->ev_perm.p, (size_t)N, 0u, bits, c->stream);
                base_used = (const int64_t*)d_keys.p;
            }
            const int per_block = kThreads * score_events_per_thread(method == 0 ? 0 : k);
            const unsigned bx = (unsigned)((N + per_block - 1) / per_block);
#define BI_ROWS(K)                                                                                                 \
    hipLaunchKernelGGL((k_score_rows<K>), dim3(bx, (unsigned)std::min(n_rows, 65535)), dim3(kThreads), 0, c->stream, \
                       base_used, (const double*)d_t.p, N, a, (const double*)tp->ps.p, tp->Bp, n_rows, (double*)c->ps.p, c->Bp,        \
                       sorted ? (const int32_t*)c->ev_perm.p : (const int32_t*)nullptr)
            if (e == hipSuccess) switch (method == 0 ? 0 : k) {
                case 0: BI_ROWS(0); break; case 1: BI_ROWS(1); break; case 2: BI_ROWS(2); break; case 3: BI_ROWS(3); break;
                case 4: BI_ROWS(4); break; case 5: BI_ROWS(5); break; case 6: BI_ROWS(6); break; case 7: BI_ROWS(7); break;
                default: BI_ROWS(8); break;
            }
#undef BI_ROWS
            if (e == hipSuccess && pad_cols && !pad_cols->empty()) {
                const int64_t n_fill = (int64_t)n_rows * (int64_t)pad_cols->size();
                hipLaunchKernelGGL(k_fill_columns, dim3((unsigned)((n_fill + 255) / 256)), dim3(256), 0, c->stream, (double*)c->ps.p, c->Bp,
                                   (int64_t)n_rows, (const int64_t*)d_pad.p, (int64_t)pad_cols->size(), 1.0);
            }
            if (e == hipSuccess) e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);              // coords are borrowed for the call only
        else (void)hipStreamSynchronize(c->stream);
        c->ev_sorted = e == hipSuccess && sorted;
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_score_events: %s", hipGetErrorString(e));
    }                                                                          // (the scratch goes back before the model is closed)
    c->h_mus = tp->h_mus;
    std::fill(c->anchor_set.begin(), c->anchor_set.end(), 1);
    c->pk_skip = true;                 // (an event tensor: bi_set_unbinned below would drop a packed shadow at once)
    rc = bi_model_end(c);
    c->pk_skip = false;
    if (rc) return rc;
    c->allow_neg = tp->allow_neg;
    return bi_set_unbinned(c, outlier_likelihood);
}

// ---- simulation ----------------------------------------------------------------------------------------------------------------

// What both simulators need on the device before they draw: the bin edges, the rates at (z, rate_scale), and per source the
// pmf over the bins (the density morphed at z times the bin volume) with its running sums.  One struct, so that a simulator
// hands all of it back in one scope before the scoring pass allocates (dens and cdf are S x B doubles each).
struct SimSetup {
    SimArgs a{};
    // (the host side of the uploads: their copies are queued, not waited for, so it lives as long as the buffers)
    PointGeom g;
    std::vector<double> r, h_edges;
    std::vector<int64_t> rowoff;
    ScratchBuf row, w, edges, rates, dens, cdf, tmp;      // tmp: the temporary storage of the device-wide scans
};

// From the caller's arguments to SimSetup: the work is queued on c's stream, nothing has been waited for.  scan_items: the
// caller scans that many int64 with s.tmp itself (0: it does not); who: the entry point, for the message of a HIP error
int sim_setup(bi_ctx* tp, bi_ctx* c, const double* z, const double* rate_scale, int method, int k, const int32_t* n_edges,
              const double* edges, size_t scan_items, const char* who, SimSetup& s) {
    if (!c) return BI_ERR_INVALID;
    if (!tp || tp == c) return fail(c, BI_ERR_INVALID, "need a templates context different from the target");
    if (c->pending || tp->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding: call bi_eval_end first");
    if (!tp->model_ready) return fail(c, BI_ERR_STATE, "the templates context holds no model");
    if (tp->device != c->device) return fail(c, BI_ERR_INVALID, "templates and target live on different devices");
    if (method != 0 && method != 1) return fail(c, BI_ERR_INVALID, "method must be 0 (piecewise) or 1 (linear)");
    AxisWalk ax;
    int rc = walk_axes(c, k, n_edges, edges, method == 1 ? 3 : 2, false, kSimWords, ax);
    if (rc) return rc;
    if (tp->d > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    if (ax.bins != tp->B) return fail(c, BI_ERR_INVALID, "the edges describe %lld bins, the templates have %lld", (long long)ax.bins, (long long)tp->B);
    s.a.k = k; s.a.S = tp->S;
    ax.put(s.a.n_edges, s.a.edge_off, s.a.stride);
    HIP_TRY(c, hipSetDevice(c->device));
    // expected events per source at z, then N_s ~ Poisson
    PointGeom& g = s.g;
    std::vector<double>& r = s.r;
    if ((rc = rates_at(c, tp, z, rate_scale, "simulation", "event simulation", g, r))) return rc;
    const int S = tp->S;
    for (int q = 0; q < S; ++q)               // (N_s travels as a 32-bit int through the samplers: keep it far inside)
        if (r[(size_t)q] >= kSimMaxRate)
            return fail(c, BI_ERR_INVALID, "event simulation draws at most 2^30 expected events per source: source %d has %g", q, r[(size_t)q]);
    const int nc = (int)g.w.size();
    const int64_t B = tp->B;
    s.rowoff.assign((size_t)S * nc, 0);
    for (int q = 0; q < S; ++q)
        for (int corner = 0; corner < nc; ++corner)
            s.rowoff[(size_t)q * nc + corner] = ((g.cell_anchor + corner_offset(tp, corner)) * S + q) * tp->Bp;
    size_t scan_bytes = 0, scan2 = 0;
    (void)prim_inclusive_scan_sum(nullptr, scan_bytes, (const double*)nullptr, (double*)nullptr, (size_t)B, c->stream);
    if (scan_items) (void)prim_exclusive_scan_sum(nullptr, scan2, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, scan_items, c->stream);
    s.h_edges.assign(edges, edges + ax.flat);
    if ((rc = dev_upload(c, s.row, s.rowoff)) || (rc = dev_upload(c, s.w, g.w)) || (rc = dev_upload(c, s.edges, s.h_edges)) ||
        (rc = dev_upload(c, s.rates, r)) || (rc = dev_alloc(c, s.dens, (size_t)S * B * sizeof(double))) ||
        (rc = dev_alloc(c, s.cdf, (size_t)S * B * sizeof(double))) ||
        (rc = dev_alloc(c, s.tmp, std::max<size_t>(std::max(scan_bytes, scan2), 256)))) return rc;
    hipError_t e = hipStreamSynchronize(tp->stream);                      // whatever filled the templates is complete
    if (e == hipSuccess) {                                                // the pmf rows and their running sums: once per call
        hipLaunchKernelGGL(k_morph_store, dim3((unsigned)((B + kThreads - 1) / kThreads), (unsigned)S), dim3(kThreads), 0, c->stream,
                           (const double*)tp->ps.p, (const int64_t*)s.row.p, (const double*)s.w.p, nc, B, (double*)s.dens.p);
        hipLaunchKernelGGL(k_sim_pmf, dim3((unsigned)((B + kThreads - 1) / kThreads), (unsigned)S), dim3(kThreads), 0, c->stream,
                           (const double*)s.dens.p, s.a, (const double*)s.edges.p, B, (double*)s.dens.p);
        e = hipGetLastError();
    }
    for (int q = 0; e == hipSuccess && q < S; ++q) {
        size_t tb = s.tmp.bytes;
        e = prim_inclusive_scan_sum(s.tmp.p, tb, (const double*)s.dens.p + (size_t)q * B, (double*)s.cdf.p + (size_t)q * B, (size_t)B, c->stream);
    }
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return BI_OK;
}

// the grid of the lookup that scores simulated events at every anchor model: the edges ('piecewise') or the bin centres ('linear')
void lookup_grid(int method, int k, const int32_t* n_edges, const double* edges, std::vector<int32_t>& n_grid, std::vector<double>& grid) {
    n_grid.assign((size_t)k, 0);
    grid.clear();
    int eo = 0;
    for (int i = 0; i < k; ++i) {
        if (method == 0) {
            n_grid[(size_t)i] = n_edges[i];
            grid.insert(grid.end(), edges + eo, edges + eo + n_edges[i]);
        } else {
            n_grid[(size_t)i] = n_edges[i] - 1;
            for (int j = 0; j + 1 < n_edges[i]; ++j) grid.push_back(0.5 * (edges[eo + j] + edges[eo + j + 1]));
        }
        eo += n_edges[i];
    }
}

// ---- event sets ------------------------------------------------------------------------------------------------------------------

// the target of a scoring call over `cols` columns becomes a context of T event sets: set t at [first[t], first[t] + n[t])
void adopt_event_sets(bi_ctx* c, const std::vector<int64_t>& first, const std::vector<int64_t>& n) {
    const int64_t T = (int64_t)n.size();
    c->n_sets = T;
    c->set_first.assign(first.begin(), first.begin() + T);
    c->set_n = n;
    c->T = T;
    c->h_lgsum.assign((size_t)T, 0.0);
    c->B = n[0];              // (see bi_context.h: whatever knows nothing of sets evaluates set 0)
    ++c->epoch;
}

// set_first [T + 1] of sets with n[t] events each (even starts), and the padding columns
void layout_event_sets(const std::vector<int64_t>& n, std::vector<int64_t>& first, std::vector<int64_t>& pads) {
    first.assign(n.size() + 1, 0);
    pads.clear();
    for (size_t t = 0; t < n.size(); ++t) {
        first[t + 1] = (first[t] + n[t] + 1) & ~(int64_t)1;
        if (n[t] & 1) pads.push_back(first[t] + n[t]);
    }
}

}  // namespace

extern "C" {

int bi_score_events(bi_ctx* tp, bi_ctx* c, int method, int k, const int32_t* n_grid, const double* grid, int64_t N,
                    const double* coords, double outlier_likelihood) {
    return score_events_impl(tp, c, method, k, n_grid, grid, N, coords, nullptr, outlier_likelihood);
}

int bi_simulate_events(bi_ctx* tp, bi_ctx* c, const double* z, const double* rate_scale, int method, int k, const int32_t* n_edges,
                       const double* edges, uint64_t seed, double outlier_likelihood, int64_t* n_per_source) {
    int64_t N = 0;
    {
        SimSetup s;           // (handed back at the end of this scope: the scoring pass below can reuse the memory)
        int rc = sim_setup(tp, c, z, rate_scale, method, k, n_edges, edges, 0, "bi_simulate_events", s);
        if (rc) return rc;
        const int S = tp->S;
        ScratchBuf d_n, d_first;
        if ((rc = dev_alloc(c, d_n, (size_t)S * sizeof(int64_t)))) return rc;
        std::vector<int64_t> n_s((size_t)S, 0);
        hipLaunchKernelGGL(k_sim_counts, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, c->stream, (const double*)s.rates.p, S, seed, (int64_t*)d_n.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(n_s.data(), d_n.p, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_simulate_events: %s", hipGetErrorString(e));
        std::vector<int64_t> first((size_t)S + 1, 0);
        for (int q = 0; q < S; ++q) first[(size_t)q + 1] = first[(size_t)q] + n_s[(size_t)q];
        N = first[(size_t)S];
        if (n_per_source) std::copy(n_s.begin(), n_s.end(), n_per_source);
        // the events themselves: coordinates [k][N] and the source of every event, kept with the target for bi_download_events
        if ((rc = dev_alloc(c, c->sim_coords, (size_t)std::max<int64_t>(N, 1) * k * sizeof(double))) ||
            (rc = dev_alloc(c, c->sim_source, (size_t)std::max<int64_t>(N, 1) * sizeof(int32_t))) || (rc = dev_upload(c, d_first, first))) return rc;
        c->sim_k = k;
        c->sim_n = N;
        c->sim_cols = -1;
        if (N > 0) {
            hipLaunchKernelGGL(k_sim_events, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, (const double*)s.cdf.p, tp->B,
                               s.a, (const double*)s.edges.p, (const int64_t*)d_first.p, seed, N, (double*)c->sim_coords.p, (int32_t*)c->sim_source.p);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_simulate_events: %s", hipGetErrorString(e));
    }
    // score them at every anchor model (bi_model_begin inside re-allocates the target's model, not the sim_* buffers)
    std::vector<int32_t> n_grid;
    std::vector<double> grid;
    lookup_grid(method, k, n_edges, edges, n_grid, grid);
    return score_events_impl(tp, c, method, k, n_grid.data(), grid.data(), N, nullptr, (const double*)c->sim_coords.p, outlier_likelihood);
}

int bi_download_events(bi_ctx* c, double* coords, int32_t* source) {
    if (!c) return BI_ERR_INVALID;
    if (c->sim_n < 0) return fail(c, BI_ERR_STATE, "no simulated events are resident (bi_simulate_events first)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->sim_cols >= 0) {            // an ensemble (bi_simulate_event_toys): the columns without the padding between the sets
        if (!multi_set(c) || c->sim_epoch != c->epoch || c->sim_n == 0) return c->sim_n == 0 ? BI_OK : fail(c, BI_ERR_STATE, "the simulated ensemble is no longer the context's data");
        std::vector<double> hc(coords ? (size_t)c->sim_cols * c->sim_k : 0);
        std::vector<int32_t> hs(source ? (size_t)c->sim_cols : 0);
        if (coords) HIP_TRY(c, hipMemcpyAsync(hc.data(), c->sim_coords.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (source) HIP_TRY(c, hipMemcpyAsync(hs.data(), c->sim_source.p, hs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int64_t at = 0;
        for (int64_t t = 0; t < c->n_sets; ++t) {
            const int64_t f = c->set_first[(size_t)t], n = c->set_n[(size_t)t];
            for (int ax = 0; coords && ax < c->sim_k; ++ax)
                std::copy(hc.begin() + (size_t)ax * c->sim_cols + f, hc.begin() + (size_t)ax * c->sim_cols + f + n, coords + (size_t)ax * c->sim_n + at);
            if (source) std::copy(hs.begin() + f, hs.begin() + f + n, source + at);
            at += n;
        }
        return BI_OK;
    }
    if (c->sim_n > 0 && coords)
        HIP_TRY(c, hipMemcpyAsync(coords, c->sim_coords.p, (size_t)c->sim_n * c->sim_k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (c->sim_n > 0 && source)
        HIP_TRY(c, hipMemcpyAsync(source, c->sim_source.p, (size_t)c->sim_n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

int64_t bi_simulated_event_count(const bi_ctx* c) { return c ? c->sim_n : -1; }

int bi_score_event_sets(bi_ctx* tp, bi_ctx* c, int method, int k, const int32_t* n_grid, const double* grid, int64_t T,
                        const int64_t* offsets, const double* coords, double outlier_likelihood) {
    if (!c) return BI_ERR_INVALID;
    if (T < 1 || !offsets) return fail(c, BI_ERR_INVALID, "need T >= 1 event sets and their offsets");
    if (offsets[0] != 0) return fail(c, BI_ERR_INVALID, "offsets[0] must be 0");
    for (int64_t t = 0; t < T; ++t)
        if (offsets[t + 1] < offsets[t]) return fail(c, BI_ERR_INVALID, "offsets are not ascending at set %lld", (long long)t);
    const int64_t N = offsets[T];
    if (T == 1) return score_events_impl(tp, c, method, k, n_grid, grid, N, coords, nullptr, outlier_likelihood);
    AxisWalk ax;              // (before the padding below reads the first grid value of every axis; scoring walks them again)
    int rc = walk_axes(c, k, n_grid, grid, 2, method == 1, kGridWords, ax);
    if (rc) return rc;
    if (N > 0 && !coords) return fail(c, BI_ERR_INVALID, "bad N / coords");
    std::vector<int64_t> n((size_t)T), first, pads;
    for (int64_t t = 0; t < T; ++t) n[(size_t)t] = offsets[t + 1] - offsets[t];
    layout_event_sets(n, first, pads);
    const int64_t cols = first[(size_t)T];
    // the caller's events at their columns; a padding column scores at the first grid value of every axis (and is then set to 1)
    std::vector<double> padded((size_t)cols * k);
    for (int i = 0; i < k; ++i) {
        double* row = padded.data() + (size_t)i * cols;
        std::fill(row, row + cols, grid[ax.off[i]]);
        for (int64_t t = 0; t < T; ++t)
            std::copy(coords + (size_t)i * N + offsets[t], coords + (size_t)i * N + offsets[t + 1], row + first[(size_t)t]);
    }
    if ((rc = score_events_impl(tp, c, method, k, n_grid, grid, cols, padded.data(), nullptr, outlier_likelihood, &pads))) return rc;
    adopt_event_sets(c, first, n);
    return BI_OK;
}

int bi_simulate_event_toys(bi_ctx* tp, bi_ctx* c, const double* z, const double* rate_scale, int method, int k, const int32_t* n_edges,
                           const double* edges, int64_t T, uint64_t seed, double outlier_likelihood, int64_t* n_per_toy_source) {
    if (!c) return BI_ERR_INVALID;
    if (T < 1 || T > ((int64_t)1 << 40)) return fail(c, BI_ERR_INVALID, "need T >= 1 toys");
    const int64_t toy0 = c->toy_offset;
    if (toy0 + T > ((int64_t)1 << 48)) return fail(c, BI_ERR_INVALID, "toy numbers are told apart up to 2^48");
    if (T == 1)               // (one set: the single toy's layout, through its call)
        return bi_simulate_events(tp, c, z, rate_scale, method, k, n_edges, edges, toy_seed(seed, (uint64_t)toy0), outlier_likelihood, n_per_toy_source);
    std::vector<int64_t> n_t((size_t)T, 0), set_first((size_t)T + 1, 0), pads;
    int64_t cols = 0;
    {
        SimSetup s;           // (handed back at the end of this scope: the scoring pass below can reuse the memory)
        int rc = sim_setup(tp, c, z, rate_scale, method, k, n_edges, edges, (size_t)(T + 1), "bi_simulate_event_toys", s);
        if (rc) return rc;
        const int S = tp->S;
        ScratchBuf d_n, d_room, d_setfirst, d_first;
        if ((rc = dev_alloc(c, d_n, (size_t)T * S * sizeof(int64_t))) || (rc = dev_alloc(c, d_room, (size_t)(T + 1) * sizeof(int64_t))) ||
            (rc = dev_alloc(c, d_setfirst, (size_t)(T + 1) * sizeof(int64_t))) || (rc = dev_alloc(c, d_first, (size_t)T * (S + 1) * sizeof(int64_t)))) return rc;
        // counts of all (t, s), the columns every toy takes, their prefix sum, the start of every (t, s): four small launches
        std::vector<int64_t> n_ts((size_t)T * S, 0);
        hipLaunchKernelGGL(k_sim_toy_counts, dim3((unsigned)((T * S + 255) / 256)), dim3(256), 0, c->stream, (const double*)s.rates.p, S, T, seed,
                           toy0, (int64_t*)d_n.p);
        hipLaunchKernelGGL(k_sim_toy_room, dim3((unsigned)((T + 1 + 255) / 256)), dim3(256), 0, c->stream, (const int64_t*)d_n.p, S, T, (int64_t*)d_room.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            size_t tb = s.tmp.bytes;
            e = prim_exclusive_scan_sum(s.tmp.p, tb, (const int64_t*)d_room.p, (int64_t*)d_setfirst.p, (int64_t)0, (size_t)(T + 1), c->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_sim_toy_first, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, c->stream, (const int64_t*)d_n.p,
                               (const int64_t*)d_setfirst.p, S, T, (int64_t*)d_first.p);
            e = hipGetLastError();
        }
        // the one read-back: the counts (they size the tensor and are what the caller asked for) and the set boundaries
        if (e == hipSuccess) e = hipMemcpyAsync(n_ts.data(), d_n.p, n_ts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(set_first.data(), d_setfirst.p, set_first.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_simulate_event_toys: %s", hipGetErrorString(e));
        if (n_per_toy_source) std::copy(n_ts.begin(), n_ts.end(), n_per_toy_source);
        std::vector<int64_t> first_chk;
        int64_t n_events = 0;
        for (int64_t t = 0; t < T; ++t) {
            for (int q = 0; q < S; ++q) n_t[(size_t)t] += n_ts[(size_t)(t * S + q)];
            n_events += n_t[(size_t)t];
        }
        layout_event_sets(n_t, first_chk, pads);
        if (first_chk != set_first) return fail(c, BI_ERR_HIP, "bi_simulate_event_toys: the device's set boundaries are not the counts' prefix sums");
        cols = set_first[(size_t)T];
        if ((rc = dev_alloc(c, c->sim_coords, (size_t)std::max<int64_t>(cols, 1) * k * sizeof(double))) ||
            (rc = dev_alloc(c, c->sim_source, (size_t)std::max<int64_t>(cols, 1) * sizeof(int32_t)))) return rc;
        c->sim_k = k;
        c->sim_n = n_events;
        c->sim_cols = cols;
        if (cols > 0) {
            hipLaunchKernelGGL(k_sim_toy_events, dim3((unsigned)((cols + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, (const double*)s.cdf.p, tp->B,
                               s.a, (const double*)s.edges.p, (const int64_t*)d_setfirst.p, (const int64_t*)d_first.p, T, seed, toy0, cols,
                               (double*)c->sim_coords.p, (int32_t*)c->sim_source.p);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_simulate_event_toys: %s", hipGetErrorString(e));
    }
    std::vector<int32_t> n_grid;
    std::vector<double> grid;
    lookup_grid(method, k, n_edges, edges, n_grid, grid);
    const int rc = score_events_impl(tp, c, method, k, n_grid.data(), grid.data(), cols, nullptr, (const double*)c->sim_coords.p, outlier_likelihood, &pads);
    if (rc) return rc;
    adopt_event_sets(c, set_first, n_t);
    c->sim_epoch = c->epoch;
    return BI_OK;
}

int bi_event_set_offsets(bi_ctx* c, int64_t* offsets) {
    if (!c || !offsets) return BI_ERR_INVALID;
    if (!c->unbinned || !c->data_ready) return fail(c, BI_ERR_STATE, "the context holds no unbinned data");
    for (int64_t t = 0; t < c->n_sets; ++t) offsets[t] = c->set_first[(size_t)t];
    const int64_t end = c->set_first[(size_t)c->n_sets - 1] + c->set_n[(size_t)c->n_sets - 1];
    offsets[c->n_sets] = c->n_sets > 1 ? ((end + 1) & ~(int64_t)1) : end;
    return BI_OK;
}

int bi_event_set_counts(bi_ctx* c, int64_t* counts) {
    if (!c || !counts) return BI_ERR_INVALID;
    if (!c->unbinned || !c->data_ready) return fail(c, BI_ERR_STATE, "the context holds no unbinned data");
    std::copy(c->set_n.begin(), c->set_n.end(), counts);
    return BI_OK;
}

int64_t bi_event_set_count(const bi_ctx* c) { return (c && c->unbinned && c->data_ready) ? c->n_sets : 0; }

int bi_set_event_sets(bi_ctx* c, int64_t T, const int64_t* counts) {
    if (!c) return BI_ERR_INVALID;
    if (!c->unbinned || !c->data_ready || c->n_sets != 1) return fail(c, BI_ERR_STATE, "bi_set_event_sets follows bi_set_unbinned");
    if (T < 1 || !counts) return fail(c, BI_ERR_INVALID, "need T >= 1 event sets and their counts");
    if (c->ev_sorted) return fail(c, BI_ERR_STATE, "the columns are ordered by histogram cell (score_sorted)");
    std::vector<int64_t> n(counts, counts + T), first, pads;
    for (int64_t t = 0; t < T; ++t)
        if (n[(size_t)t] < 0) return fail(c, BI_ERR_INVALID, "event set %lld has a negative count", (long long)t);
    if (T == 1) return n[0] == c->B ? BI_OK : fail(c, BI_ERR_INVALID, "one set of %lld events, the model has %lld columns", (long long)n[0], (long long)c->B);
    layout_event_sets(n, first, pads);
    if (first[(size_t)T] != c->B)
        return fail(c, BI_ERR_INVALID, "the sets take %lld columns (even starts), the model has %lld", (long long)first[(size_t)T], (long long)c->B);
    adopt_event_sets(c, first, n);
    return BI_OK;
}

int bi_download_event_set(bi_ctx* c, int64_t t, double* out) {
    if (!c) return BI_ERR_INVALID;
    if (!c->unbinned || !c->data_ready) return fail(c, BI_ERR_STATE, "the context holds no unbinned data");
    if (t < 0 || t >= c->n_sets) return fail(c, BI_ERR_INVALID, "event set %lld outside [0, %lld)", (long long)t, (long long)c->n_sets);
    if (c->ev_sorted) return fail(c, BI_ERR_STATE, "the columns are ordered by histogram cell (score_sorted): bi_interpolate hands them back in event order");
    const int64_t n = c->set_n[(size_t)t];
    if (n == 0) return BI_OK;
    if (!out) return fail(c, BI_ERR_INVALID, "out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)n * sizeof(double), (const double*)c->ps.p + c->set_first[(size_t)t], (size_t)c->Bp * sizeof(double),
                                (size_t)n * sizeof(double), (size_t)(c->A * c->S), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

}  // extern "C"
