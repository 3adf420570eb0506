// bi_sourcewise_sim.h -- source-wise models: event-level toys drawn on the device and scored into the event store (host half; the
// kernels are bi_k_sourcewise_sim.h's, translation unit tu_sourcewise_sim.hip).  bi_sourcewise_simulate_event_toys,
// bi_sourcewise_simulated_event_count, bi_sourcewise_download_events.
//
// One call draws T = sum n_toys[h] toys at H truths, truth-major, in bi_simulate_event_toys' stream (include/blueice_hip.h), and
// they become the context's T event sets in the layout of bi_sourcewise_events.h:
//   1. screen, fill and upload of the truths: FacBatch of order 0 (bi_factored.h), whose rates are r_s = M_s(z_h) rs_s;
//   2. the counts of all (t, s), the room of every toy (whole tiles, at least one), the exclusive scan, the per-(t, s) starts;
//      ONE read-back of the counts and the set boundaries, checked against events_layout (which also holds compact_budget);
//   3. truths in sub-batches of kSimScratchBytes (or the parameter sim_truth_chunk): k_sourcewise_pmf writes the sub-batch's pmf
//      rows [truth][s][B], prim_inclusive_scan_sum their running sums row by row, and k_sourcewise_sim_events draws the columns
//      of the sub-batch's toys -- a contiguous range, because toys are truth-major;
//   4. the store: events_create, then events_score_columns on the coordinates where they lie (clip = 1: a 'linear' lookup clips
//      when it scores; the stored positions stay as drawn).
// Everything is validated before step 4, which is the first to touch the previous store; after a device error the context holds
// no store.  The coordinates and sources stay with the store (bi_ctx::Factored::sim_*) until it is released or replaced.
#pragma once

namespace {

constexpr size_t kSimScratchBytes = (size_t)256 << 20;     // pmf + cdf rows of one sub-batch of truths (16 S B bytes per truth)

// profiling: the device time of the call's four parts -- 0 counts + layout, 1 pmf rows + running sums, 2 the event kernel, 3 scoring
// -- from the scopes it opened (read-only parameters sim_ns_layout, sim_ns_pmf, sim_ns_events, sim_ns_score); zeros when profiling is off
void sim_part_times(bi_ctx* c, size_t scope0, const std::vector<int>& part) {
    for (int64_t& ns : c->sim_part_ns) ns = 0;
    if (!c->profiling) return;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return;
    for (size_t i = 0; i < part.size() && scope0 + i < c->ev_used; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, c->ev_pool[scope0 + i].first, c->ev_pool[scope0 + i].second) == hipSuccess)
            c->sim_part_ns[part[i]] += (int64_t)((double)t * 1e6);
    }
}

int sourcewise_simulate_event_toys(bi_ctx* c, int method, int k, const int32_t* n_edges, const double* edges, int64_t H, const double* z,
                                   const double* rate_scale, const int64_t* n_toys, uint64_t seed, double outlier, int64_t* n_per_toy_source) {
    const char* who = "bi_sourcewise_simulate_event_toys";
    bi_ctx::Factored& m = c->fac;
    if (method != 0 && method != 1) return fail(c, BI_ERR_INVALID, "%s: method must be 0 (piecewise) or 1 (linear)", who);
    AxisWalk ax, gax;
    int rc = walk_axes(c, k, n_edges, edges, method == 1 ? 3 : 2, false, kSimWords, ax);
    if (rc) return rc;
    if (ax.bins != m.B)
        return fail(c, BI_ERR_INVALID, "%s: the edges describe %lld bins, the model's rows have %lld", who, (long long)ax.bins, (long long)m.B);
    if (!(outlier >= 0.0 && outlier < std::numeric_limits<double>::infinity()))
        return fail(c, BI_ERR_INVALID, "%s: outlier_likelihood = %g outside [0, inf)", who, outlier);
    if (H < 1 || !n_toys) return fail(c, BI_ERR_INVALID, "%s: need H >= 1 truth points and their numbers of toys", who);
    int64_t T = 0;
    for (int64_t h = 0; h < H; ++h) {
        if (n_toys[h] < 0) return fail(c, BI_ERR_INVALID, "%s: n_toys[%lld] = %lld is negative", who, (long long)h, (long long)n_toys[h]);
        if (n_toys[h] > INT32_MAX - T) return fail(c, BI_ERR_INVALID, "%s: a call draws fewer than 2^31 toys", who);
        T += n_toys[h];
    }
    if (T < 1) return fail(c, BI_ERR_INVALID, "%s: need T >= 1 toys", who);
    const int64_t toy0 = c->toy_offset;
    if (toy0 + T > ((int64_t)1 << 48)) return fail(c, BI_ERR_INVALID, "%s: toy numbers are told apart up to 2^48", who);
    if (m.d > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    HIP_TRY(c, hipSetDevice(c->device));

    // every truth before anything is drawn: the box, the rates
    FacBatch b(c, 0, false);
    const int S = b.S;
    std::vector<int32_t> st((size_t)H, 0);
    b.screen(H, z, rate_scale, nullptr, st.data(), [](int64_t) {});
    for (int64_t h = 0; h < H; ++h) {
        if (st[(size_t)h] & BI_ST_OUT_OF_BOUNDS) return fail(c, BI_ERR_INVALID, "%s (truth %lld): point is outside the anchor box", who, (long long)h);
        if (st[(size_t)h]) return fail(c, BI_ERR_INVALID, "%s (truth %lld): a rate is outside [0, inf)", who, (long long)h);
    }
    b.fill(z, rate_scale, nullptr);
    for (int64_t h = 0; h < H; ++h)
        for (int s = 0; s < S; ++s)               // (N_s travels as a 32-bit int through the samplers: keep it far inside)
            if (b.rates[(size_t)(h * b.SC + s)] >= kSimMaxRate)
                return fail(c, BI_ERR_INVALID, "%s (truth %lld): event simulation draws at most 2^30 expected events per source: source %d has %g", who,
                            (long long)h, s, b.rates[(size_t)(h * b.SC + s)]);
    std::vector<int32_t> n_grid;
    std::vector<double> grid;
    lookup_grid(method, k, n_edges, edges, n_grid, grid);
    if ((rc = walk_axes(c, k, n_grid.data(), grid.data(), 2, method == 1, kGridWords, gax))) return rc;

    std::vector<int32_t> truth((size_t)T);
    std::vector<int64_t> first_toy((size_t)H + 1, 0);
    for (int64_t h = 0, t = 0; h < H; ++h) {
        for (int64_t j = 0; j < n_toys[h]; ++j, ++t) truth[(size_t)t] = (int32_t)h;
        first_toy[(size_t)h + 1] = t;
    }
    const std::vector<double> h_edges(edges, edges + ax.flat);
    if ((rc = b.upload({{truth.data(), truth.size() * sizeof(int32_t)}, {h_edges.data(), h_edges.size() * sizeof(double)}}, 0))) return rc;

    const int64_t B = m.B;
    SourcewiseSimArgs a{};
    a.sim.k = k;
    a.sim.S = S;
    ax.put(a.sim.n_edges, a.sim.edge_off, a.sim.stride);
    a.edges = b.pu.dev<double>(b.first_extra + 1);
    a.rates = b.pu.dev<double>(2);
    a.rate_stride = b.SC;
    a.truth = b.pu.dev<int32_t>(b.first_extra);
    a.T = T;
    a.toy0 = toy0;
    a.seed = seed;
    a.B = B;

    // the truths of a sub-batch: what the scratch bound holds, or what the caller forces
    const size_t per_truth = (size_t)16 * (size_t)S * (size_t)B;
    int64_t chunk = c->sim_truth_chunk > 0 ? c->sim_truth_chunk : (int64_t)std::max<size_t>(1, kSimScratchBytes / per_truth);
    chunk = std::min(std::min(chunk, H), kSwLaunchItems);

    size_t scan_bytes = 0, scan2 = 0;
    (void)prim_inclusive_scan_sum(nullptr, scan_bytes, (const double*)nullptr, (double*)nullptr, (size_t)B, c->stream);
    (void)prim_exclusive_scan_sum(nullptr, scan2, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(T + 1), c->stream);
    ScratchBuf d_n, d_room, d_setfirst, d_first, d_tmp, d_pmf, d_cdf;
    DevBuf coords, source;                       // they become the store's once it stands
    auto give_up = [&](int code) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(coords);
        dev_free(source);
        return code;
    };
    if ((rc = dev_alloc(c, d_n, (size_t)T * S * sizeof(int64_t))) || (rc = dev_alloc(c, d_room, (size_t)(T + 1) * sizeof(int64_t))) ||
        (rc = dev_alloc(c, d_setfirst, (size_t)(T + 1) * sizeof(int64_t))) || (rc = dev_alloc(c, d_first, (size_t)T * (S + 1) * sizeof(int64_t))) ||
        (rc = dev_alloc(c, d_tmp, std::max<size_t>(std::max(scan_bytes, scan2), 256))))
        return give_up(rc);
    a.n = (int64_t*)d_n.p;
    a.room = (int64_t*)d_room.p;
    a.set_first = (const int64_t*)d_setfirst.p;
    a.first = (int64_t*)d_first.p;

    // counts of all (t, s), the room of every toy, their prefix sums, the start of every (t, s); then the one read-back: the counts
    // (they size the store and are what the caller asked for) and the set boundaries
    std::vector<int64_t> n_ts((size_t)T * S, 0), set_first((size_t)T + 1, 0), n_t((size_t)T, 0), first_chk;
    hipError_t e;
    const size_t scope0 = c->ev_used;            // (profiling: the scopes of this call in order, and the part each belongs to)
    std::vector<int> part;
    {
        EventScope ev(c);
        part.push_back(0);
        launch_sourcewise_sim_counts(c, a);
        launch_sourcewise_sim_room(c, a);
        e = hipGetLastError();
        if (e == hipSuccess) {
            size_t tb = d_tmp.bytes;
            e = prim_exclusive_scan_sum(d_tmp.p, tb, (const int64_t*)d_room.p, (int64_t*)d_setfirst.p, (int64_t)0, (size_t)(T + 1), c->stream);
        }
        if (e == hipSuccess) {
            launch_sourcewise_sim_first(c, a);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(n_ts.data(), d_n.p, n_ts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(set_first.data(), d_setfirst.p, set_first.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return give_up(fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e)));
    int64_t n_events = 0, cols = 0;
    for (int64_t t = 0; t < T; ++t) {
        for (int s = 0; s < S; ++s) n_t[(size_t)t] += n_ts[(size_t)(t * S + s)];
        n_events += n_t[(size_t)t];
    }
    if ((rc = events_layout(c, who, T, n_t.data(), first_chk, cols))) return give_up(rc);      // (compact_budget: nothing is built)
    first_chk.push_back(cols);
    if (first_chk != set_first) return give_up(fail(c, BI_ERR_HIP, "%s: the device's set boundaries are not the layout of the counts", who));

    // the events: pmf rows, running sums and the columns of the toys, one sub-batch of truths after the other
    if ((rc = dev_alloc(c, coords, (size_t)cols * k * sizeof(double))) || (rc = dev_alloc(c, source, (size_t)cols * sizeof(int32_t))) ||
        (rc = dev_alloc(c, d_pmf, (size_t)chunk * per_truth / 2)) || (rc = dev_alloc(c, d_cdf, (size_t)chunk * per_truth / 2)))
        return give_up(rc);
    a.cdf = (const double*)d_cdf.p;
    a.cols = cols;
    a.coords = (double*)coords.p;
    a.source = (int32_t*)source.p;
    SourcewisePmfArgs pa{};
    pa.sim = a.sim;
    pa.edges = a.edges;
    pa.out = (double*)d_pmf.p;
    pa.B = B;
    for (int64_t h0 = 0; h0 < H && e == hipSuccess; h0 += chunk) {
        const int64_t nh = std::min(chunk, H - h0);
        const int64_t t0 = first_toy[(size_t)h0], t1 = first_toy[(size_t)(h0 + nh)];
        if (t1 == t0) continue;                  // (truths without toys)
        {
            EventScope ev(c);
            part.push_back(1);
            pa.f = b.args();
            b.point_at(pa.f, h0);
            const int bad = launch_sourcewise_pmf(c, b.SC, b.EM, pa, nh);
            if (bad) return give_up(fail(c, bad, "%s: no kernel variant for %d source slots with %d own axes", who, b.SC, b.EM));
            e = hipGetLastError();
            for (int64_t r = 0; r < nh * S && e == hipSuccess; ++r) {
                size_t tb = d_tmp.bytes;
                e = prim_inclusive_scan_sum(d_tmp.p, tb, (const double*)d_pmf.p + (size_t)r * B, (double*)d_cdf.p + (size_t)r * B, (size_t)B, c->stream);
            }
        }
        if (e != hipSuccess) break;
        EventScope ev(c);
        part.push_back(2);
        a.t0 = t0;
        a.nt = t1 - t0;
        a.h0 = h0;
        a.col0 = set_first[(size_t)t0];
        a.ncols = set_first[(size_t)t1] - a.col0;
        launch_sourcewise_sim_events(c, a);
        e = hipGetLastError();
        ++c->last_point_pieces;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return give_up(fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e)));
    dev_free(d_pmf);                             // (the scoring pass below can reuse the memory)
    dev_free(d_cdf);

    // the store: from here on the previous one is gone
    if ((rc = events_create(c, who, T, n_t.data(), outlier))) return give_up(rc);
    if (n_events > 0) {
        EventScope ev(c);
        part.push_back(3);
        if ((rc = events_score_columns(c, who, method, k, gax, grid.data(), (const double*)coords.p, 1))) return give_up(rc);
    }
    sim_part_times(c, scope0, part);
    if ((rc = events_close(c, who))) return give_up(rc);
    m.sim_coords = coords;
    m.sim_source = source;
    m.sim_k = k;
    m.sim_n = n_events;
    if (n_per_toy_source) std::copy(n_ts.begin(), n_ts.end(), n_per_toy_source);
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_sourcewise_simulate_event_toys(bi_ctx* c, int method, int k, const int32_t* n_edges, const double* edges, int64_t H, const double* z,
                                      const double* rate_scale, const int64_t* n_toys, uint64_t seed, double outlier_likelihood,
                                      int64_t* n_per_toy_source) {
    int rc = fac_check(c, "bi_sourcewise_simulate_event_toys", false, true);
    if (rc) return rc;
    try {
        return sourcewise_simulate_event_toys(c, method, k, n_edges, edges, H, z, rate_scale, n_toys, seed, outlier_likelihood, n_per_toy_source);
    } catch (const std::bad_alloc&) {
        (void)hipStreamSynchronize(c->stream);
        return fail(c, BI_ERR_NOMEM, "bi_sourcewise_simulate_event_toys: out of host memory");
    }
}

int64_t bi_sourcewise_simulated_event_count(const bi_ctx* c) { return c ? c->fac.sim_n : -1; }

int bi_sourcewise_download_events(bi_ctx* c, double* coords, int32_t* source) {
    const char* who = "bi_sourcewise_download_events";
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    const bi_ctx::Factored& m = c->fac;
    if (!m.ev_ready || m.sim_n < 0)
        return fail(c, BI_ERR_STATE, "%s: the context's event store holds no simulated events (bi_sourcewise_simulate_event_toys first; another "
                    "store has replaced them since)", who);
    if (m.sim_n == 0) return BI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the columns without the padding behind the sets
    const int64_t cols = m.ev_cols, N = m.sim_n;
    try {
        std::vector<double> hc(coords ? (size_t)cols * m.sim_k : 0);
        std::vector<int32_t> hs(source ? (size_t)cols : 0);
        if (coords) HIP_TRY(c, hipMemcpyAsync(hc.data(), m.sim_coords.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (source) HIP_TRY(c, hipMemcpyAsync(hs.data(), m.sim_source.p, hs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int64_t at = 0;
        for (int64_t t = 0; t < m.ev_T; ++t) {
            const int64_t f = m.ev_first[(size_t)t], n = m.ev_n[(size_t)t];
            for (int i = 0; coords && i < m.sim_k; ++i)
                std::copy(hc.begin() + (size_t)i * cols + f, hc.begin() + (size_t)i * cols + f + n, coords + (size_t)i * N + at);
            if (source) std::copy(hs.begin() + f, hs.begin() + f + n, source + at);
            at += n;
        }
    } catch (const std::bad_alloc&) {
        (void)hipStreamSynchronize(c->stream);
        return fail(c, BI_ERR_NOMEM, "%s: out of host memory", who);
    }
    return BI_OK;
}

}  // extern "C"
