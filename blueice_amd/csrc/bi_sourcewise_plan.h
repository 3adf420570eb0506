// bi_sourcewise_plan.h -- source-wise models: the loops over staged points that never hand descriptors across the bus (host
// half; the planner is k_sourcewise_plan, bi_k_sourcewise_plan.h).  bi_eval_sourcewise_planned, bi_sample_stretch_sourcewise.
//
// bi_eval_factored screens and fills its work items on host threads (FacBatch, bi_factored.h) and uploads them; a loop over
// this model would do that twice per iteration.  PlannedItems keeps the buffers of up to n_max items on the device and queues,
// for n staged points in VarMap's layouts, k_sourcewise_plan -> k_morph_factored (values only, with the planner's live words)
// -> k_finish, with FacBatch::run's block count per item and its sub-batching (kFacPartialDoubles, gridDim.y chunks of 65 535).
// The evaluation has a fixed number of blocks per item and no in-launch mailbox, so nothing of that needs a host read: queue()
// waits for nothing, the partial buffers are allocated once and reused in stream order, and the sampler's step loop below runs
// without a stream synchronisation (counters[4]).  A live point's sums are the blocks' of bi_eval_factored, added in its order:
// ll is bit for bit the host path's.  A rejected point's blocks return at entry and k_finish skips it (perm -1, written by the
// planner with the point's -inf: so the perm is the planner's, per call of queue(), not an identity filled once).
// Where the non-empty-bin form is built and chosen (fac_nonempty_on; bi_sourcewise_nonempty.h) the same queue runs the planner's NE
// variant -> k_sourcewise_nonempty -> k_finish: the descriptors point into the datasets' compacted copies, the tile count is per
// item, and the grid's x is the most blocks an item of any dataset of the store takes -- known when the form is built, so still
// nothing is read and nothing waited for.
// On a finished event store (bi_sourcewise_events.h; bi_eval_sourcewise_events_planned, bi_sample_stretch_sourcewise_events, and
// through bi_grid.h bi_grid_reduce_sourcewise_events) the queue runs the planner's EV variant -> k_sourcewise_events (values only)
// -> k_finish: rows at the point's set's columns, the set's number of events and tiles per item, sum_s r_s for the finish, from the
// device table of the sets (ev_tab, uploaded when the store is finished).  The event kernel reads no live word: a rejected point
// gets zero tiles, so its blocks post +0.0 and return at entry.  The grid's x is the most blocks any set takes (ev_max_nbx).
#pragma once

namespace {

struct PlannedItems {
    bi_ctx* c;
    const bi_ctx::Factored& m;
    int SC, EM, W, NR;
    bool ev;                    // the event store (bi_sourcewise_events.h): the planner's EV variant and k_sourcewise_events
    bool ne;                    // the non-empty-bin form (bi_sourcewise_nonempty.h): the planner's NE variant and k_sourcewise_nonempty
    int nbx;                    // (ne, ev: the most blocks an item of ANY dataset of the store takes -- known without a host read)
    int64_t n_max = 0, per_call = 1;
    ScratchBuf status, live, rowoff, coef, rates, cnt_off, slot_lg, perm, partial, pflags, tiles;
    FactoredArgs fa{};
    SourcewiseNonemptyArgs na{};
    SourcewiseEventsArgs ea{};
    SourcewisePlanArgs pa{};

    // (a finished event store is what the context evaluates, as in FacBatch; only the entry points for it get here while one exists)
    explicit PlannedItems(bi_ctx* ctx)
        : c(ctx), m(ctx->fac), SC(m.S <= 2 ? 2 : m.S <= 4 ? 4 : 8), EM(std::max(1, m.max_own)), W(1 + EM), NR(m.n_rows_point),
          ev(m.ev_ready), ne(!ev && fac_nonempty_on(ctx)),
          nbx(ev ? m.ev_max_nbx : ne ? m.ne_max_nbx : std::min((int)(m.Bp / kTile), kFacBlocks)) {}

    // room for n_max items, both argument blocks; evaluate = false: the planner's buffers alone (queue() must not be called)
    int init(int64_t n, bool evaluate = true) {
        n_max = n;
        per_call = std::max<int64_t>(1, kFacPartialDoubles / (int64_t)nbx);
        const size_t un = (size_t)n, part = (size_t)std::min<int64_t>(std::min<int64_t>(65535, per_call), n) * (size_t)nbx;
        int rc;
        if ((rc = dev_alloc(c, status, un * sizeof(int32_t))) || (rc = dev_alloc(c, live, un * sizeof(unsigned))) ||
            (rc = dev_alloc(c, rowoff, un * NR * sizeof(int64_t))) || (rc = dev_alloc(c, coef, un * NR * W * sizeof(double))) ||
            (rc = dev_alloc(c, rates, un * SC * sizeof(double))) || (rc = dev_alloc(c, cnt_off, un * sizeof(int64_t))) ||
            (rc = dev_alloc(c, slot_lg, un * sizeof(double))) || (rc = dev_alloc(c, perm, un * sizeof(int64_t))) ||
            (evaluate && ((rc = dev_alloc(c, partial, part * sizeof(double))) || (rc = dev_alloc(c, pflags, part * sizeof(unsigned))))))
            return rc;
        if ((ne || ev) && (rc = dev_alloc(c, tiles, un * sizeof(int32_t)))) return rc;
        fa = FacBatch(c, 0).args();
        const char* g = (const char*)m.geom.p;
        pa.g.anchors = (const double*)(g + m.geom_off[0]);
        pa.g.anchor_off = (const int32_t*)(g + m.geom_off[1]);
        pa.g.n_own = (const int32_t*)(g + m.geom_off[2]);
        pa.g.own = (const int32_t*)(g + m.geom_off[3]);
        pa.g.own_stride = (const int64_t*)(g + m.geom_off[4]);
        pa.g.row_first = (const int64_t*)(g + m.geom_off[5]);
        pa.g.mus = (const double*)(g + m.geom_off[6]);
        pa.g.lgsum = (const double*)m.lgsum_dev.p;
        pa.g.T = m.T; pa.g.Bp = m.Bp; pa.g.d = m.d; pa.g.S = m.S;
        pa.NR = NR; pa.W = W;
        for (int s = 0; s < 8; ++s) pa.e[s] = fa.e[s];
        pa.status = (int32_t*)status.p; pa.live = (unsigned*)live.p; pa.rowoff = (int64_t*)rowoff.p; pa.coef = (double*)coef.p;
        pa.rates = (double*)rates.p; pa.cnt_off = (int64_t*)cnt_off.p; pa.slot_lg = (double*)slot_lg.p; pa.perm = (int64_t*)perm.p;
        if (ne) {
            pa.g.rowsum = (const double*)(g + m.geom_off[7]);
            pa.g.ne_off = (const int64_t*)m.ne_tab.p;
            pa.g.ne_np = pa.g.ne_off + m.T;
            pa.g.ne_cnt_off = pa.g.ne_off + 2 * m.T;
            pa.tiles = (int32_t*)tiles.p;
            na.ps = (const double*)m.ne_ps.p;
            na.counts = (const double*)m.ne_cnt.p;
            na.NR = NR;
            na.chunks = fa.chunks;
            na.max_blocks = kFacBlocks;
            for (int s = 0; s < 8; ++s) na.e[s] = fa.e[s];
        }
        if (ev) {
            pa.g.T = m.ev_T;
            pa.ev_first = (const int64_t*)m.ev_tab.p;
            pa.ev_n = pa.ev_first + m.ev_T;
            pa.ev_cols = m.ev_cols;
            pa.tiles = (int32_t*)tiles.p;
            ea.ps = (const double*)m.ev_ps.p;
            ea.outlier = m.ev_outlier;
            ea.NR = NR;
            ea.chunks = fa.chunks;
            ea.max_blocks = kFacBlocks;
            for (int s = 0; s < 8; ++s) ea.e[s] = fa.e[s];
        }
        return BI_OK;
    }

    // Queue the evaluation of the first n points staged at z / rs / ds (device) into out [n] (device); waits for nothing.
    // *launches (nullable) advances by what was queued.
    int queue(int64_t n, const double* z, const double* rs, const int64_t* ds, double* out, const char* who, int64_t* launches) {
        SourcewisePlanArgs p = pa;
        p.z = z; p.rs = rs; p.ds = ds; p.n = n; p.out = out;
        int rc = ev ? launch_sourcewise_plan_events(c, SC, p) : ne ? launch_sourcewise_plan_nonempty(c, SC, p) : launch_sourcewise_plan(c, SC, p);
        if (rc) return fail(c, rc, "%s: no planner variant for %d source slots", who, SC);
        HIP_TRY(c, hipGetLastError());
        int64_t queued = 1;
        const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && n == 1);
        c->last_point_pieces = 0;
        for (int64_t j0 = 0; j0 < n; j0 += per_call)
            for (int64_t i0 = j0; i0 < std::min(n, j0 + per_call); i0 += 65535) {
                const int64_t ni = std::min<int64_t>(65535, std::min(n, j0 + per_call) - i0);
                FactoredArgs b = fa;
                b.rowoff = (const int64_t*)rowoff.p + i0 * NR;
                b.coef = (const double*)coef.p + i0 * NR * W;
                b.rates = (const double*)rates.p + i0 * SC;
                b.item_cnt = (const int64_t*)cnt_off.p + i0;
                b.live = (const unsigned*)live.p + i0;
                b.partial = (double*)partial.p;
                b.pflags = (unsigned*)pflags.p;
                const dim3 grid((unsigned)nbx, (unsigned)ni);
                c->last_morph_nbx = grid.x; c->last_morph_items = grid.y; c->last_morph_fused = 0;
                if (ev) {
                    SourcewiseEventsArgs q = ea;
                    q.rowoff = b.rowoff; q.coef = b.coef; q.rates = b.rates; q.item_n = b.item_cnt;
                    q.item_tiles = (const int32_t*)tiles.p + i0;
                    q.partial = b.partial; q.pflags = b.pflags;
                    rc = launch_sourcewise_events(c, SC, EM, false, q, grid);
                } else if (ne) {
                    SourcewiseNonemptyArgs q = na;
                    q.rowoff = b.rowoff; q.coef = b.coef; q.rates = b.rates; q.item_cnt = b.item_cnt; q.live = b.live;
                    q.item_tiles = (const int32_t*)tiles.p + i0;
                    q.partial = b.partial; q.pflags = b.pflags;
                    rc = launch_sourcewise_nonempty(c, SC, EM, false, q, grid);
                } else
                    rc = launch_morph_factored(c, SC, EM, false, b, grid, nt);
                if (rc)
                    return fail(c, rc, "%s: no kernel variant for %d source slots with %d own axes", who, SC, EM);
                launch_finish(c, (const double*)partial.p, (const unsigned*)pflags.p, nbx, 1, ni, (const int64_t*)perm.p + i0,
                              (const double*)slot_lg.p + i0, out, nullptr);
                HIP_TRY(c, hipGetLastError());
                ++c->last_point_pieces;
                queued += 2;
            }
        if (launches) *launches += queued;
        return BI_OK;
    }
};

int sample_stretch_sourcewise(bi_ctx* c, const char* who, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                              const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                              const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble, const double* prior_mean,
                              const double* prior_sigma, const double* prior_const, double* chain, double* ll, int64_t* n_accepted,
                              int64_t* counters) {
    const size_t nE = (size_t)E, nW = (size_t)E * W;
    SamplerBuffers b;
    ResidentPoints pts;
    PlannedItems items(c);
    StretchArgs s{};
    int rc;
    if ((rc = stretch_check_chain(c, who, n_steps, nW, F))) return rc;
    // (host copies that live until the uploads have been waited for)
    const std::vector<double> h_lo = host_copy(lo, (size_t)F, 0.0), h_hi = host_copy(hi, (size_t)F, 0.0), h_x = host_copy(x0, nW * F, 0.0);
    if ((rc = pts.bind(c, s, E, (int64_t)nW, F, var_kind, var_index, z0, scale0, unit, dataset, c->fac.d, c->fac.S)) ||
        (rc = dev_upload(c, b.lo, h_lo)) || (rc = dev_upload(c, b.hi, h_hi)) || (rc = dev_upload(c, b.x, h_x)))
        return rc;
    const std::vector<double> h_pmean = host_copy(prior_sigma ? prior_mean : nullptr, (size_t)F, 0.0),
                              h_psigma = host_copy(prior_sigma, (size_t)F, std::numeric_limits<double>::infinity()),
                              h_pconst = host_copy(prior_const, nE, 0.0);
    const bool terms = prior_sigma || prior_const;
    if (prior_sigma && ((rc = dev_upload(c, b.pmean, h_pmean)) || (rc = dev_upload(c, b.psigma, h_psigma)))) return rc;
    if (prior_const && (rc = dev_upload(c, b.pconst, h_pconst))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t steps = (size_t)n_steps;
    if ((rc = dev_alloc(c, b.ll, nW * sizeof(double))) || (rc = dev_alloc(c, b.nacc, nW * sizeof(int64_t))) ||
        (rc = dev_alloc(c, b.chain, std::max<size_t>(steps, 1) * nW * F * sizeof(double))) ||
        (rc = dev_alloc(c, b.chain_ll, std::max<size_t>(steps, 1) * nW * sizeof(double))) || (rc = items.init((int64_t)nW)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(b.nacc.p, 0, nW * sizeof(int64_t), c->stream));
    s.E = E; s.W = W;
    s.first_ensemble = first_ensemble;
    s.k0 = (uint32_t)seed; s.k1 = (uint32_t)(seed >> 32);
    s.a = a;
    s.lo = (const double*)b.lo.p; s.hi = (const double*)b.hi.p;
    s.x = (double*)b.x.p; s.ll = (double*)b.ll.p; s.n_accepted = (int64_t*)b.nacc.p;
    s.ll_prop = (const double*)pts.llp.p;
    s.st_prop = (const int32_t*)items.status.p;
    s.prior_mean = prior_sigma ? (const double*)b.pmean.p : nullptr;
    s.prior_sigma = prior_sigma ? (const double*)b.psigma.p : nullptr;
    s.prior_const = prior_const ? (const double*)b.pconst.p : nullptr;
    int64_t launches = 0, evaluations = 0, half_steps = 0, loop_syncs = 0;
    const double* zp = c->fac.d > 0 ? (const double*)pts.zp.p : nullptr;

    // the start: every walker's own log density, read back once -- the only host read before the final copy
    s.h = -1;
    launch_stretch_propose(c, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = items.queue((int64_t)nW, zp, (const double*)pts.rsp.p, (const int64_t*)pts.dsp.p, (double*)pts.llp.p, who, &launches))) return rc;
    evaluations += (int64_t)nW;
    {
        std::vector<double> h_ll(nW);
        std::vector<int32_t> h_st(nW);
        hipError_t e = hipSuccess;
        if (terms) {
            launch_stretch_start_density(c, s);                 // b.ll = llp + p
            e = hipGetLastError();
        } else
            e = hipMemcpyAsync(b.ll.p, pts.llp.p, nW * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_ll.data(), b.ll.p, nW * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_st.data(), items.status.p, nW * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        else (void)hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s (start): %s", who, hipGetErrorString(e));
        if ((rc = stretch_check_start(c, who, nW, W, F, h_x, h_lo, h_hi, h_ll, h_st, terms))) return rc;
    }

    // the step loop: five kinds of launches per half-step, queued in order on the context's stream; nothing is read or waited for
    const int64_t n = E * (W / 2);
    for (int64_t t = 0; t < n_steps && !rc; ++t)
        for (int h = 0; h < 2 && !rc; ++h) {
            s.t = t; s.h = h;
            s.chain = (double*)b.chain.p + (size_t)t * nW * F;
            s.chain_ll = (double*)b.chain_ll.p + (size_t)t * nW;
            launch_stretch_propose(c, s);
            if (hipGetLastError() != hipSuccess) { rc = fail(c, BI_ERR_HIP, "%s (propose): launch failed", who); break; }
            if ((rc = items.queue(n, zp, (const double*)pts.rsp.p, (const int64_t*)pts.dsp.p, (double*)pts.llp.p, who, &launches))) break;
            launch_stretch_accept(c, s);
            if (hipGetLastError() != hipSuccess) { rc = fail(c, BI_ERR_HIP, "%s (accept): launch failed", who); break; }
            evaluations += n;
            ++half_steps;
            ++c->n_sampler_half_steps;
        }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);                  // (the buffers are freed with the scope)
        return rc;
    }
    // one copy of chain, log likelihoods and acceptance counters at the end of the call
    hipError_t e = hipSuccess;
    if (n_steps > 0) {
        e = hipMemcpyAsync(chain, b.chain.p, steps * nW * F * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ll, b.chain_ll.p, steps * nW * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(n_accepted, b.nacc.p, nW * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    if (counters) {
        counters[0] = half_steps; counters[1] = evaluations; counters[2] = 0; counters[3] = launches; counters[4] = loop_syncs;
        for (size_t w = 0; w < nW; ++w) counters[2] += n_accepted[w];
    }
    return BI_OK;
}

// the event store's entry points: a finished store, else BI_ERR_STATE naming the binned spelling
int events_routes_check(bi_ctx* c, const char* who, const char* binned) {
    int rc = fac_check(c, who, false, true);
    if (rc) return rc;
    if (c->fac.ev_open) return fail(c, BI_ERR_STATE, "%s: the event store is still being filled (bi_sourcewise_events_end first)", who);
    if (!c->fac.ev_ready)
        return fail(c, BI_ERR_STATE, "%s: the context holds no event store (bi_sourcewise_events_begin ... _end or bi_sourcewise_score_events "
                    "first; against counts the call is %s)", who, binned);
    return BI_OK;
}

// bi_eval_sourcewise_planned and bi_eval_sourcewise_events_planned behind their state checks
int eval_sourcewise_planned(bi_ctx* c, const char* who, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                            int32_t* status) {
    int rc;
    if (P < 0 || (P > 0 && !ll)) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointer", who);
    const int d = c->fac.d, S = c->fac.S;
    if (d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (P == 0) return BI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        // the rows as they are: rate_scale NULL is ones, dataset NULL is dataset 0
        const std::vector<double> ones(rate_scale ? 0 : (size_t)P * S, 1.0);
        const std::vector<int64_t> zeros(dataset ? 0 : (size_t)P, 0);
        ScratchBuf rows, d_ll;
        PackedUpload pu;
        PlannedItems items(c);
        if ((rc = packed_upload(c, {{z, (size_t)P * d * sizeof(double)}, {rate_scale ? rate_scale : ones.data(), (size_t)P * S * sizeof(double)},
                                    {dataset ? dataset : zeros.data(), (size_t)P * sizeof(int64_t)}},
                                0, pu, &rows)) ||
            (rc = dev_alloc(c, d_ll, (size_t)P * sizeof(double))) || (rc = items.init(P)))
            return rc;
        rc = items.queue(P, d > 0 ? pu.dev<double>(0) : nullptr, pu.dev<double>(1), pu.dev<int64_t>(2), (double*)d_ll.p, who, nullptr);
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(ll, d_ll.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (!rc && e == hipSuccess && status)
            e = hipMemcpyAsync(status, items.status.p, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (rc) return rc;
        if (e != hipSuccess || e2 != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
        return BI_OK;
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "%s: out of host memory", who);
    }
}

// bi_sample_stretch_sourcewise and bi_sample_stretch_sourcewise_events behind their state checks; T: the sets `dataset` indexes
int sample_stretch_sourcewise_checked(bi_ctx* c, const char* who, int64_t T, int64_t E, int W, int F, const int32_t* var_kind,
                                      const int32_t* var_index, const double* z0, const double* scale0, const double* unit, const int64_t* dataset,
                                      const double* x0, const double* lo, const double* hi, int64_t n_steps, double a, uint64_t seed,
                                      int64_t first_ensemble, const double* prior_mean, const double* prior_sigma, const double* prior_const,
                                      double* chain, double* ll, int64_t* n_accepted, int64_t* counters) {
    int rc;
    if ((rc = stretch_check_args(c, who, who, c->fac.d, c->fac.S, T, E, W, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi,
                                 n_steps, a, first_ensemble, prior_mean, prior_sigma, prior_const, chain, ll, n_accepted)))
        return rc;
    if (counters) counters[0] = counters[1] = counters[2] = counters[3] = counters[4] = 0;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        return sample_stretch_sourcewise(c, who, E, W, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a, seed, first_ensemble,
                                         prior_mean, prior_sigma, prior_const, chain, ll, n_accepted, counters);
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "%s: out of host memory", who);
    }
}

}  // namespace

extern "C" {

int bi_eval_sourcewise_planned(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                               int32_t* status) {
    const char* who = "bi_eval_sourcewise_planned";
    int rc = fac_check(c, who, true);
    if (rc) return rc;
    return eval_sourcewise_planned(c, who, P, z, rate_scale, dataset, ll, status);
}

int bi_eval_sourcewise_events_planned(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                                      int32_t* status) {
    const char* who = "bi_eval_sourcewise_events_planned";
    int rc = events_routes_check(c, who, "bi_eval_sourcewise_planned");
    if (rc) return rc;
    return eval_sourcewise_planned(c, who, P, z, rate_scale, dataset, ll, status);
}

int bi_sample_stretch_sourcewise(bi_ctx* c, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                                 const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                                 const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble, const double* prior_mean,
                                 const double* prior_sigma, const double* prior_const, double* chain, double* ll, int64_t* n_accepted,
                                 int64_t* counters) {
    const char* who = "bi_sample_stretch_sourcewise";
    int rc = fac_check(c, who, true);
    if (rc) return rc;
    return sample_stretch_sourcewise_checked(c, who, c->fac.T, E, W, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a, seed,
                                             first_ensemble, prior_mean, prior_sigma, prior_const, chain, ll, n_accepted, counters);
}

int bi_sample_stretch_sourcewise_events(bi_ctx* c, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                                        const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                                        const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble,
                                        const double* prior_mean, const double* prior_sigma, const double* prior_const, double* chain, double* ll,
                                        int64_t* n_accepted, int64_t* counters) {
    const char* who = "bi_sample_stretch_sourcewise_events";
    int rc = events_routes_check(c, who, "bi_sample_stretch_sourcewise");
    if (rc) return rc;
    return sample_stretch_sourcewise_checked(c, who, c->fac.ev_T, E, W, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a,
                                             seed, first_ensemble, prior_mean, prior_sigma, prior_const, chain, ll, n_accepted, counters);
}

}  // extern "C"
