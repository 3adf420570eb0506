// bi_sourcewise_scan.h -- source-wise models on the matrix-core scan route (host half; the planner's kernels are
// bi_k_sourcewise_scan.h's).  bi_eval_sourcewise_scan; bi_grid_reduce_sourcewise (bi_grid.h) takes it as route 1.
//
// PlannedItems (bi_sourcewise_plan.h) gives every staged point a work item of its own, whose blocks stream the point's NR rows:
// a batch whose points pile up in a handful of cell tuples -- a gridded likelihood -- reads the same rows once per point.
// k_scan_mfma (bi_k_scan.h) reads a group's rows once per strip and forms mu[bin][point] = sum_k row_k[bin] coef_k[point] for 16
// points at a time on the fp64 matrix cores; it is written over rows named by `rowoff`, so the compacted copies of the non-empty-
// bin form (bi_sourcewise_nonempty.h: all the model's rows per dataset, padded to whole tiles) are rows it can stream as they are.
// ScanItems turns n staged points (VarMap's layouts) into its work items without handing anything across the bus:
//     1. screen    k_sourcewise_plan<SC, NE = true>, unchanged: status words, live words, rowoff [NR], coef [NR][W], rates [SC],
//                  cnt_off, tiles, slot_lg per point, -inf for a rejected point -- bit for bit bi_eval_sourcewise_planned's
//     2. key       k_sourcewise_scan_key: the tuple of cells and the dataset as one 64-bit key, rejected points above all others
//     3. sort      prim_sort_pairs over the bits of the key space; groups of equal keys, 16-point items and a padded last item per
//                  group by the per-position route of bi_planning_device.h (k_plan_heads, k_plan_item_heads, k_plan_group_flags,
//                  k_plan_count_valid and the prefix scans of bi_prim.h); k_sourcewise_scan_cut cuts very long groups, and
//                  k_sourcewise_scan_groups stands for k_plan_group_first / k_plan_group_items, which want the counts on the
//                  host first.  ONE host read per call: valid points, items, groups, the most items of a group.
//     4. fill      k_sourcewise_scan_fill: coef[(item NR + k) 16 + slot] = w_k r_s(k), rowoff / item_cnt / item_tiles from the
//                  group's first point, slot_lg and perm per slot
//     5. evaluate  launch_scan_mfma(c, 2, true, NR, ...) on m.ne_ps / m.ne_cnt, `partial` zeroed on the stream first, nslots by the
//                  rule of bi_planning_device.h (scan_resident_blocks: full rounds of resident blocks, evened-out strips), one
//                  launch per 65 535 groups
//     6. finish    k_finish_scan: the nslots partial sums of a slot in a fixed order, less slot_lg, through perm into `out`
// The kernel adds sum n log mu over the listed bins; the linear term sum_s lambda_s and the lgamma sum are the planner's slot_lg.
//
// Conditions: the non-empty-bin form built and chosen (fac_nonempty_on), NR <= 32, and a key space below 2^63.
// Properties: no floating-point atomics besides k_scan_mfma's own, which go into partial slots one wave owns; no scratch in the
// new kernels; the same call gives the same bits every time.  UNLIKE the per-point kernels, a point's bits may depend on the
// batch it is evaluated in: which 16 points share an item, the number of partial slots (nslots follows the number of groups) and
// whether a block of bins takes the product form (every point of the item must allow it) all follow from the batch.  The status
// words and the -inf of rejected points do not.
#pragma once

#include <optional>

namespace {

// 0: the scan route can take this context's source-wise model; else the message's cause (1 form, 2 rows, 3 key space)
int sourcewise_scan_refusal(const bi_ctx* c, uint64_t* bad_key = nullptr) {
    const bi_ctx::Factored& m = c->fac;
    if (!fac_nonempty_on(c)) return 1;
    if (m.n_rows_point > 32) return 2;
    uint64_t cells = 1;
    for (int s = 0; s < m.S; ++s) {
        const uint64_t n = (uint64_t)(m.row_first[(size_t)s + 1] - m.row_first[(size_t)s]);
        if (cells > (((uint64_t)1 << 63) - 1) / n) return 3;
        cells *= n;
    }
    const uint64_t T = (uint64_t)std::max<int64_t>(m.T, 1);
    if (cells > (((uint64_t)1 << 63) - 1) / T) return 3;
    if (bad_key) *bad_key = cells * T;
    return 0;
}

int sourcewise_scan_check(bi_ctx* c, const char* who) {
    switch (sourcewise_scan_refusal(c)) {
        case 1:
            return fail(c, BI_ERR_INVALID, "%s: the scan route streams the compacted rows of the non-empty-bin form: build it with "
                                           "bi_sourcewise_build_nonempty (and leave sourcewise_form at 1)", who);
        case 2:
            return fail(c, BI_ERR_INVALID, "%s: a point of this model reads %d rows, the matrix-core scan kernel takes at most 32 (the row limit)",
                        who, c->fac.n_rows_point);
        case 3:
            return fail(c, BI_ERR_INVALID, "%s: the cell tuples of this model times its %lld datasets do not fit a 63-bit sort key", who,
                        (long long)c->fac.T);
    }
    return BI_OK;
}

struct ScanItems {
    bi_ctx* c;
    const bi_ctx::Factored& m;
    PlannedItems pt;            // the planner's argument block and its per-point buffers
    int SC, NR;
    int end_bit = 64;
    int64_t n_max = 0, strips = 1;
    SourcewiseScanArgs sa{};
    ScratchBuf keys, keys2, idx, idx2, d_a, gstart, item_incl, gid_incl, tmp, scal, grp_first, grp_items;
    ScratchBuf rowoff, coef, item_cnt, item_tiles, slot_lg, perm, partial;

    explicit ScanItems(bi_ctx* ctx) : c(ctx), m(ctx->fac), pt(ctx), SC(pt.SC), NR(pt.NR) {}

    // room for n_max points; the items' buffers follow the counts of every call
    int init(int64_t n) {
        uint64_t bad_key = 0;
        if (sourcewise_scan_refusal(c, &bad_key)) return fail(c, BI_ERR_STATE, "ScanItems: the scan route is not available");
        n_max = n;
        int rc = pt.init(n, false);             // (the planner's buffers alone: the per-point kernels' partial sums are not used here)
        if (rc) return rc;
        const size_t un = (size_t)n;
        size_t sort_bytes = 0, max_bytes = 0, sum_bytes = 0;
        end_bit = 1;
        while (end_bit < 64 && (bad_key >> end_bit) != 0) ++end_bit;
        (void)prim_sort_pairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int64_t*)nullptr, (int64_t*)nullptr, un, 0u,
                              (unsigned)end_bit, c->stream);
        (void)prim_inclusive_scan_max(nullptr, max_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, un, c->stream);
        (void)prim_inclusive_scan_sum(nullptr, sum_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, un, c->stream);
        if ((rc = dev_alloc(c, keys, un * 8)) || (rc = dev_alloc(c, keys2, un * 8)) || (rc = dev_alloc(c, idx, un * 8)) ||
            (rc = dev_alloc(c, idx2, un * 8)) || (rc = dev_alloc(c, d_a, un * 8)) || (rc = dev_alloc(c, gstart, un * 8)) ||
            (rc = dev_alloc(c, item_incl, un * 8)) || (rc = dev_alloc(c, gid_incl, un * 8)) || (rc = dev_alloc(c, scal, 64)) ||
            (rc = dev_alloc(c, grp_first, un * 8)) || (rc = dev_alloc(c, grp_items, un * 4)) ||
            (rc = dev_alloc(c, tmp, std::max({sort_bytes, max_bytes, sum_bytes, (size_t)256}))))
            return rc;
        int64_t max_np = kTile;
        for (int64_t np : m.ne_np) max_np = std::max(max_np, np);
        strips = max_np / 32;                  // k_scan_mfma<2, ..>: strips of 32 bins
        sa.status = (const int32_t*)pt.status.p; sa.rowoff_pt = (const int64_t*)pt.rowoff.p; sa.coef_pt = (const double*)pt.coef.p;
        sa.rates_pt = (const double*)pt.rates.p; sa.cnt_off_pt = (const int64_t*)pt.cnt_off.p; sa.tiles_pt = (const int32_t*)pt.tiles.p;
        sa.slot_lg_pt = (const double*)pt.slot_lg.p;
        sa.ne_off = pt.pa.g.ne_off; sa.ne_np = pt.pa.g.ne_np;
        sa.T = m.T; sa.NR = NR; sa.W = pt.W; sa.SC = SC; sa.S = m.S;
        sa.bad_key = bad_key;
        int first = 0;
        for (int s = 0; s < 8; ++s) {
            sa.first[s] = first;
            sa.row_first[s] = s < m.S ? m.row_first[(size_t)s] : 0;
            sa.mult[s] = 0;
            if (s < m.S) first += 1 << m.n_own[(size_t)s];
        }
        int64_t mult = 1;
        for (int s = m.S - 1; s >= 0; --s) {
            sa.mult[s] = mult;
            mult *= m.row_first[(size_t)s + 1] - m.row_first[(size_t)s];
        }
        sa.keys = (uint64_t*)keys.p; sa.idx = (int64_t*)idx.p;
        sa.idx_s = (const int64_t*)idx2.p; sa.gstart = (int64_t*)gstart.p;
        sa.item_incl = (const int64_t*)item_incl.p; sa.gid_incl = (const int64_t*)gid_incl.p;
        sa.scal = (int64_t*)scal.p; sa.grp_first = (int64_t*)grp_first.p; sa.grp_items = (int32_t*)grp_items.p;
        return BI_OK;
    }

    // waves per group (a multiple of four): the rule of plan_points_resident_impl's scan plans (bi_planning_device.h) for rows
    // in bin order -- the fewest rounds of resident blocks times strips per wave among the evened-out splits, and among those
    // within 1 % the finest that leaves a wave 8 strips.  That rule is a lambda local to the planner there and cannot be called:
    // this is a copy of its branch for rows in bin order (no forced split, no pipe-bound model) and must be kept in step by hand.
    int64_t waves_per_group(int64_t n_groups, int64_t n_items, int resident) const {
        const int64_t capacity = (int64_t)c->prop.multiProcessorCount * std::max(1, resident);
        const int64_t slot_cap = std::max<int64_t>(4, ((int64_t)1 << 30) / std::max<int64_t>(1, n_items * 16 * (int64_t)sizeof(double)));
        const int64_t b_max = std::max<int64_t>(1, std::min<int64_t>(strips / 4, slot_cap / 4));
        auto cost_of = [&](int64_t b) -> double {
            const int64_t per_wave = (strips + 4 * b - 1) / (4 * b);
            if ((strips + 4 * per_wave - 1) / (4 * per_wave) != b) return 1e300;
            return (double)((b * n_groups + capacity - 1) / capacity) * (double)per_wave;
        };
        double best_cost = 1e300;
        int64_t best_b = 1;
        for (int64_t b = 1; b <= b_max; ++b)
            if (cost_of(b) < best_cost) { best_cost = cost_of(b); best_b = b; }
        for (int64_t b = b_max; b > best_b; --b)
            if (cost_of(b) <= 1.01 * best_cost && (strips + 4 * b - 1) / (4 * b) >= 8) { best_b = b; break; }
        return best_b * 4;
    }

    // Queue the evaluation of the first n points staged at z / rs / ds (device) into out [n] (device), in the caller's order.
    // counters (nullable) advance: [0] groups, [1] items, [2] live points, [3] launches, [4] host reads.
    int queue(int64_t n, const double* z, const double* rs, const int64_t* ds, double* out, const char* who, int64_t* counters) {
        if (n < 1) return BI_OK;
        if (n > n_max) return fail(c, BI_ERR_INVALID, "%s: %lld points staged, room for %lld", who, (long long)n, (long long)n_max);
        const size_t un = (size_t)n;
        int64_t launches = 0;
        hipError_t e = hipSuccess;
        int64_t h_scal[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        SourcewiseScanArgs a = sa;
        {
            // the planner's share of a call: everything in front of the matrix-core launch, the host read included
            std::optional<EventScope> ev;
            if (c->sourcewise_scan_timed & 1) ev.emplace(c);
            SourcewisePlanArgs p = pt.pa;
            p.z = z; p.rs = rs; p.ds = ds; p.n = n; p.out = out;
            if (launch_sourcewise_plan_nonempty(c, SC, p)) return fail(c, BI_ERR_INVALID, "%s: no planner variant for %d source slots", who, SC);
            a.ds = ds; a.n = n;
            launch_sourcewise_scan_key(c, a);
            HIP_TRY(c, hipGetLastError());
            size_t tb = tmp.bytes;
            e = prim_sort_pairs(tmp.p, tb, (const uint64_t*)keys.p, (uint64_t*)keys2.p, (const int64_t*)idx.p, (int64_t*)idx2.p, un, 0u,
                                (unsigned)end_bit, c->stream);
            if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s (sort): %s", who, hipGetErrorString(e));
            // groups of at most `cut` points: about three rounds of resident blocks over the chip even when every point shares one
            // tuple of cells (a group gives at most strips / 16 blocks); shorter groups stay whole
            const int resident0 = scan_resident_blocks(false, 2, NR);
            const int64_t capacity = (int64_t)c->prop.multiProcessorCount * std::max(1, resident0);
            const int64_t b_cap = std::max<int64_t>(1, strips / 16), pieces = (3 * capacity + b_cap - 1) / b_cap;
            const int64_t cut_items = std::max<int64_t>(16, (((n + 15) / 16 + pieces - 1) / pieces + 3) / 4 * 4);
            a.cut = cut_items * 16;
            const unsigned nblk = (unsigned)((n + kThreads - 1) / kThreads);
            const uint64_t* keys_s = (const uint64_t*)keys2.p;
            HIP_TRY(c, hipMemsetAsync(scal.p, 0, 64, c->stream));
            hipLaunchKernelGGL(k_plan_heads, dim3(nblk), dim3(kThreads), 0, c->stream, keys_s, n, (int64_t*)d_a.p);
            tb = tmp.bytes;
            e = prim_inclusive_scan_max(tmp.p, tb, (const int64_t*)d_a.p, (int64_t*)gstart.p, un, c->stream);
            if (e == hipSuccess) {
                launch_sourcewise_scan_cut(c, (int64_t*)gstart.p, n, a.cut);
                hipLaunchKernelGGL(k_plan_item_heads, dim3(nblk), dim3(kThreads), 0, c->stream, (const int64_t*)gstart.p, n, 16, (int64_t*)d_a.p);
                tb = tmp.bytes;
                e = prim_inclusive_scan_sum(tmp.p, tb, (const int64_t*)d_a.p, (int64_t*)item_incl.p, un, c->stream);
            }
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_plan_group_flags, dim3(nblk), dim3(kThreads), 0, c->stream, (const int64_t*)gstart.p, n, (int64_t*)d_a.p);
                tb = tmp.bytes;
                e = prim_inclusive_scan_sum(tmp.p, tb, (const int64_t*)d_a.p, (int64_t*)gid_incl.p, un, c->stream);
            }
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_plan_count_valid, dim3(1), dim3(64), 0, c->stream, keys_s, n, a.bad_key, (int64_t*)scal.p);
                launch_sourcewise_scan_groups(c, a);
                e = hipGetLastError();
            }
            // the one host read of the call: valid points, items, groups, the most items of a group
            if (e == hipSuccess) e = hipMemcpyAsync(h_scal, scal.p, sizeof h_scal, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            else (void)hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s (planning): %s", who, hipGetErrorString(e));
            launches += 12;
            const int64_t n_valid = h_scal[0], n_items = h_scal[1];
            if (n_valid > 0) {
                const size_t ni = (size_t)n_items;
                int rc;
                if ((rc = dev_alloc(c, rowoff, ni * NR * 8)) || (rc = dev_alloc(c, coef, ni * NR * 16 * 8)) || (rc = dev_alloc(c, item_cnt, ni * 8)) ||
                    (rc = dev_alloc(c, item_tiles, ni * 4)) || (rc = dev_alloc(c, slot_lg, ni * 16 * 8)) || (rc = dev_alloc(c, perm, ni * 16 * 8)))
                    return rc;
                a.n_valid = n_valid;
                a.rowoff = (int64_t*)rowoff.p; a.coef = (double*)coef.p; a.item_cnt = (int64_t*)item_cnt.p;
                a.item_tiles = (int32_t*)item_tiles.p; a.slot_lg = (double*)slot_lg.p; a.perm = (int64_t*)perm.p;
                launch_sourcewise_scan_fill(c, a);
                HIP_TRY(c, hipGetLastError());
                ++launches;
            }
        }
        const int64_t n_valid = h_scal[0], n_items = h_scal[1], n_groups = h_scal[6];
        if (n_valid > 0) {
            const int resident = scan_resident_blocks(false, 2, NR);
            const int64_t nslots = waves_per_group(n_groups, n_items, resident);
            int rc;
            if ((rc = dev_alloc(c, partial, (size_t)n_items * (size_t)nslots * 16 * sizeof(double)))) return rc;
            HIP_TRY(c, hipMemsetAsync(partial.p, 0, (size_t)n_items * (size_t)nslots * 16 * sizeof(double), c->stream));
            ScanArgs s{};
            s.ps = (const double*)m.ne_ps.p; s.counts = (const double*)m.ne_cnt.p;
            s.rowoff = (const int64_t*)rowoff.p; s.coef = (const double*)coef.p;
            s.item_cnt = (const int64_t*)item_cnt.p; s.item_tiles = (const int32_t*)item_tiles.p;
            s.partial = (double*)partial.p; s.NS = NR; s.nslots = (int)nslots;
            c->last_scan_nslots = nslots; c->last_scan_resident = resident;
            c->last_scan_groups = n_groups; c->last_scan_max_items = h_scal[3];
            c->last_scan_cb = 2; c->last_scan_by_count = 0; c->last_scan_prod = 0;
            for (int64_t g0 = 0; g0 < n_groups; g0 += 65535) {
                const int64_t ng = std::min<int64_t>(65535, n_groups - g0);
                s.grp_first = (const int64_t*)grp_first.p + g0;
                s.grp_items = (const int32_t*)grp_items.p + g0;
                std::optional<EventScope> ev;
                if (c->sourcewise_scan_timed & 2) ev.emplace(c);
                ++c->n_scan_launches;
                launch_scan_mfma(c, 2, true, NR, dim3((unsigned)(nslots / 4), (unsigned)ng), s);
                ++launches;
            }
            hipLaunchKernelGGL(k_finish_scan, dim3((unsigned)((n_items + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, c->stream,
                               (const double*)partial.p, (int)nslots, n_items, (const int64_t*)perm.p, (const double*)slot_lg.p, out);
            HIP_TRY(c, hipGetLastError());
            launches += 2;
        }
        if (counters) {
            counters[0] += n_groups; counters[1] += n_items; counters[2] += n_valid; counters[3] += launches; counters[4] += 1;
        }
        return BI_OK;
    }
};

}  // namespace

extern "C" {

int bi_eval_sourcewise_scan(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                            int32_t* status, int64_t* counters) {
    const char* who = "bi_eval_sourcewise_scan";
    int rc = fac_check(c, who, true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !ll)) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointer", who);
    const int d = c->fac.d, S = c->fac.S;
    if (d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (counters) counters[0] = counters[1] = counters[2] = counters[3] = counters[4] = 0;
    if (P == 0) return BI_OK;
    if ((rc = sourcewise_scan_check(c, who))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        // the rows as they are: rate_scale NULL is ones, dataset NULL is dataset 0
        const std::vector<double> ones(rate_scale ? 0 : (size_t)P * S, 1.0);
        const std::vector<int64_t> zeros(dataset ? 0 : (size_t)P, 0);
        ScratchBuf rows, d_ll;
        PackedUpload pu;
        ScanItems items(c);
        if ((rc = packed_upload(c, {{z, (size_t)P * d * sizeof(double)}, {rate_scale ? rate_scale : ones.data(), (size_t)P * S * sizeof(double)},
                                    {dataset ? dataset : zeros.data(), (size_t)P * sizeof(int64_t)}},
                                0, pu, &rows)) ||
            (rc = dev_alloc(c, d_ll, (size_t)P * sizeof(double))) || (rc = items.init(P)))
            return rc;
        rc = items.queue(P, d > 0 ? pu.dev<double>(0) : nullptr, pu.dev<double>(1), pu.dev<int64_t>(2), (double*)d_ll.p, who, counters);
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(ll, d_ll.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (!rc && e == hipSuccess && status)
            e = hipMemcpyAsync(status, items.pt.status.p, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (rc) return rc;
        if (e != hipSuccess || e2 != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
        return BI_OK;
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "%s: out of host memory", who);
    }
}

}  // extern "C"
