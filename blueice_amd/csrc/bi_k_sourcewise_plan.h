// bi_k_sourcewise_plan.h -- k_sourcewise_plan<SC>: the device path from a staged point of a source-wise model to a work item of
// k_morph_factored.  Translation unit tu_sourcewise_plan.hip; host half bi_sourcewise_plan.h.
//
// Input: n points in VarMap's layouts (z [n][d], rs [n][S], ds [n]) and the device copy of the model's geometry
// (SourcewiseGeom).  Output per point: the status word of fac_screen (bi_factored.h) -- dataset, then the anchor box over all d
// axes with nan outside, then the rates -- and the value-order descriptors of FacBatch::fill, bit for bit: rowoff [n][NR],
// coef [n][NR][W] (column 0 = w_c, the others zero), rates [n][SC], cnt_off [n], slot_lg [n]; the live word [n] that
// k_morph_factored<.., GRAD = false, ..> reads at block entry; and k_finish's perm [n]: i for a live point, -1 for a rejected
// one, whose result k_finish then neither sums nor writes -- the planner writes its -inf into out [n] itself.
//
// One thread per (point, source slot): the SC lanes of a point are neighbours in one wave.  A lane tests the box of the axes
// a = slot, slot + SC, ..., computes its own source, and the group ORs its flags with log2(SC) lane exchanges.  So the dependent
// loads of a point are one binary search per own axis (at most three, side by side) and one rate per corner, whatever d and S
// are, and a half-step of the sampler is one launch of ceil(n SC / 256) blocks.  The limits e_s <= 3 and 8 corners are unrolled,
// so every index into t[], st[] is a compile-time constant (no scratch: profiles/sourcewise_plan_kernel_resources.txt); the
// geometry arrays are indexed by the run-time slot from global memory, not from the kernel arguments.
//
// The arithmetic, every operation rounded on its own (the host is compiled without contraction):
//     k      = (number of anchors <= z) - 1, clamped to [0, n - 2]      find_cell: the upper bound, the last cell closed
//     t      = (z - g_k) / (g_{k+1} - g_k)                              one IEEE division
//     w_c    = prod_j (t_j or 1 - t_j), own-axis order from 1.0; first own axis = most significant corner bit
//     M_s    = sum_c mus[row_c] w_c, left to right from 0.0;   r_s = M_s rs_s
// A rejected point gets the same in-range descriptors (k is clamped whatever z is, nan included) with cnt_off = 0 and
// slot_lg = 0, and never runs: live = 0, perm = -1.
#pragma once

namespace {

// (k, t) of z on the axis whose n >= 2 anchors are g[0 .. n)
__device__ __forceinline__ void plan_find_cell(const double* __restrict__ g, int n, double z, int& k, double& t) {
    int lo = 0, hi = n;                    // std::upper_bound: the first anchor with z < g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(z < g[mid])) lo = mid + 1;
        else hi = mid;
    }
    k = min(max(lo - 1, 0), n - 2);
    const double gk = g[k];
    t = __ddiv_rn(__dsub_rn(z, gk), __dsub_rn(g[k + 1], gk));
}

//
// NE = true: the descriptors of k_sourcewise_nonempty instead (the non-empty-bin form, bi_sourcewise_nonempty.h), bit for bit
// FacBatch::fill's on that route: rowoff = ne_off[ds] + row ne_np[ds], cnt_off = ne_cnt_off[ds], tiles = ne_np[ds] / 512, and
//     N_s      = sum_c w_c R_{s,c}, one fma per corner from 0.0;   lambda_s = r_s N_s
//     slot_lg  = (sum_s lambda_s, sources ascending from 0.0) + lgsum[ds]
// (the lane of source slot s computes lambda_s, lane 0 collects them in order).  NE = false is the code it was.
//
// EV = true (with NE = false): the descriptors of k_sourcewise_events instead (the event store, bi_sourcewise_events.h), bit for
// bit FacBatch::fill's with events = true; a.g.T is the number of event sets:
//     rowoff   = ev_first[ds] + row ev_cols,   cnt_off = ev_n[ds] (the kernel's item_n),   tiles = max(1, ceil(ev_n[ds] / 512))
//     slot_lg  = sum_s r_s, sources ascending from 0.0, one rounded addition each (the slot lanes hand r_s to lane 0)
// No lgamma, no rowsum.  The event kernel reads no live word: a rejected point gets tiles = 0, with which every block of its item
// posts +0.0 and returns at entry.  EV = false is the code it was.
template <int SC, bool NE = false, bool EV = false>
__global__ __launch_bounds__(kThreads) void k_sourcewise_plan(const SourcewisePlanArgs a) {
    static_assert(SC == 2 || SC == 4 || SC == 8, "the source slots of a point share a wave");
    static_assert(!(NE && EV), "the non-empty-bin form and the event store are two forms of the data");
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t i = gid / SC;
    const int s = (int)(gid % SC);
    if (i >= a.n) return;                  // (whole groups: the lane exchanges below stay inside a point)
    const SourcewiseGeom& m = a.g;

    // the box test, this lane's share of the d axes (owned or not); nan is outside
    unsigned flags = 0u;
    for (int ax = s; ax < m.d; ax += SC) {
        const int o = m.anchor_off[ax], n = m.anchor_off[ax + 1] - o;
        const double v = a.z[i * m.d + ax];
        if (!(m.anchors[o] <= v && v <= m.anchors[o + n - 1])) flags |= (unsigned)BI_ST_OUT_OF_BOUNDS;
    }

    // this lane's source: cell and fraction of its own axes, then its corner rows, weights and rate
    const bool real = s < m.S;
    const int e = real ? m.n_own[s] : -1;
    int first = 0;                         // the source's first row within the item
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q < s && a.e[q] >= 0) first += 1 << a.e[q];
    double rate = 0.0;
    [[maybe_unused]] double lambda = 0.0;
    [[maybe_unused]] int64_t ne_off = 0, ne_np = 0;
    if constexpr (NE) {
        const int64_t ds = a.ds[i];
        const int64_t t = (ds < 0 || ds >= m.T) ? 0 : ds;      // (a rejected point: in-range descriptors that never run)
        ne_off = m.ne_off[t];
        ne_np = m.ne_np[t];
    }
    [[maybe_unused]] int64_t ev_first = 0, ev_n = 0;
    if constexpr (EV) {
        const int64_t ds = a.ds[i];
        const int64_t t = (ds < 0 || ds >= m.T) ? 0 : ds;      // (a rejected point: in-range descriptors that never run)
        ev_first = a.ev_first[t];
        ev_n = a.ev_n[t];
    }
    if (real) {
        int64_t base = m.row_first[s];
        double t[kFacMaxOwn];
        int64_t st[kFacMaxOwn];
#pragma unroll
        for (int j = 0; j < kFacMaxOwn; ++j) {
            t[j] = 0.0;
            st[j] = 0;
            if (j < e) {
                const int ax = m.own[s * kFacMaxOwn + j];
                const int o = m.anchor_off[ax], n = m.anchor_off[ax + 1] - o;
                int k;
                plan_find_cell(m.anchors + o, n, a.z[i * m.d + ax], k, t[j]);
                st[j] = m.own_stride[s * kFacMaxOwn + j];
                base += (int64_t)k * st[j];
            }
        }
        const int nc = 1 << e;
        double M = 0.0;
        [[maybe_unused]] double N = 0.0;
#pragma unroll
        for (int c = 0; c < (1 << kFacMaxOwn); ++c) {
            if (c < nc) {
                int64_t r = base;
                double wc = 1.0;
#pragma unroll
                for (int j = 0; j < kFacMaxOwn; ++j)
                    if (j < e) {
                        const bool up = (c >> (e - 1 - j)) & 1;
                        if (up) r += st[j];
                        wc = __dmul_rn(wc, up ? t[j] : __dsub_rn(1.0, t[j]));
                    }
                const int64_t row = i * a.NR + first + c;
                if constexpr (NE) {
                    a.rowoff[row] = ne_off + r * ne_np;
                    N = __fma_rn(wc, m.rowsum[r], N);
                } else if constexpr (EV) {
                    a.rowoff[row] = ev_first + r * a.ev_cols;
                } else {
                    a.rowoff[row] = r * m.Bp;
                }
                a.coef[row * a.W] = wc;
                for (int x = 1; x < a.W; ++x) a.coef[row * a.W + x] = 0.0;
                M = __dadd_rn(M, __dmul_rn(m.mus[r], wc));
            }
        }
        rate = __dmul_rn(M, a.rs[i * m.S + s]);
        if constexpr (NE) lambda = __dmul_rn(rate, N);
        if (!(rate >= 0.0 && rate < __builtin_huge_val())) flags |= (unsigned)BI_ST_UNPHYSICAL;
    }
    a.rates[i * SC + s] = rate;            // (a padded slot: zero)

#pragma unroll
    for (int x = 1; x < SC; x <<= 1) flags |= (unsigned)__shfl_xor((int)flags, x);
    [[maybe_unused]] double lam_sum = 0.0;
    if constexpr (NE) {
#pragma unroll
        for (int q = 0; q < SC; ++q) lam_sum = __dadd_rn(lam_sum, __shfl(lambda, q, SC));      // (a padded slot adds +0.0)
    }
    if constexpr (EV) {
#pragma unroll
        for (int q = 0; q < SC; ++q) lam_sum = __dadd_rn(lam_sum, __shfl(rate, q, SC));        // (a padded slot adds +0.0)
    }
    if (s == 0) {
        const int64_t ds = a.ds[i];
        const int32_t status = (ds < 0 || ds >= m.T) ? BI_ST_BAD_DATASET
                               : (flags & BI_ST_OUT_OF_BOUNDS) ? BI_ST_OUT_OF_BOUNDS
                               : (flags & BI_ST_UNPHYSICAL)    ? BI_ST_UNPHYSICAL
                                                               : 0;
        a.status[i] = status;
        a.live[i] = status == 0 ? 1u : 0u;
        if constexpr (NE) {
            a.cnt_off[i] = status == 0 ? m.ne_cnt_off[ds] : 0;
            a.slot_lg[i] = status == 0 ? __dadd_rn(lam_sum, m.lgsum[ds]) : 0.0;
            a.tiles[i] = (int32_t)(ne_np / kTile);
        } else if constexpr (EV) {
            a.cnt_off[i] = status == 0 ? ev_n : 0;
            a.slot_lg[i] = status == 0 ? lam_sum : 0.0;
            a.tiles[i] = status != 0 ? 0 : ev_n > kTile ? (int32_t)((ev_n + kTile - 1) / kTile) : 1;
        } else {
            a.cnt_off[i] = status == 0 ? ds * m.Bp : 0;
            a.slot_lg[i] = status == 0 ? m.lgsum[ds] : 0.0;
        }
        a.perm[i] = status == 0 ? i : -1;
        if (status != 0) a.out[i] = -__builtin_huge_val();
    }
}

}  // namespace
