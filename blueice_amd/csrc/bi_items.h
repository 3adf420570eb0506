// bi_items.h -- the host path of "one work item per live point", from the screen to k_finish, that bi_eval_grad, bi_eval_hess,
// bi_eval_gof and bi_eval_real share, and the value-only rows of the entry points that write bins (bi_expected_counts,
// bi_set_asimov_counts, bi_expected_coarse):
//   ItemRoute          which rows a context's point evaluations read (dense, compacted non-empty bins, events), decided once
//   screen_points      the early exits of every point, with or without the dataset test
//   PointDerivs        one live point's rates, corner-weight derivatives and first-order coefficient columns
//   ItemBatch          the six descriptor arrays of the live points: filled on host threads, uploaded in one copy, bound into
//                      the kernel's argument block chunk by chunk (run_item_chunks), the sums finished by k_finish
//   fill_value_rows, download_live_runs    descriptors and download of the kernels that write bins, not sums
#pragma once

namespace {

inline bool any_negative_source(const bi_ctx* c) {
    bool any_neg = false;
    for (int q = 0; q < c->S; ++q) any_neg |= (c->allow_neg[(size_t)q] != 0);
    return any_neg;
}

// The rows a point evaluation of this context reads, per dataset ds:
//   compact   the non-empty bins of every dataset (ps_c / cnt_c; the empty bins enter through h_Tz), else
//   unb       pdf values at the events, no counts; by_set: several event sets side by side on the event axis, set t at
//             columns [set_first[t], set_first[t] + set_n[t]) of every row, else
//   the dense rows and counts.
struct ItemRoute {
    const bi_ctx* c;
    bool compact, unb, by_set;
    const double* ps;
    const double* counts;          // (unbinned: never read, any valid device address)

    // by_set: the caller addresses the event sets of an unbinned context by its dataset column (else: set 0, whose columns B counts)
    explicit ItemRoute(const bi_ctx* ctx, bool sets = false)
        : c(ctx), compact(ctx->sparse && ctx->compact_ready && ctx->ps_nonneg && !ctx->unbinned && ctx->bb_source < 0 && !any_negative_source(ctx)),
          unb(ctx->unbinned), by_set(sets && multi_set(ctx)),
          ps(compact ? (const double*)ctx->ps_c.p : (const double*)ctx->ps.p),
          counts(unb ? (const double*)ctx->ps.p : (compact ? (const double*)ctx->cnt_c.p : (const double*)ctx->counts.p)) {}

    // the dense rows whatever the context prefers (binned contexts; the real-valued store, which exists in dense form only)
    static ItemRoute dense(const bi_ctx* ctx) {
        ItemRoute rt(ctx);
        rt.compact = false;
        rt.ps = (const double*)ctx->ps.p;
        rt.counts = (const double*)ctx->counts.p;
        return rt;
    }

    bool has_counts() const { return unb || compact || c->dense_counts; }
    int64_t row_stride(int64_t ds) const { return compact ? c->h_c_np[(size_t)ds] : c->Bp; }
    int64_t row_base(int64_t ds) const { return compact ? c->h_c_off[(size_t)ds] : (by_set ? c->set_first[(size_t)ds] : 0); }
    // (several event sets: the item's tiles cover its own segment, and k_morph_sets takes the segment's length here)
    int64_t cnt_off(int64_t ds) const { return by_set ? c->set_n[(size_t)ds] : unb ? 0 : (compact ? c->h_cnt_off[(size_t)ds] : ds * c->Bp); }
    int32_t tiles(int64_t ds) const {
        return by_set ? (int32_t)std::max<int64_t>(1, (c->set_n[(size_t)ds] + kTile - 1) / kTile) : (int32_t)(row_stride(ds) / kTile);
    }
    // nontemporal loads of the dense rows of a launch of n_items items
    bool nt(int64_t n_items) const { return !compact && (c->nt_loads == 1 || (c->nt_loads == 2 && n_items == 1)); }
};

// screen_point over P points on a few host threads, reset(p) first (the caller's defaults for point p's outputs); status
// [P] (nullable) gets every point's bit.  dataset_test = false: the box and rate tests alone (what does not depend on the
// context's data), dataset is not read.  -> the points that pass, in order.
template <class F>
std::vector<int64_t> screen_points(const bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                                   int32_t* status, F reset, bool dataset_test = true) {
    std::vector<int32_t> st((size_t)P);
    parallel_for(P, 2048, [&](int64_t lo, int64_t hi) {
        PointGeom g;
        std::vector<double> r((size_t)c->S);
        for (int64_t p = lo; p < hi; ++p) {
            reset(p);
            const double* zp = z ? z + p * c->d : nullptr;
            const double* rs = rate_scale ? rate_scale + p * c->S : nullptr;
            st[(size_t)p] = dataset_test ? screen_point(c, zp, rs, dataset ? dataset[p] : 0, g, r.data()) : screen_point_rates(c, zp, rs, g, r.data());
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

    // descriptor row (corner, s): its row of the template tensor, and its value coefficient a_k = w_c r_s
    int64_t row(int corner, int s) const { return (g.cell_anchor + corner_off[(size_t)corner]) * S + s; }
    double value(int corner, int s) const { return g.w[(size_t)corner] * r[(size_t)s]; }

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
        lg[0] = rate_sum();
        for (int i = 0; i < de; ++i) {
            double v = 0.0;
            for (int s = 0; s < S; ++s) v += dmus[(size_t)i * S + s] * rs[s];
            lg[axis_col[i]] = v;
        }
        for (int s = 0; s < S; ++s) lg[rate_col0 + s] = mus[(size_t)s];
    }
    double rate_sum() const {
        double rsum = 0.0;
        for (int s = 0; s < S; ++s) rsum += r[(size_t)s];
        return rsum;
    }
};

// The tail of the one-item-per-point paths: n_items work items of nsl result slots, on nbx blocks each (at most max_tiles;
// about four blocks per CU slot in all).  Per chunk of at most 65 535 items (gridDim.y), launch(i0, grid, partial, pflags)
// points its kernel's arguments at items i0 ... and launches it on the grid; the kernel assigns every (item, block, slot)
// of partial / pflags, so the chunks, in order on one stream, share one chunk's buffers.  k_finish then adds the partials up
// into out[perm] - slot_lg (status |= their flag bits when given).  Synchronises the stream.  fixed_nbx > 0: that many blocks
// per item whatever the batch (the order in which an item's sums are added then does not depend on n_items).  The chunks
// launched are counted in last_point_pieces.
template <class L>
int run_item_chunks(bi_ctx* c, int64_t n_items, int max_tiles, int nsl, const int64_t* perm, const double* slot_lg, double* out,
                    int32_t* status, const char* what, L launch, int fixed_nbx = 0) {
    const int64_t slots = (int64_t)c->prop.multiProcessorCount * c->blocks_per_cu;
    const int nbx = fixed_nbx > 0 ? fixed_nbx
                                  : (int)std::min<int64_t>(max_tiles, n_items == 1 ? slots : std::max<int64_t>(1, (4 * slots + n_items - 1) / n_items));
    const int64_t chunk = 65535, part_items = std::min(chunk, n_items);
    ScratchBuf d_part, d_flag;
    int rc;
    if ((rc = dev_alloc(c, d_part, (size_t)part_items * nbx * nsl * sizeof(double))) ||
        (rc = dev_alloc(c, d_flag, (size_t)part_items * nbx * nsl * sizeof(unsigned)))) return rc;
    hipError_t e = hipSuccess;
    c->last_point_pieces = 0;
    for (int64_t i0 = 0; i0 < n_items && e == hipSuccess; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        if ((rc = launch(i0, dim3((unsigned)nbx, (unsigned)ni), (double*)d_part.p, (unsigned*)d_flag.p))) return rc;
        ++c->last_point_pieces;
        launch_finish(c, (const double*)d_part.p, (const unsigned*)d_flag.p, nbx, nsl, ni * nsl, perm + i0 * nsl, slot_lg + i0 * nsl,
                      out, status);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return BI_OK;
}

// The descriptors of one work item per live point, NS = 2^d_eff * S corner rows of G coefficient columns each and nsl result
// slots, of which the first n_out are wanted (k_finish writes item i's to out[i * n_out ...], the others nowhere):
//   rowoff [n][NS]   row_base + row * row_stride of the item's dataset (ItemRoute)
//   coef [n][NS][G]  the caller's columns (zero where it writes none)
//   cnt_off, tiles   [n] the dataset's counts and tiles (ItemRoute)
//   perm, slot_lg    [n][nsl] where a slot's sum goes and what k_finish subtracts from it
struct ItemBatch {
    const std::vector<int64_t>& live;
    int64_t n_items;
    int NS, G, nsl, n_out;
    std::vector<int64_t> rowoff, cnt_off, perm;
    std::vector<double> coef, slot_lg;
    std::vector<int32_t> tiles;
    int max_tiles = 1;
    PackedUpload pu;

    ItemBatch(const bi_ctx* c, const std::vector<int64_t>& live_points, int G_, int nsl_, int n_out_)
        : live(live_points), n_items((int64_t)live_points.size()), NS((1 << (int)c->eff_axes.size()) * c->S), G(G_), nsl(nsl_), n_out(n_out_),
          rowoff((size_t)n_items * NS), cnt_off((size_t)n_items), perm((size_t)n_items * nsl, -1), coef((size_t)n_items * NS * G, 0.0),
          slot_lg((size_t)n_items * nsl, 0.0), tiles((size_t)n_items) {}

    // Fills the arrays on host threads (grain items per task).  Per item, in this order: row(pd, col, corner, s) writes the
    // coefficient columns of every corner row; on the compacted route the first n_lg slot constants gather col[q] * Tz[ds, row]
    // over the rows; item(pd, lg, ds) then finishes the item's slot constants lg [nsl].
    template <class Row, class Item>
    void fill(const ItemRoute& rt, const double* z, const double* rate_scale, const int64_t* dataset, bool second_order, int64_t grain,
              int n_lg, Row row, Item item) {
        const bi_ctx* c = rt.c;
        const int64_t n_rows = c->A * c->S;
        parallel_for(n_items, grain, [&](int64_t lo, int64_t hi) {
            PointDerivs pd(c, second_order);
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t p = live[(size_t)i];
                const int64_t ds = dataset ? dataset[p] : 0;
                pd.at(z ? z + p * c->d : nullptr, rate_scale ? rate_scale + p * c->S : nullptr);
                const int64_t row_stride = rt.row_stride(ds), row_base = rt.row_base(ds);
                const size_t ro = (size_t)i * NS, co = (size_t)i * NS * G, po = (size_t)i * nsl;
                int k = 0;
                for (int corner = 0; corner < pd.nc; ++corner)
                    for (int s = 0; s < pd.S; ++s, ++k) {
                        const int64_t r = pd.row(corner, s);
                        rowoff[ro + k] = row_base + r * row_stride;
                        double* col = &coef[co + (size_t)k * G];
                        row(pd, col, corner, s);
                        if (rt.compact) {
                            const double tz = c->h_Tz[(size_t)(ds * n_rows + r)];
                            for (int q = 0; q < n_lg; ++q) slot_lg[po + q] += col[q] * tz;
                        }
                    }
                item(pd, &slot_lg[po], ds);
                for (int q = 0; q < n_out; ++q) perm[po + q] = i * n_out + q;
                cnt_off[(size_t)i] = rt.cnt_off(ds);
                tiles[(size_t)i] = rt.tiles(ds);
            }
        });
        for (int32_t t : tiles) max_tiles = std::max(max_tiles, (int)t);
    }

    // descriptors: one packed copy; results: k_finish writes them straight into pinned host memory (out())
    int upload(bi_ctx* c) {
        return packed_upload(c, {{rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)},
                                 {cnt_off.data(), cnt_off.size() * sizeof(int64_t)}, {tiles.data(), tiles.size() * sizeof(int32_t)},
                                 {perm.data(), perm.size() * sizeof(int64_t)}, {slot_lg.data(), slot_lg.size() * sizeof(double)}},
                             (size_t)n_items * n_out * sizeof(double), pu);
    }
    const double* out(int64_t i) const { return (const double*)pu.host_out() + (size_t)i * n_out; }      // item i's n_out results

    // run_item_chunks with a copy of `a` (LaunchArgs or HessArgs) pointed at every chunk's items: launch(b, grid) -> error code
    template <class Args, class L>
    int run(bi_ctx* c, const Args& a, const char* what, L launch) const {
        return run_item_chunks(c, n_items, max_tiles, nsl, pu.dev<int64_t>(4), pu.dev<double>(5), (double*)pu.host_out(), nullptr, what,
                               [&](int64_t i0, dim3 grid, double* partial, unsigned* pflags) {
                                   Args b = a;
                                   b.rowoff = pu.dev<int64_t>(0) + i0 * NS;
                                   b.coef = pu.dev<double>(1) + i0 * NS * G;
                                   b.item_cnt = pu.dev<int64_t>(2) + i0;
                                   b.item_tiles = pu.dev<int32_t>(3) + i0;
                                   b.partial = partial;
                                   b.pflags = pflags;
                                   return launch(b, grid);
                               });
    }
};

// The value-only descriptors of kernels that write bins: for the n points live[i] (nullptr: the points 0 ... n - 1), the rows
// of the dense tensor, rowoff [n][NS] = row * Bp, and coef [n][NS] = a_k = w_c r_s (PointDerivs::value: the bits of column 0
// of every other path)
void fill_value_rows(PointDerivs& pd, const int64_t* live, int64_t n, const double* z, const double* rate_scale, int64_t* rowoff,
                     double* coef) {
    const bi_ctx* c = pd.c;
    for (int64_t i = 0, k = 0; i < n; ++i) {
        const int64_t p = live ? live[i] : i;
        pd.at(z ? z + p * c->d : nullptr, rate_scale ? rate_scale + p * c->S : nullptr);
        for (int corner = 0; corner < pd.nc; ++corner)
            for (int s = 0; s < pd.S; ++s, ++k) {
                rowoff[k] = pd.row(corner, s) * c->Bp;
                coef[k] = pd.value(corner, s);
            }
    }
}

// d_out [n][per_item] (device), the results of the points live[0 ... n), -> out[live[i]]: runs of consecutive live points are
// consecutive in `out` too, one copy each.  e: the error state so far (nothing is copied after an error).  Synchronises the
// stream either way.
hipError_t download_live_runs(bi_ctx* c, const int64_t* live, int64_t n, const double* d_out, int64_t per_item, double* out, hipError_t e) {
    for (int64_t i = 0; i < n && e == hipSuccess;) {
        int64_t j = i + 1;
        while (j < n && live[j] == live[j - 1] + 1) ++j;
        e = hipMemcpyAsync(out + live[i] * per_item, d_out + i * per_item, (size_t)((j - i) * per_item) * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream);
        i = j;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    return e;
}

}  // namespace
