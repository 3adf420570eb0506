// bi_coarse.h -- bi_set_coarse_binning, bi_expected_coarse and bi_coarse_counts (host half; the kernels are k_morph_coarse,
// k_coarse_finish and k_coarse_list, bi_k_coarse.h).
//
// A coarse binning is a tensor product of groups of adjacent fine bins, one list of boundaries e_0 < ... < e_m per analysis
// axis; fine bins below e_0 or from e_m on belong to no cell.  With b = r L + x (x on the last axis) the binning becomes, once:
//     the fine rows of every coarse row in CSR form (ascending inside a coarse row, left-out rows absent), row_map [NR],
//     the boundaries of the column groups xb [Cx + 1] and x_map [L].
// bi_expected_coarse: per live point the value rows of bi_items.h, bi_expected_counts's (row offsets and a_k = w_corner r_source
// of the 2^d_eff S corner rows), one launch pair and one download of the live runs per chunk of points; the chunk is sized so that the x-resolved partial sums of
// k_morph_coarse and the output stay within ~64 MB each.  bi_expected_coarse_jacobian: the same with the G = 1 + D padded
// first-order columns of bi_fisher.h per corner row (ItemBatch / PointDerivs::first_order) and k_morph_coarse_jac<G>, whose G
// columns the finish kernels take for R = G groups of rows: mu and d mu / d theta of every cell.  bi_coarse_counts: the dense counts rows through the same kernels,
// or the non-empty-bin lists through k_coarse_list where only those exist.
// The builder of a binning (coarse_build), the launch geometry, the chunks and the launch pair take the binning they work on as
// an argument: bi_sourcewise_coarse.h runs them over the source-wise store's own binning (bi_ctx::sw_coarse).
#pragma once

namespace {

constexpr int kCoarseBlocksPerCu = 4;      // blocks per CU that k_morph_coarse's grid aims at for ONE (point, group of rows)

// The launch geometry of k_morph_coarse, from the binning and the device alone (never from the number of points: the order of
// every sum, and with it the last bits of a point's result, must not depend on the batch the point came in):
//   TX = 64, 128 or 256 lanes along x, the smallest that covers the Lx live columns (256 with several x-tiles);
//   nsplit shares per coarse row, enough for kCoarseBlocksPerCu blocks per CU, each sub-row keeping at least 4 fine rows.
//   wide: the finish kernel that gives a cell a block instead of a thread, where a cell gathers at least kCoarseWide partials.
constexpr int64_t kCoarseWide = 256;      // (at least one partial per thread of the block)
struct CoarseGeometry {
    int tx_shift, n_xt, nsplit, wide;
};

CoarseGeometry coarse_geometry(const bi_ctx* c, const bi_ctx::Coarse& q) {
    CoarseGeometry g;
    g.tx_shift = q.Lx <= 64 ? 6 : (q.Lx <= 128 ? 7 : 8);
    const int64_t TX = (int64_t)1 << g.tx_shift, TY = kThreads >> g.tx_shift;
    g.n_xt = (int)((q.Lx + TX - 1) / TX);
    const int64_t blocks = q.CR * g.n_xt;
    const int64_t want = ((int64_t)kCoarseBlocksPerCu * std::max(1, c->prop.multiProcessorCount) + blocks - 1) / blocks;
    g.nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(want, q.max_rows / (4 * TY)));
    g.wide = g.nsplit * q.max_width >= kCoarseWide ? 1 : 0;
    return g;
}

int coarse_check(bi_ctx* c, const char* what, bool need_data) {
    int rc = gof_check(c, what, need_data);
    if (rc) return rc;
    if (!c->coarse.set) return fail(c, BI_ERR_STATE, "%s: no coarse binning is set (bi_set_coarse_binning first; a new model releases it)", what);
    return BI_OK;
}

// the arguments of one launch pair over n_items items whose descriptors lie at rowoff / coef (device): partial -> d_out [n_items][R][C];
// q: the binning, the grid model's (c->coarse) or the source-wise store's (c->sw_coarse)
CoarseArgs coarse_args(bi_ctx* c, const bi_ctx::Coarse& q, const double* rows, const int64_t* rowoff, const double* coef, int NS, int S, int R,
                       int64_t n_items, double* partial, double* d_out) {
    const CoarseGeometry g = coarse_geometry(c, q);
    CoarseArgs a{};
    a.ps = rows; a.rowoff = rowoff; a.coef = coef;
    a.row_off = (const int64_t*)q.row_off.p; a.row_list = (const int32_t*)q.row_list.p; a.xb = (const int32_t*)q.xb.p;
    a.partial = partial; a.out = d_out;
    a.L = q.L; a.x_lo = q.x_lo; a.Lx = q.Lx; a.CR = q.CR; a.Cx = q.Cx;
    a.n_out = n_items * R * q.C;
    a.NS = NS; a.S = S; a.R = R;
    a.nsplit = g.nsplit; a.n_xt = g.n_xt; a.tx_shift = g.tx_shift; a.wide = g.wide;
    return a;
}

void coarse_launch(bi_ctx* c, const bi_ctx::Coarse& q, const double* rows, const int64_t* rowoff, const double* coef, int NS, int S, int R,
                   int64_t n_items, double* partial, double* d_out) {
    launch_morph_coarse(c, coarse_args(c, q, rows, rowoff, coef, NS, S, R, n_items, partial, d_out), n_items);
}

// items per launch: the partial sums and the output of a chunk within ~64 MB each, a launch at most 32 768 items
int64_t coarse_chunk(const bi_ctx* c, const bi_ctx::Coarse& q, int64_t n_items, int R) {
    const int64_t per_item = std::max<int64_t>((int64_t)R * q.CR * coarse_geometry(c, q).nsplit * q.Lx, (int64_t)R * q.C);
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_items, 32768), ((int64_t)1 << 23) / per_item));
}

// What bi_set_coarse_binning and bi_sourcewise_set_coarse_binning (bi_sourcewise_coarse.h) share: the checks of the axes against the
// B fine bins of the caller's model, the per-axis group maps, the CSR of fine rows per coarse row, xb and the launch-size check,
// into the binning q (the grid model's or the source-wise store's).  The caller has checked that its model is ready.
int coarse_build(bi_ctx* c, bi_ctx::Coarse& q, const char* who, int64_t B, int k, const int32_t* n_fine, const int32_t* n_groups,
                 const int32_t* bounds, int64_t* n_cells) {
    int rc;
    if (k < 1 || k > kMaxDim || !n_fine || !n_groups || !bounds) return fail(c, BI_ERR_INVALID, "%s: need 0..%d axes with their bins, groups and boundaries", who, kMaxDim);
    int64_t bins = 1;
    int off[kMaxDim];
    for (int j = 0, at = 0; j < k; ++j) {
        if (n_fine[j] < 1) return fail(c, BI_ERR_INVALID, "%s: axis %d has %d fine bins", who, j, n_fine[j]);
        if (n_groups[j] < 1) return fail(c, BI_ERR_INVALID, "%s: axis %d has %d groups (need >= 1)", who, j, n_groups[j]);
        if (n_groups[j] > n_fine[j]) return fail(c, BI_ERR_INVALID, "%s: axis %d has more groups (%d) than fine bins (%d)", who, j, n_groups[j], n_fine[j]);
        const int32_t* e = bounds + at;
        if (e[0] < 0 || e[n_groups[j]] > n_fine[j])
            return fail(c, BI_ERR_INVALID, "%s: the boundaries of axis %d leave [0, %d]", who, j, n_fine[j]);
        for (int i = 1; i <= n_groups[j]; ++i)
            if (!(e[i] > e[i - 1])) return fail(c, BI_ERR_INVALID, "%s: the boundaries of axis %d are not strictly ascending", who, j);
        off[j] = at;
        at += n_groups[j] + 1;
        bins *= n_fine[j];
        if (bins > B) break;         // (already too many: the product cannot overflow)
    }
    if (bins != B) return fail(c, BI_ERR_INVALID, "%s: the axes have %s%lld fine bins, the model %lld", who, bins > B ? "more than " : "", (long long)std::min(bins, B), (long long)B);
    const int64_t L = n_fine[k - 1], NR = B / L;
    if (NR > (int64_t)std::numeric_limits<int32_t>::max()) return fail(c, BI_ERR_INVALID, "%s: %lld fine rows are more than a 32-bit index holds", who, (long long)NR);
    HIP_TRY(c, hipSetDevice(c->device));
    release_coarse(q);

    // fine index -> group (-1: left out), per axis
    std::vector<std::vector<int32_t>> group_of((size_t)k);
    for (int j = 0; j < k; ++j) {
        group_of[(size_t)j].assign((size_t)n_fine[j], -1);
        const int32_t* e = bounds + off[j];
        for (int g = 0; g < n_groups[j]; ++g)
            for (int32_t i = e[g]; i < e[g + 1]; ++i) group_of[(size_t)j][(size_t)i] = g;
    }
    q.L = L; q.NR = NR;
    q.Cx = n_groups[k - 1];
    q.CR = 1;
    for (int j = 0; j + 1 < k; ++j) q.CR *= n_groups[j];
    q.C = q.CR * q.Cx;
    const int32_t* ex = bounds + off[k - 1];
    q.x_lo = ex[0];
    q.Lx = ex[q.Cx] - ex[0];
    const std::vector<int32_t> xb(ex, ex + q.Cx + 1);
    q.max_width = 0;
    for (int64_t j = 0; j < q.Cx; ++j) q.max_width = std::max<int64_t>(q.max_width, ex[j + 1] - ex[j]);

    // fine row -> coarse row, walking the leading axes in C order
    std::vector<int32_t> row_map((size_t)NR);
    {
        std::vector<int32_t> at((size_t)std::max(k - 1, 1), 0);
        for (int64_t r = 0; r < NR; ++r) {
            int64_t cr = 0;
            for (int j = 0; j + 1 < k && cr >= 0; ++j) {
                const int32_t g = group_of[(size_t)j][(size_t)at[(size_t)j]];
                cr = g < 0 ? -1 : cr * n_groups[j] + g;
            }
            row_map[(size_t)r] = (int32_t)cr;
            for (int j = k - 2; j >= 0; --j) {
                if (++at[(size_t)j] < n_fine[j]) break;
                at[(size_t)j] = 0;
            }
        }
    }
    std::vector<int64_t> row_off((size_t)q.CR + 1, 0);
    for (int64_t r = 0; r < NR; ++r)
        if (row_map[(size_t)r] >= 0) ++row_off[(size_t)row_map[(size_t)r] + 1];
    q.max_rows = 0;
    for (int64_t i = 0; i < q.CR; ++i) {
        q.max_rows = std::max(q.max_rows, row_off[(size_t)i + 1]);
        row_off[(size_t)i + 1] += row_off[(size_t)i];
    }
    std::vector<int32_t> row_list((size_t)std::max<int64_t>(row_off[(size_t)q.CR], 1), 0);
    {
        std::vector<int64_t> fill(row_off.begin(), row_off.end() - 1);
        for (int64_t r = 0; r < NR; ++r)
            if (row_map[(size_t)r] >= 0) row_list[(size_t)fill[(size_t)row_map[(size_t)r]]++] = (int32_t)r;
    }
    if ((rc = dev_upload(c, q.row_off, row_off)) || (rc = dev_upload(c, q.row_list, row_list)) || (rc = dev_upload(c, q.xb, xb)) ||
        (rc = dev_upload(c, q.row_map, row_map)) || (rc = dev_upload(c, q.x_map, group_of[(size_t)k - 1]))) {
        (void)hipStreamSynchronize(c->stream);
        release_coarse(q);
        return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the host vectors are alive until here)
    q.set = true;
    const CoarseGeometry g = coarse_geometry(c, q);
    // (a launch's threads along x must stay below 2^32: 2^24 blocks of 256)
    if (q.CR * g.nsplit * g.n_xt >= ((int64_t)1 << 32) / kThreads) {
        release_coarse(q);
        return fail(c, BI_ERR_INVALID, "%s: %lld coarse rows x %d x-tiles are more blocks than one launch holds (2^24)", who,
                    (long long)q.CR, g.n_xt);
    }
    if (n_cells) *n_cells = q.C;
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_set_coarse_binning(bi_ctx* c, int k, const int32_t* n_fine, const int32_t* n_groups, const int32_t* bounds, int64_t* n_cells) {
    if (!c) return BI_ERR_INVALID;
    if (n_cells) *n_cells = 0;
    if (k == 0) {
        if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
        HIP_TRY(c, hipSetDevice(c->device));
        release_coarse(c);
        return BI_OK;
    }
    int rc = gof_check(c, "bi_set_coarse_binning", false);
    if (rc) return rc;
    return coarse_build(c, c->coarse, "bi_set_coarse_binning", c->B, k, n_fine, n_groups, bounds, n_cells);
}

int bi_expected_coarse(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int per_source, double* out, int32_t* status) {
    int rc = coarse_check(c, "bi_expected_coarse", false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !out)) return fail(c, BI_ERR_INVALID, "bad P / output pointer");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    const int S = c->S;
    const int de = (int)c->eff_axes.size();
    const int NS = (1 << de) * S, R = per_source ? S : 1;
    const int64_t per_item = (int64_t)R * c->coarse.C;
    HIP_TRY(c, hipSetDevice(c->device));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    // the screen of bi_expected_counts (no dataset test); here the bit is reported too
    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, nullptr, status,
                                                    [&](int64_t p) { std::fill(out + p * per_item, out + (p + 1) * per_item, qnan); }, false);
    const int64_t n_items = (int64_t)live.size();
    c->last_point_pieces = 0;
    if (n_items == 0) return BI_OK;
    const int64_t chunk = coarse_chunk(c, c->coarse, n_items, R);
    const CoarseGeometry geo = coarse_geometry(c, c->coarse);
    ScratchBuf d_partial, d_out;
    if ((rc = dev_alloc(c, d_partial, (size_t)(chunk * R * c->coarse.CR * geo.nsplit * c->coarse.Lx) * sizeof(double))) ||
        (rc = dev_alloc(c, d_out, (size_t)(chunk * per_item) * sizeof(double)))) return rc;
    std::vector<int64_t> rowoff((size_t)chunk * NS);
    std::vector<double> coef((size_t)chunk * NS);
    PointDerivs pd(c, false);
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        fill_value_rows(pd, &live[(size_t)i0], ni, z, rate_scale, rowoff.data(), coef.data());
        PackedUpload pu;
        if ((rc = packed_upload(c, {{rowoff.data(), (size_t)ni * NS * sizeof(int64_t)}, {coef.data(), (size_t)ni * NS * sizeof(double)}}, 0, pu)))
            return rc;
        coarse_launch(c, c->coarse, (const double*)c->ps.p, pu.dev<int64_t>(0), pu.dev<double>(1), NS, S, R, ni, (double*)d_partial.p, (double*)d_out.p);
        ++c->last_point_pieces;
        // (the staging block of packed_upload, d_partial and d_out are reused by the next chunk: the download synchronises)
        const hipError_t e = download_live_runs(c, &live[(size_t)i0], ni, (const double*)d_out.p, per_item, out, hipGetLastError());
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_expected_coarse: %s", hipGetErrorString(e));
    }
    return BI_OK;
}

int bi_expected_coarse_jacobian(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, double* mu, double* jac, int32_t* status) {
    int rc = coarse_check(c, "bi_expected_coarse_jacobian", false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!mu || !jac))) return fail(c, BI_ERR_INVALID, "bad P / output pointer");
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    const int S = c->S, d = c->d;
    const int de = (int)c->eff_axes.size();
    const int D = de + S, F = d + S;
    int G, DM;
    if (!fisher_variant(D, G, DM))
        return fail(c, BI_ERR_INVALID, "bi_expected_coarse_jacobian: 1 + d_eff + S = %d exceeds %d coefficient columns", 1 + D, kMaxG);
    const int NS = (1 << de) * S;
    const int64_t C = c->coarse.C;
    HIP_TRY(c, hipSetDevice(c->device));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<int64_t> live = screen_points(c, P, z, rate_scale, nullptr, status, [&](int64_t p) {
        std::fill(mu + p * C, mu + (p + 1) * C, qnan);
        std::fill(jac + p * F * C, jac + (p + 1) * F * C, qnan);
    }, false);
    const int64_t n_items = (int64_t)live.size();
    c->last_point_pieces = 0;
    if (n_items == 0) return BI_OK;

    // full parameter index of first-order index q, and the columns of the effective axes (bi_fisher.h's)
    std::vector<int> full((size_t)D), axis_col((size_t)de);
    for (int q = 0; q < D; ++q) full[(size_t)q] = q < de ? c->eff_axes[(size_t)q] : d + (q - de);
    for (int i = 0; i < de; ++i) axis_col[(size_t)i] = 1 + i;
    const ItemRoute rt = ItemRoute::dense(c);
    const int64_t chunk = coarse_chunk(c, c->coarse, n_items, G);
    const CoarseGeometry geo = coarse_geometry(c, c->coarse);
    ScratchBuf d_partial, d_out;
    if ((rc = dev_alloc(c, d_partial, (size_t)(chunk * G * c->coarse.CR * geo.nsplit * c->coarse.Lx) * sizeof(double))) ||
        (rc = dev_alloc(c, d_out, (size_t)(chunk * G * C) * sizeof(double)))) return rc;
    // The device holds a chunk's cells as [item][G][C], the padded columns; the caller's arrays are [P][C] and [P][F][C].  The
    // chunk comes down as one run and is dealt out here.
    std::vector<double> stage((size_t)(chunk * G * C));
    std::vector<int64_t> run((size_t)chunk);
    for (int64_t i = 0; i < chunk; ++i) run[(size_t)i] = i;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        const std::vector<int64_t> part(live.begin() + i0, live.begin() + i0 + ni);
        ItemBatch batch(c, part, G, 1, 0);                 // (rowoff and coef are what is used: no result slot is wanted)
        batch.fill(rt, z, rate_scale, nullptr, false, 1024, 0,
                   [&](const PointDerivs& pd, double* col, int corner, int s) { pd.first_order(col, corner, s, axis_col.data(), 1 + de + s); },
                   [](const PointDerivs&, double*, int64_t) {});
        if ((rc = batch.upload(c))) return rc;
        const CoarseArgs a = coarse_args(c, c->coarse, rt.ps, batch.pu.dev<int64_t>(0), batch.pu.dev<double>(1), NS, S, G, ni, (double*)d_partial.p,
                                         (double*)d_out.p);
        if (launch_morph_coarse_jac(c, G, a, ni)) return fail(c, BI_ERR_INVALID, "bi_expected_coarse_jacobian: no kernel variant for G = %d", G);
        ++c->last_point_pieces;
        // (the staging block of the batch, d_partial and d_out are reused by the next chunk: the download synchronises)
        const hipError_t e = download_live_runs(c, run.data(), ni, (const double*)d_out.p, (int64_t)G * C, stage.data(), hipGetLastError());
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_expected_coarse_jacobian: %s", hipGetErrorString(e));
        parallel_for(ni, 64, [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t p = part[(size_t)i];
                const double* h = stage.data() + i * G * C;
                std::copy(h, h + C, mu + p * C);
                std::fill(jac + p * F * C, jac + (p + 1) * F * C, 0.0);            // rows of single-anchor axes stay zero
                for (int q = 0; q < D; ++q) std::copy(h + (1 + q) * C, h + (2 + q) * C, jac + (p * F + full[(size_t)q]) * C);
            }
        });
    }
    return BI_OK;
}

int bi_coarse_counts(bi_ctx* c, int64_t n, const int64_t* dataset, double* out) {
    int rc = coarse_check(c, "bi_coarse_counts", true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !out)) return fail(c, BI_ERR_INVALID, "bad n / output pointer");
    if (!dataset && n != c->T) return fail(c, BI_ERR_INVALID, "bi_coarse_counts: without a dataset list n must be the %lld resident datasets (got %lld)", (long long)c->T, (long long)n);
    for (int64_t i = 0; dataset && i < n; ++i)
        if (dataset[i] < 0 || dataset[i] >= c->T)
            return fail(c, BI_ERR_INVALID, "bi_coarse_counts: dataset %lld outside [0,%lld)", (long long)dataset[i], (long long)c->T);
    if (!c->dense_counts && !c->csr_ready) return fail(c, BI_ERR_STATE, "no counts resident");
    c->last_point_pieces = 0;
    if (n == 0) return BI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const bi_ctx::Coarse& q = c->coarse;
    const bool dense = c->dense_counts;
    const int64_t chunk = dense ? coarse_chunk(c, c->coarse, n, 1) : std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n, 32768), ((int64_t)1 << 23) / q.C));
    ScratchBuf d_partial, d_out, d_table;
    if ((rc = dev_alloc(c, d_out, (size_t)(chunk * q.C) * sizeof(double)))) return rc;
    if (dense && (rc = dev_alloc(c, d_partial, (size_t)(chunk * q.CR * coarse_geometry(c, q).nsplit * q.Lx) * sizeof(double)))) return rc;
    if (!dense && (rc = dev_alloc(c, d_table, (size_t)(chunk * q.C) * sizeof(unsigned long long)))) return rc;
    std::vector<int64_t> first((size_t)chunk);        // dense: the element offset of the dataset's counts row; lists: the dataset
    const std::vector<double> ones(dense ? (size_t)chunk : 0, 1.0);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t ni = std::min(chunk, n - i0);
        for (int64_t i = 0; i < ni; ++i) {
            const int64_t t = dataset ? dataset[i0 + i] : i0 + i;
            first[(size_t)i] = dense ? t * c->Bp : t;
        }
        PackedUpload pu;            // (the coefficients a_0 = 1 are the dense path's alone)
        if ((rc = packed_upload(c, {{first.data(), (size_t)ni * sizeof(int64_t)}, {ones.data(), dense ? (size_t)ni * sizeof(double) : 0}}, 0, pu))) return rc;
        hipError_t e = hipSuccess;
        if (dense) {
            coarse_launch(c, q, (const double*)c->counts.p, pu.dev<int64_t>(0), pu.dev<double>(1), 1, 1, 1, ni, (double*)d_partial.p, (double*)d_out.p);
        } else {
            e = hipMemsetAsync(d_table.p, 0, (size_t)(ni * q.C) * sizeof(unsigned long long), c->stream);
            CoarseListArgs a{};
            a.nz_idx = (const int32_t*)c->nz_idx.p; a.nz_n = (const double*)c->nz_n.p; a.nz_off = (const int64_t*)c->nz_off.p;
            a.dataset = pu.dev<int64_t>(0);
            a.row_map = (const int32_t*)q.row_map.p; a.x_map = (const int32_t*)q.x_map.p;
            a.table = (unsigned long long*)d_table.p;
            a.L = q.L; a.Cx = q.Cx; a.C = q.C;
            if (e == hipSuccess) launch_coarse_list(c, a, ni, (double*)d_out.p);
        }
        ++c->last_point_pieces;
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + i0 * q.C, d_out.p, (size_t)(ni * q.C) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        else (void)hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_coarse_counts: %s", hipGetErrorString(e));
    }
    return BI_OK;
}

}  // extern "C"
