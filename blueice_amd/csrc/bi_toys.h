// bi_toys.h -- the host half of the toy-MC EVALUATION: bi_eval_datasets (one parameter point against many datasets) and
// bi_eval_datasets_points (several points), with their _device forms.  The kernels are bi_k_toys.h (tu_toys.hip).
//
// What the multi-point form replaces.  The reference's toy-MC users evaluate every toy dataset at many hypotheses -- the loops of
// blueice/inference.py:392-443 (one likelihood call per hypothesis and dataset) around blueice/model.py:69-91 (simulate, set_data).
// bi_eval_datasets takes ONE point: P hypotheses were P calls, each streaming the T datasets' non-empty-bin lists (188 MB at
// BASELINE.json configs[2]) and each paying its own log mu pass (264 MB), its own three launches and its own wait.  Here:
//   (1) k_morph_logmu_multi<GC>: the points are ordered by grid cell and chopped into PASSES of PP = 4 (or 2) points, the passes
//       into groups of two; the points of a GROUP (GC = 2 PP) that share a cell share ONE pass over the cell's 2^d S template
//       rows (hypotheses that differ in their rates only -- the usual signal-strength scan -- always do); log mu is written one
//       row per point, lm[pass][PP][Bp] (coalesced stores whatever the cells; the dot kernel interleaves the PP rows of its tile
//       as it stages them);
//   (2) k_dataset_dot_multi<L, AHEAD, W, PP>: ONE pass over the tile-major entry lists per pass of points: a block stages the
//       log mu of its bin tile for all PP points side by side in LDS (4096 bins x 4 points x 8 B = 128 KB of the CU's 160 KB) and
//       an entry's one LDS address yields PP values (PP / 2 ds_read_b128): the 188 MB entry stream, the offsets, the decode and
//       the run bookkeeping are paid once per PP evaluations of a dataset;
//   (3) k_dataset_finish_multi: per (point, dataset) the tiles' partial sums in tile order, minus sum mu of the point and
//       sum lgamma of the dataset -- a fixed order, bitwise reproducible -- into out[point][dataset] in the caller's point order.
// Algorithmic bytes per call: 8 (2^d S) B per distinct grid cell of a group of passes + 8 PP B (log mu written and staged once) per pass
// + W bytes per list entry per PASS (not per point).
#pragma once

namespace {

// The 2^d S stream rows of a screened point and their coefficients w_corner * rate_source, k = corner * S + source: rowoff[k]
// (or NULL: the rows of another point of the same cell are in place already) and coef[k * stride + column].
void point_streams(const bi_ctx* c, const PointGeom& g, const double* rates, int64_t* rowoff, double* coef, int stride = 1, int column = 0) {
    int k = 0;
    for (int corner = 0; corner < (int)g.w.size(); ++corner)
        for (int s = 0; s < c->S; ++s, ++k) {
            if (rowoff) rowoff[k] = ((g.cell_anchor + corner_offset(c, corner)) * c->S + s) * c->Bp;
            coef[(size_t)k * stride + column] = g.w[(size_t)corner] * rates[s];
        }
}

// The argument checks of the toy-MC entry points, `what` at P points (the single-point form: P = 1)
int check_toy_call(bi_ctx* c, const char* what, int64_t P, const double* z, int64_t t0, int64_t t1, const double* out, const double* out_dev) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (c->bb_source >= 0) return fail(c, BI_ERR_INVALID, "%s is not available with Beeston-Barlow", what);
    if (multi_set(c)) return refuse_sets(c, what);
    if (c->unbinned) return fail(c, BI_ERR_INVALID, "%s needs a binned likelihood", what);
    if (P < 0 || P > 65535) return fail(c, BI_ERR_INVALID, "P = %lld outside [0, 65535]", (long long)P);
    if (t0 < 0 || t1 > c->T || t0 > t1) return fail(c, BI_ERR_INVALID, "dataset range [%lld,%lld) outside [0,%lld)", (long long)t0, (long long)t1, (long long)c->T);
    if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    if (P > 0 && t1 > t0 && !out && !out_dev) return fail(c, BI_ERR_INVALID, "out is NULL");
    return BI_OK;
}

// The completion word of a toy-MC call: the last block of the call's last finish kernel publishes a sequence number in the
// pinned block, behind the results if they go there (packed_upload keeps 64 spare bytes behind them), and the call polls that
// word (as single evaluations do) instead of synchronising the stream.
struct ToyDone {
    unsigned long long* word = nullptr;
    unsigned long long seq = 0;
    bool arrived = false;
    // the finish kernels' block counter (zeroed once: the publishing block leaves it at zero), the word's place, the next number
    int arm(bi_ctx* c, const PackedUpload& pu, size_t result_bytes) {
        int rc;
        if ((rc = dev_alloc(c, c->toy_blocks_done, 64))) return rc;
        if (!c->toy_blocks_done_zeroed) {
            HIP_TRY(c, hipMemsetAsync(c->toy_blocks_done.p, 0, 64, c->stream));
            c->toy_blocks_done_zeroed = true;
        }
        word = (unsigned long long*)((char*)pu.host_out() + (result_bytes + 63) / 64 * 64);
        seq = ++c->toy_seq;
        *(volatile unsigned long long*)word = 0ull;
        return BI_OK;
    }
    // The word arrives ~0.1 ms after the launches for 10^4 datasets: spin for the first ~30 us, then give the core away between
    // looks, and leave it to the stream synchronise after a time that scales with the work: 2 ms + 1 us per evaluation, at most 50 ms.
    void wait(bi_ctx* c, int64_t evaluations) {
        arrived = wait_word(word, seq, std::chrono::microseconds(30), std::chrono::microseconds(std::min<int64_t>(50000, 2000 + evaluations)));
        ++c->n_toy_polled;
    }
    // (falls back to the stream sync, which also reports a faulted kernel; every 256th call synchronises anyway, so the
    //  runtime retires its completed commands at a steady pace)
    bool must_sync() const { return !arrived || (seq & 255ull) == 0; }
    // (a completion word that never came -- a launch that failed part way -- leaves the finish kernel's block counter in an
    //  unknown state: it is zeroed again before the next call, which would otherwise wait out its 50 ms every time)
    void close(bi_ctx* c) const {
        if (word && !arrived) c->toy_blocks_done_zeroed = false;
    }
};

// Tile-major copy of the context's non-empty-bin lists for tiles of `tile_bins` bins (a power of two, at most kDotTile): the
// entries of bin tile 0 (dataset 0, 1, ...), then tile 1, ... -- see k_tm_scatter.  Two-byte entries where every count is at
// most 7 (toys of sparse expectations), four-byte entries otherwise; ok = false (and nothing kept) when some count fits neither.
int build_tile_major(bi_ctx* c, int tile_bins, DevBuf& entries, DevBuf& off, bool& ok, int& width_out) {
    int tile_shift = 0;
    while ((1 << tile_shift) < tile_bins) ++tile_shift;
    const int n_tl = (int)((c->B + tile_bins - 1) / tile_bins);
    const int64_t nnz = c->h_nz_off.back(), cells = (int64_t)n_tl * c->T;
    const uint32_t pad_entry = (uint32_t)tile_bins << 3;          // four-byte lists: the offset of the extra LDS slot behind the tile (0.0), count 0
    int rc;
    ScratchBuf d_tile, d_cnt, d_tmp, d_bad;
    size_t scan_bytes = 0;
    (void)prim_exclusive_scan_sum(nullptr, scan_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(cells + 1), c->stream);
    if ((rc = dev_alloc(c, d_tile, (size_t)c->T * (n_tl + 1) * sizeof(int32_t))) || (rc = dev_alloc(c, d_cnt, (size_t)(cells + 1) * sizeof(int64_t))) ||
        (rc = dev_alloc(c, d_tmp, std::max<size_t>(scan_bytes, 256))) || (rc = dev_alloc(c, d_bad, 64)) ||
        (rc = dev_alloc(c, off, (size_t)(cells + 1) * sizeof(int64_t)))) return rc;
    TileListArgs a{(const int32_t*)c->nz_idx.p, (const double*)c->nz_n.p, (const int64_t*)c->nz_off.p, (int32_t*)d_tile.p, (int64_t*)d_cnt.p,
                   (const int64_t*)off.p, nullptr, (int*)d_bad.p, c->T, n_tl, tile_shift, 0};
    launch_csr_tile_offsets(c, a);
    hipError_t e = hipGetLastError();
    // two-byte entries where every count is at most 7 (toys of sparse expectations), four-byte entries otherwise: the first
    // format is tried, and a count that does not fit sends the build to the second
    ok = false;
    for (int width = c->dot_entry16 ? 2 : 4; e == hipSuccess && !ok; width = 4) {
        const int group = 16 / width;
        const size_t n_entries = (size_t)(nnz + (group - 1) * cells + kDotPad);     // (every run padded to whole 16-byte groups; + the kernel's read-ahead)
        if ((rc = dev_alloc(c, entries, n_entries * width))) return rc;
        a.entries = entries.p;
        a.width = width;
        e = hipMemsetAsync(d_bad.p, 0, 64, c->stream);
        // (two-byte entries: 13 bits of offset -- tiles of 8192 bins use them all, their padding is entry 0, dropped by a select on
        //  the count; tiles of up to 4096 bins leave the bit for the offset of the extra zero slot behind the tile, as four-byte
        //  entries have it)
        if (e == hipSuccess && width == 2 && tile_bins > 4096) e = hipMemsetAsync(entries.p, 0, n_entries * 2, c->stream);
        if (e == hipSuccess && width == 2 && tile_bins <= 4096) e = hipMemsetD16Async((hipDeviceptr_t)entries.p, (unsigned short)pad_entry, n_entries, c->stream);
        if (e == hipSuccess && width == 4) e = hipMemsetD32Async((hipDeviceptr_t)entries.p, (int)pad_entry, n_entries, c->stream);
        launch_tm_counts(c, a);
        size_t tb = d_tmp.bytes;
        if (e == hipSuccess) e = prim_exclusive_scan_sum(d_tmp.p, tb, (const int64_t*)d_cnt.p, (int64_t*)off.p, (int64_t)0, (size_t)(cells + 1), c->stream);
        launch_tm_scatter(c, a);
        int bad = 0;
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) break;
        ok = bad == 0;
        width_out = width;
        if (width == 4) break;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_eval_datasets (tile-major lists): %s", hipGetErrorString(e));
    if (!ok) { dev_free(entries); dev_free(off); }
    return BI_OK;
}

// out_dev != NULL: results stay in HBM at out_dev[0 .. t1 - t0) (the call still returns after the stream has drained:
// its descriptors travel through the context's pinned staging block, which the next call reuses)
int eval_datasets_impl(bi_ctx* c, const double* z, const double* rate_scale, int64_t t0, int64_t t1, double* out,
                       double* out_dev, int32_t* status) {
    int rc = check_toy_call(c, "bi_eval_datasets", 1, z, t0, t1, out, out_dev);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t n = t1 - t0;
    if (status) *status = 0;
    const double ninf = -std::numeric_limits<double>::infinity();
    auto reject = [&](int32_t bit) -> int {          // the reference returns -inf before it looks at any data
        if (status) *status = bit;
        if (out_dev) {
            // on the context's stream, like every other write to (and the caller's collectives on) that buffer
            if (n) {
                hipLaunchKernelGGL(k_fill_value, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, out_dev, n, ninf);
                hipError_t e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_eval_datasets_device: %s", hipGetErrorString(e));
            }
        } else {
            std::fill(out, out + n, ninf);
        }
        return BI_OK;
    };
    PointGeom g;
    std::vector<double> r((size_t)c->S);
    if (const int32_t bit = screen_point(c, z, rate_scale, 0, g, r.data())) return reject(bit);
    const int NS = (int)g.w.size() * c->S;
    std::vector<int64_t> rowoff((size_t)NS);
    std::vector<double> coef((size_t)NS);
    point_streams(c, g, r.data(), rowoff.data(), coef.data());
    const int n_tiles = n_tiles_of(c);
    const int64_t slots = (int64_t)c->prop.multiProcessorCount * c->blocks_per_cu;
    const int nmu = (int)std::min<int64_t>(n_tiles, slots);
    ScratchBuf d_out;
    const bool csr = (c->sparse && c->csr_ready) || !c->dense_counts;
    if (csr && !c->csr_ready) return fail(c, BI_ERR_STATE, "no counts resident");
    // Non-empty-bin lists with enough entries per (dataset, bin tile): the tiled kernel (log mu staged through LDS, the
    // lists re-ordered tile by tile once per data upload).
    const int n_tl = (int)((c->B + kDotTile - 1) / kDotTile);
    bool tiled = csr && c->dot_tiled && n >= 64 && n_tl >= 4 && c->h_nz_off.size() == (size_t)c->T + 1 &&
                 c->h_nz_off.back() >= (int64_t)16 * c->T * n_tl && (int64_t)c->T * (n_tl + 1) <= ((int64_t)1 << 28);
    if (tiled && c->nz_tile_epoch != c->epoch) {
        if ((rc = build_tile_major(c, kDotTile, c->tm_entries, c->tm_off, c->tm_ok, c->tm_width))) return rc;
        c->nz_tile_epoch = c->epoch;
    }
    tiled = tiled && c->tm_ok;
    const int64_t chunk = tiled ? std::max<int64_t>(64, ((int64_t)1 << 27) / n_tl) : (csr ? 1048576 : 16384);
    const int nbx = tiled ? n_tl : csr ? 1 : (int)std::min<int64_t>(n_tiles, std::max<int64_t>(1, 4 * slots / std::max<int64_t>(1, (std::min(n, chunk) + kDotGroup - 1) / kDotGroup)));
    // descriptors in one packed copy; up to 4 MB of results are written straight into pinned host memory
    const bool host_out = !out_dev && (size_t)n * sizeof(double) <= ((size_t)4 << 20);
    // (up to kMaxSingleStreams streams the point's descriptors ride in the kernel arguments: no copy ahead of the launch)
    const bool by_value = NS <= kMaxSingleStreams && (c->toy_fast_call & 1);
    PackedUpload pu;
    std::vector<std::pair<const void*, size_t>> parts;
    if (!by_value) parts = {{rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)}};
    if ((rc = packed_upload(c, parts, host_out ? (size_t)n * sizeof(double) : 0, pu)) ||
        (rc = dev_alloc(c, c->logmu, (size_t)c->Bp * sizeof(double))) ||
        (rc = dev_alloc(c, c->scratch, (size_t)nmu * sizeof(double) + (size_t)nmu * sizeof(unsigned) + 64)) ||
        (rc = dev_alloc(c, c->scratch2, (size_t)std::min(n, chunk) * nbx * sizeof(double))) ||
        (!host_out && !out_dev && (rc = dev_alloc(c, d_out, (size_t)std::max<int64_t>(n, 1) * sizeof(double))))) return rc;
    double* res = out_dev ? out_dev : (host_out ? (double*)pu.host_out() : (double*)d_out.p);
    LaunchArgs a{};
    a.ps = (const double*)c->ps.p;
    a.rowoff = by_value ? nullptr : pu.dev<int64_t>(0);
    a.coef = by_value ? nullptr : pu.dev<double>(1);
    a.partial = (double*)c->scratch.p;
    a.pflags = (unsigned*)((char*)c->scratch.p + (((size_t)nmu * sizeof(double) + 63) / 64) * 64);
    a.B = c->B; a.Bp = c->Bp; a.n0 = NS; a.n_tiles = n_tiles;
    // One chunk of tiled partials whose results go to pinned host memory: the call polls the completion word
    ToyDone done;
    if (tiled && host_out && n <= chunk && c->poll_result && !c->profiling && (c->toy_fast_call & 6) == 6 &&
        (rc = done.arm(c, pu, (size_t)n * sizeof(double)))) return rc;
    {
        EventScope ev(c);
        if (by_value) {
            PointDesc pd;
            memcpy(pd.rowoff, rowoff.data(), rowoff.size() * sizeof(int64_t));
            memcpy(pd.coef, coef.data(), coef.size() * sizeof(double));
            launch_morph_logmu(c, nmu, a, &pd, (double*)c->logmu.p, 0);
        } else
            launch_morph_logmu(c, nmu, a, nullptr, (double*)c->logmu.p, 0);
    }
    for (int64_t s0 = 0; s0 < n; s0 += chunk) {
        const int64_t ni = std::min(chunk, n - s0);
        {
            EventScope ev(c);
            if (tiled) {
                // datasets split over blockIdx.y so that ~4 blocks per CU exist; every block stages its tile once
                // (and few enough datasets per block for its 32-bit entry indices: datasets x kDotTile < 2^31)
                // as many blocks as are resident at once: ONE round, every block's start-up paid once
                const int resident = dataset_dot_tiled_resident(c);
                const unsigned by = (unsigned)std::max<int64_t>({1, std::min<int64_t>((ni + 255) / 256, (int64_t)resident * c->prop.multiProcessorCount / n_tl),
                                                                 (ni + 262143) / 262144});
                launch_dataset_dot_tiled(c, by, ToyDotArgs{c->tm_entries.p, (const int64_t*)c->tm_off.p, c->T, n_tl, (const double*)c->logmu.p, c->B, c->Bp,
                                                           t0 + s0, ni, (double*)c->scratch2.p});
            } else if (csr)
                launch_dataset_dot_csr(c, ni, (const int32_t*)c->nz_idx.p, (const double*)c->nz_n.p, (const int64_t*)c->nz_off.p,
                                       (const double*)c->logmu.p, t0 + s0, (double*)c->scratch2.p);
            else
                launch_dataset_dot(c, dim3((unsigned)nbx, (unsigned)((ni + kDotGroup - 1) / kDotGroup)), (const double*)c->counts.p,
                                   (const double*)c->logmu.p, c->Bp, n_tiles, t0 + s0, ni, (double*)c->scratch2.p);
        }
        ToyFinishArgs f{};
        f.partial = (const double*)c->scratch2.p;
        f.nbx = nbx;
        f.t_stride = tiled ? (int64_t)1 : (int64_t)nbx;
        f.b_stride = tiled ? ni : (int64_t)1;
        f.mu = (const double*)a.partial; f.mu_flags = (const unsigned*)a.pflags; f.nmu = nmu;
        f.lgsum = (const double*)c->lgsum.p; f.t0 = t0 + s0; f.n = ni; f.out = res + s0;
        f.blocks_done = (unsigned*)c->toy_blocks_done.p; f.done = done.word; f.seq = done.seq;
        if (tiled && (c->toy_fast_call & 2)) launch_dataset_finish_tiled(c, f);
        else launch_dataset_finish(c, f);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && n && !host_out && !out_dev) e = hipMemcpyAsync(out, d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && done.word) done.wait(c, n);
    if (e == hipSuccess && done.must_sync()) e = hipStreamSynchronize(c->stream);
    done.close(c);
    if (e == hipSuccess && n && host_out) memcpy(out, res, (size_t)n * sizeof(double));
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_eval_datasets: %s", hipGetErrorString(e));
    return BI_OK;
}

// P points x datasets [t0, t1) -> out [P][t1 - t0] (host) or out_dev (device, same layout); status [P] or NULL
int eval_datasets_points_impl(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int64_t t0, int64_t t1, double* out,
                              double* out_dev, int32_t* status) {
    int rc = check_toy_call(c, "bi_eval_datasets_points", P, z, t0, t1, out, out_dev);
    if (rc) return rc;
    const int64_t n = t1 - t0;
    if (status) std::fill(status, status + P, 0);
    if (P == 0 || n == 0) return BI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int S = c->S, d = c->d;
    // point by point through bi_eval_datasets: what the call means, and the route of everything the multi-point kernels do not
    // cover (dense counts, few datasets, lists whose counts fit neither entry format, models with more streams than a point's
    // descriptors hold)
    auto one_by_one = [&]() -> int {
        for (int64_t p = 0; p < P; ++p) {
            int32_t st = 0;
            const int r1 = eval_datasets_impl(c, z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr, t0, t1,
                                              out ? out + p * n : nullptr, out_dev ? out_dev + p * n : nullptr, &st);
            if (r1) return r1;
            if (status) status[p] = st;
        }
        return BI_OK;
    };
    const bool csr = (c->sparse && c->csr_ready) || !c->dense_counts;
    if (csr && !c->csr_ready) return fail(c, BI_ERR_STATE, "no counts resident");
    const int n_tl = (int)((c->B + kDotTileMulti - 1) / kDotTileMulti);
    const int nc = 1 << (int)c->eff_axes.size(), NS = nc * S;
    bool multi = csr && c->dot_tiled && c->toy_points_pp != 1 && P >= 2 && n >= 64 && n_tl >= 4 && c->h_nz_off.size() == (size_t)c->T + 1 &&
                 c->h_nz_off.back() >= (int64_t)8 * c->T * n_tl && (int64_t)c->T * (n_tl + 1) <= ((int64_t)1 << 28) && n <= ((int64_t)1 << 18);
    if (multi && c->tmm_epoch != c->epoch) {
        if ((rc = build_tile_major(c, kDotTileMulti, c->tmm_entries, c->tmm_off, c->tmm_ok, c->tmm_width))) return rc;
        c->tmm_epoch = c->epoch;
    }
    if (!multi || !c->tmm_ok) return one_by_one();

    // ---- per point: geometry, rates, early exits (blueice/likelihood.py:345-347, 397-415) ----
    struct Pt { int64_t cell; int idx; };
    std::vector<Pt> valid;
    std::vector<int32_t> bad_rows;
    std::vector<PointGeom> geom((size_t)P);
    std::vector<double> rates((size_t)P * S);
    for (int64_t p = 0; p < P; ++p) {
        PointGeom& g = geom[(size_t)p];
        if (const int32_t bit = screen_point(c, z ? z + p * d : nullptr, rate_scale ? rate_scale + p * S : nullptr, 0, g,
                                             rates.data() + (size_t)p * S)) {
            if (status) status[p] = bit;
            bad_rows.push_back((int32_t)p);
            continue;
        }
        valid.push_back(Pt{g.cell_anchor, (int)p});
    }
    const int n_valid = (int)valid.size();
    std::stable_sort(valid.begin(), valid.end(), [](const Pt& a, const Pt& b) { return a.cell < b.cell; });
    const int PP = (c->toy_points_pp == 2 || (c->toy_points_pp == 0 && n_valid <= 2)) ? 2 : 4;
    const int n_pass = (n_valid + PP - 1) / PP;

    // ---- work items of the log mu kernel: the points of a GROUP of passes that share a cell ----
    // the passes are worked in groups of kPassGroup (two): the log mu rows and the per-tile partial sums of a group live in
    // scratch buffers that the next group reuses (stream order) -- 32 hypotheses x 10^4 datasets would otherwise want 0.6 GB of
    // partial sums at once, beyond what the context's recycle cache parks.  A work item covers the points of a group in one
    // cell, across its passes: eight hypotheses of one cell read the cell's anchor rows once, not once per pass.
    constexpr int kPassGroup = 2;
    const int GC = PP * kPassGroup;
    std::vector<int64_t> rowoff;
    std::vector<double> coef;
    std::vector<int32_t> meta, colmap((size_t)std::max(n_pass, 1) * PP * 2, -1);
    int n_items = 0;
    bool shared_anchor = false;           // two items read rows of the same anchor model (neighbouring cells share corners): then
    std::vector<char> anchor_used((size_t)c->A, 0);   // the default cache policy wins over the nontemporal hint
    const int n_groups = (n_pass + kPassGroup - 1) / kPassGroup;
    std::vector<int> item_begin((size_t)n_groups + 1, 0);
    for (int gr = 0; gr < n_groups; ++gr) {
        item_begin[(size_t)gr] = n_items;
        const int v0 = gr * GC, v1 = std::min(n_valid, v0 + GC);
        const int rows_of_group = std::min(kPassGroup, n_pass - gr * kPassGroup) * PP;   // rows of the table the dot kernel stages
        int v = v0;
        while (v < v1) {
            int w = v + 1;
            while (w < v1 && valid[(size_t)w].cell == valid[(size_t)v].cell) ++w;
            const PointGeom& g0 = geom[(size_t)valid[(size_t)v].idx];
            const size_t ro = rowoff.size(), co = coef.size();
            rowoff.resize(ro + NS);
            coef.resize(co + (size_t)NS * GC, 0.0);
            for (int q = v; q < w; ++q) {       // column q - v0 of the item's matrix: the point's place in the group's table
                const int p = valid[(size_t)q].idx;
                point_streams(c, geom[(size_t)p], rates.data() + (size_t)p * S, q == v ? rowoff.data() + ro : nullptr, coef.data() + co, GC, q - v0);
            }
            // the last rows of a group's last pass without a point repeat nothing: they stay zero (log 0 = -inf in the table, never
            // read back)
            const bool last_item_of_short_group = (w == v1) && (v1 - v0 < rows_of_group);
            meta.insert(meta.end(), {v - v0, last_item_of_short_group ? rows_of_group - (v - v0) : w - v, 0, 0});
            for (int q = v; q < w; ++q) {
                colmap[(size_t)q * 2 + 0] = n_items;          // [pass][column] flat = the point's place in the cell order
                colmap[(size_t)q * 2 + 1] = valid[(size_t)q].idx;
            }
            for (int corner = 0; corner < nc; ++corner) {
                char& used = anchor_used[(size_t)(g0.cell_anchor + corner_offset(c, corner))];
                if (used) shared_anchor = true;
                used = 1;
            }
            ++n_items;
            v = w;
        }
    }
    item_begin[(size_t)n_groups] = n_items;
    int max_group_items = 1;
    for (int gr = 0; gr < n_groups; ++gr) max_group_items = std::max(max_group_items, item_begin[(size_t)gr + 1] - item_begin[(size_t)gr]);
    const double ninf = -std::numeric_limits<double>::infinity();
    const bool host_out = !out_dev && (size_t)P * n * sizeof(double) <= ((size_t)4 << 20);
    ScratchBuf d_out, d_lm, d_part, d_mu;
    const int n_tiles = n_tiles_of(c);
    const int64_t slots = (int64_t)c->prop.multiProcessorCount * c->blocks_per_cu;
    const int nmu = (int)std::max<int64_t>(1, std::min<int64_t>(n_tiles, (slots + max_group_items - 1) / max_group_items));   // blocks per item of a log mu launch
    PackedUpload pu;
    std::vector<std::pair<const void*, size_t>> parts = {{rowoff.data(), rowoff.size() * sizeof(int64_t)}, {coef.data(), coef.size() * sizeof(double)},
                                                        {meta.data(), meta.size() * sizeof(int32_t)}, {colmap.data(), colmap.size() * sizeof(int32_t)},
                                                        {bad_rows.data(), bad_rows.size() * sizeof(int32_t)}};
    const size_t mu_bytes = (size_t)std::max(n_items, 1) * nmu * GC * sizeof(double);
    // Two groups in flight (toy_points_overlap = 1, more than one group, no per-kernel timing): the dot kernel is bound by LDS, the
    // log mu pass and the finish by HBM -- the next group's log mu pass and the last group's finish run on the context's second
    // (low-priority) stream BESIDE the dot kernel (a block of which leaves 32 KB of LDS and half the wave slots of its CU), each on
    // its own half of the scratch buffers.  OFF by default: measured on 32 hypotheses x 10^4 toys of C2 the kernels do run side by
    // side (rocprofv3 trace), but each slows the other by what it gains -- the dot kernel 200 -> 245-310 us beside a 105 us finish
    // and a 120 us log mu pass (60 and 52 us alone): 1.37-1.41 ms per call against 1.33-1.39 in sequence
    // (tools/probe/toy_points_overlap.py).  The same bits either way.
    const bool overlap = c->toy_points_overlap && n_groups > 1 && !c->profiling;
    const int n_buf = overlap ? 2 : 1;
    const size_t lm_group = (size_t)std::min(n_pass, kPassGroup) * c->Bp * PP;                 // doubles per group
    const size_t part_group = (size_t)std::min(n_pass, kPassGroup) * n_tl * ((n + kPartBlock - 1) / kPartBlock * kPartBlock) * PP;
    if ((rc = packed_upload(c, parts, host_out ? (size_t)P * n * sizeof(double) : 0, pu)) ||
        (n_pass > 0 && (rc = dev_alloc(c, d_lm, (size_t)n_buf * lm_group * sizeof(double)))) ||
        (n_pass > 0 && (rc = dev_alloc(c, d_part, (size_t)n_buf * part_group * sizeof(double)))) ||
        (rc = dev_alloc(c, d_mu, 2 * ((mu_bytes + 63) / 64 * 64) + (size_t)std::max(n_groups, 1) * GC * 16)) ||
        (!host_out && !out_dev && (rc = dev_alloc(c, d_out, (size_t)P * n * sizeof(double))))) return rc;
    double* res = out_dev ? out_dev : (host_out ? (double*)pu.host_out() : (double*)d_out.p);
    hipError_t e = hipSuccess;
    ToyDone done;
    if (n_valid > 0) {
        LaunchArgs a{};
        a.ps = (const double*)c->ps.p;
        a.rowoff = pu.dev<int64_t>(0);
        a.coef = pu.dev<double>(1);
        a.partial = (double*)d_mu.p;
        a.pflags = (unsigned*)((char*)d_mu.p + (mu_bytes + 63) / 64 * 64);
        // per group: sum mu and the flag of every column of its table (MuTotals: the dot kernel's first block of a pass)
        double* mu_tot = (double*)((char*)d_mu.p + 2 * ((mu_bytes + 63) / 64 * 64));
        unsigned* mu_flag = (unsigned*)(mu_tot + (size_t)std::max(n_groups, 1) * GC);
        a.B = c->B; a.Bp = c->Bp; a.n0 = NS; a.n_tiles = n_tiles; a.chunks = (int)c->tile_chunks;
        const bool nt = c->nt_loads == 1 || (c->nt_loads == 2 && !shared_anchor);
        // the dot kernel: the datasets split over blockIdx.y so that a pass fills the chip once where it can (one resident block per
        // CU: 128 KB of LDS each)
        const unsigned by = (unsigned)std::max<int64_t>({1, std::min<int64_t>((n + 255) / 256, (int64_t)c->prop.multiProcessorCount / n_tl), (n + 262143) / 262144});
        // the completion word in the pinned block (behind the results, if they go there): polled instead of a stream synchronisation,
        // whether the results land in pinned host memory or stay in HBM (out_dev)
        if ((host_out || out_dev) && c->poll_result && !c->profiling && (c->toy_fast_call & 4) &&
            (rc = done.arm(c, pu, host_out ? (size_t)P * n * sizeof(double) : 0))) return rc;
        hipStream_t sA = c->stream, sB = c->stream;
        hipEvent_t *ev_lm = c->tp_ev, *ev_dot = c->tp_ev + 2, *ev_fin = c->tp_ev + 4;
        if (overlap) {
            if (!c->stream2) {                 // the lowest priority: the dot kernel's blocks go first wherever both could
                int lo = 0, hi = 0;
                (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
                e = hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo);
            }
            for (int k = 0; k < 7 && e == hipSuccess; ++k)
                if (!c->tp_ev[k]) e = hipEventCreateWithFlags(&c->tp_ev[k], hipEventDisableTiming);
            if (e == hipSuccess) {
                sB = c->stream2;
                e = hipEventRecord(c->tp_ev[6], sA);                       // the descriptors' upload (and whatever ran before) first
                if (e == hipSuccess) e = hipStreamWaitEvent(sB, c->tp_ev[6], 0);
            }
        }
        auto launch_logmu = [&](int gr) {
            const int ib = item_begin[(size_t)gr], ie = item_begin[(size_t)gr + 1];
            LaunchArgs b = a;
            b.rowoff = a.rowoff + (int64_t)ib * NS;
            b.coef = a.coef + (int64_t)ib * NS * GC;
            b.partial = a.partial + (int64_t)ib * nmu * GC;
            b.pflags = a.pflags + (int64_t)ib * nmu * GC;
            EventScope ev(c);
            launch_morph_logmu_multi(c, sB, GC, nt, dim3((unsigned)nmu, (unsigned)(ie - ib)), b, pu.dev<int32_t>(2) + 4 * ib,
                                     (double*)d_lm.p + (size_t)(gr % n_buf) * lm_group);
        };
        if (e == hipSuccess) {
            launch_logmu(0);
            if (overlap) e = hipEventRecord(ev_lm[0], sB);
        }
        for (int gr = 0; gr < n_groups && e == hipSuccess; ++gr) {
            const int g0 = gr * kPassGroup;
            const int np = std::min(kPassGroup, n_pass - g0);
            const bool last = gr + 1 == n_groups;
            const double* lm = (const double*)d_lm.p + (size_t)(gr % n_buf) * lm_group;
            double* part = (double*)d_part.p + (size_t)(gr % n_buf) * part_group;
            if (!last) {                       // the next group's log mu rows: beside this group's dot kernel when the streams differ
                if (overlap && gr >= 1) e = hipStreamWaitEvent(sB, ev_dot[(gr + 1) % 2], 0);      // (its half of the table: read by group gr - 1)
                if (e == hipSuccess && overlap) {
                    launch_logmu(gr + 1);
                    e = hipEventRecord(ev_lm[(gr + 1) % 2], sB);
                }
            }
            if (e == hipSuccess && overlap) e = hipStreamWaitEvent(sA, ev_lm[gr % 2], 0);
            if (e == hipSuccess && overlap && gr >= 2) e = hipStreamWaitEvent(sA, ev_fin[gr % 2], 0);   // (its half of the partial sums: read by group gr - 2's finish)
            if (e != hipSuccess) break;
            const int32_t* colmap_dev = pu.dev<int32_t>(3) + (int64_t)g0 * PP * 2;
            {
                EventScope ev(c);
                e = launch_dataset_dot_multi(c, sA, PP, by, np,
                                             ToyDotArgs{c->tmm_entries.p, (const int64_t*)c->tmm_off.p, c->T, n_tl, lm, c->B, c->Bp, t0, n, part},
                                             MuTotals{colmap_dev, (const double*)a.partial, (const unsigned*)a.pflags, nmu, GC,
                                                      mu_tot + (size_t)gr * GC, mu_flag + (size_t)gr * GC});
            }
            if (e == hipSuccess && overlap) {
                e = hipEventRecord(ev_dot[gr % 2], sA);
                if (e == hipSuccess) e = hipStreamWaitEvent(sB, ev_dot[gr % 2], 0);
            }
            if (e == hipSuccess) {
                EventScope ev(c);
                // (the completion word is published by the LAST group's finish: the second stream runs the finishes in order, and a
                //  group's finish follows its dot kernel)
                ToyFinishArgs f{};
                f.partial = (const double*)part; f.nbx = n_tl; f.colmap = colmap_dev;
                f.mu = (const double*)(mu_tot + (size_t)gr * GC); f.mu_flags = (const unsigned*)(mu_flag + (size_t)gr * GC);
                f.lgsum = (const double*)c->lgsum.p; f.t0 = t0; f.n = n; f.out = res; f.out_stride = n;
                f.blocks_done = (unsigned*)c->toy_blocks_done.p; f.done = last ? done.word : nullptr; f.seq = done.seq;
                launch_dataset_finish_multi(c, sB, PP, np, f);
                if (overlap) e = hipEventRecord(ev_fin[gr % 2], sB);
            }
            if (e == hipSuccess && !overlap && !last) launch_logmu(gr + 1);
        }
        if (e == hipSuccess && overlap) {      // what follows on the context's stream follows the finishes
            e = hipStreamWaitEvent(sA, ev_fin[(n_groups - 1) % 2], 0);
            if (e == hipSuccess) e = hipStreamWaitEvent(sA, ev_fin[n_groups % 2], 0);
        }
        c->n_toy_points_passes += n_pass;
    }
    if (e == hipSuccess && !bad_rows.empty()) launch_fill_rows(c, res, n, pu.dev<int32_t>(4), (int)bad_rows.size(), n, ninf);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && !host_out && !out_dev) e = hipMemcpyAsync(out, d_out.p, (size_t)P * n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && done.word && bad_rows.empty()) done.wait(c, (int64_t)n_valid * n);
    if (e == hipSuccess && done.must_sync()) e = hipStreamSynchronize(c->stream);
    else if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); if (c->stream2) (void)hipStreamSynchronize(c->stream2); }
    done.close(c);
    if (e == hipSuccess && host_out) memcpy(out, res, (size_t)P * n * sizeof(double));
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_eval_datasets_points: %s", hipGetErrorString(e));
    return BI_OK;
}

}  // namespace
