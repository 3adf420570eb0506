// tu_toys.hip -- translation unit of the toy-MC evaluation kernels (bi_k_toys.h) and of the choice among their variants.  See
// bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_toys.h"

void launch_csr_tile_offsets(bi_ctx* c, const TileListArgs& a) {
    hipLaunchKernelGGL(k_csr_tile_offsets, dim3((unsigned)a.T), dim3(kThreads), 0, c->stream, a.nz_idx, a.nz_off, a.n_tl, a.tile_off, a.tile_shift);
}

void launch_tm_counts(bi_ctx* c, const TileListArgs& a) {
    const int64_t cells = (int64_t)a.n_tl * a.T;
    hipLaunchKernelGGL(k_tm_counts, dim3((unsigned)((cells + 1 + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)a.tile_off, a.T, a.n_tl,
                       a.cnt, 16 / a.width);
}

void launch_tm_scatter(bi_ctx* c, const TileListArgs& a) {
    if (a.width == 2)
        hipLaunchKernelGGL((k_tm_scatter<uint16_t>), dim3((unsigned)a.T), dim3(kThreads), 0, c->stream, a.nz_idx, a.nz_n, a.nz_off,
                           (const int32_t*)a.tile_off, a.T, a.n_tl, a.tm_off, (uint16_t*)a.entries, a.bad, a.tile_shift);
    else
        hipLaunchKernelGGL((k_tm_scatter<uint32_t>), dim3((unsigned)a.T), dim3(kThreads), 0, c->stream, a.nz_idx, a.nz_n, a.nz_off,
                           (const int32_t*)a.tile_off, a.T, a.n_tl, a.tm_off, (uint32_t*)a.entries, a.bad, a.tile_shift);
}

void launch_morph_logmu(bi_ctx* c, int nmu, const LaunchArgs& a, const PointDesc* pd, double* logmu, int store_mu) {
    if (pd) hipLaunchKernelGGL(k_morph_logmu_desc, dim3((unsigned)nmu), dim3(kThreads), 0, c->stream, a, *pd, logmu, store_mu);
    else hipLaunchKernelGGL(k_morph_logmu, dim3((unsigned)nmu), dim3(kThreads), 0, c->stream, a, logmu, store_mu);
}

void launch_dataset_dot(bi_ctx* c, dim3 grid, const double* counts, const double* logmu, int64_t Bp, int n_tiles, int64_t t0, int64_t n, double* partial) {
    hipLaunchKernelGGL(k_dataset_dot, grid, dim3(kThreads), 0, c->stream, counts, logmu, Bp, n_tiles, t0, n, partial);
}

void launch_dataset_dot_csr(bi_ctx* c, int64_t n, const int32_t* nz_idx, const double* nz_n, const int64_t* nz_off, const double* logmu, int64_t t0, double* partial) {
    hipLaunchKernelGGL(k_dataset_dot_csr, dim3((unsigned)n), dim3(kThreads), 0, c->stream, nz_idx, nz_n, nz_off, logmu, t0, partial);
}

namespace {

// variant: 4-byte entries <8, 3> (96 slots per run) or <16, 2>; 2-byte entries <8, 2, 2> (128 slots) or, dot_lanes 4, <4, 3, 2> (96 slots)
// (dot_lanes 0 = the best measured for the entry width: 8 lanes with four-byte entries, 4 with two-byte ones)
int dot_tiled_variant(const bi_ctx* c) {
    return c->tm_width == 2 ? ((c->dot_lanes == 4 || c->dot_lanes == 0) ? 3 : 2) : (c->dot_lanes == 16 ? 1 : 0);
}

}  // namespace

// as many blocks as are resident at once (the 8-lane variant's registers allow one per CU, the 16-lane variant's two; asked from the
// runtime once)
int dataset_dot_tiled_resident(bi_ctx* c) {
    const int variant = dot_tiled_variant(c);
    static std::atomic<int> resident_cache[4];
    std::atomic<int>& rslot = resident_cache[variant];
    int resident = c->dot_blocks_per_cu > 0 ? (int)c->dot_blocks_per_cu : rslot.load();
    if (resident <= 0) {
        int r = 0;
        const void* f = variant == 0 ? (const void*)k_dataset_dot_tiled<8, 3, 4> : variant == 1 ? (const void*)k_dataset_dot_tiled<16, 2, 4>
                      : variant == 2 ? (const void*)k_dataset_dot_tiled<8, 2, 2> : (const void*)k_dataset_dot_tiled<4, 3, 2>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, f, kDotThreads, 0) != hipSuccess || r < 1) r = 1;
        rslot.store(r);
        resident = r;
    }
    return resident;
}

void launch_dataset_dot_tiled(bi_ctx* c, unsigned by, const ToyDotArgs& a) {
#define BI_DOT(L, AHEAD, W)                                                                                        \
    hipLaunchKernelGGL((k_dataset_dot_tiled<L, AHEAD, W>), dim3((unsigned)a.n_tl, by), dim3(kDotThreads), 0, c->stream, \
                       a.entries, a.off, a.T, a.n_tl, a.lm, a.B, a.t0, a.n, a.partial)
    const int variant = dot_tiled_variant(c);
    if (variant == 0) BI_DOT(8, 3, 4); else if (variant == 1) BI_DOT(16, 2, 4); else if (variant == 2) BI_DOT(8, 2, 2); else BI_DOT(4, 3, 2);
#undef BI_DOT
}

void launch_dataset_finish(bi_ctx* c, const ToyFinishArgs& a) {
    hipLaunchKernelGGL(k_dataset_finish, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, c->stream, a.partial, a.nbx, a.t_stride, a.b_stride,
                       a.mu, a.mu_flags, a.nmu, a.lgsum, a.t0, a.n, a.out);
}

void launch_dataset_finish_tiled(bi_ctx* c, const ToyFinishArgs& a) {
    hipLaunchKernelGGL(k_dataset_finish_tiled, dim3((unsigned)((a.n + 63) / 64)), dim3(kThreads), 0, c->stream, a.partial, a.nbx, a.mu, a.mu_flags,
                       a.nmu, a.lgsum, a.t0, a.n, a.out, a.blocks_done, a.done, a.seq);
}

void launch_morph_logmu_multi(bi_ctx* c, hipStream_t s, int GC, bool nt, dim3 grid, const LaunchArgs& a, const int32_t* meta, double* lm) {
#define BI_LM(GCv) /* GCv: rows of a group's table */                                                              \
    do {                                                                                                           \
        if (nt) hipLaunchKernelGGL((k_morph_logmu_multi<GCv, true>), grid, dim3(kThreads), 0, s, a, meta, lm);     \
        else hipLaunchKernelGGL((k_morph_logmu_multi<GCv, false>), grid, dim3(kThreads), 0, s, a, meta, lm);       \
    } while (0)
    if (GC == 4) BI_LM(4); else BI_LM(8);
#undef BI_LM
}

hipError_t launch_dataset_dot_multi(bi_ctx* c, hipStream_t s, int PP, unsigned by, int np, const ToyDotArgs& a, const MuTotals& mt) {
    const size_t lds = (size_t)(kDotTileMulti + 1) * 16 * (PP / 2);            // planes of 16-byte cells (+ the zero cell)
    const int variant = (c->tmm_width == 2 ? 0 : 2) + (PP == 4 ? 0 : 1);     // {W2 PP4, W2 PP2, W4 PP4, W4 PP2}
    const int lanes = (int)c->toy_points_lanes;
    const dim3 grid((unsigned)a.n_tl, by, (unsigned)np);
    hipError_t e = hipSuccess;
    // L x AHEAD x (16 / W) entry slots per run; a run holds ~38 entries at configs[2] (tiles of 4096 bins)
#define BI_DM(Lv, Av, Wv, PPv)                                                                                             \
    do {                                                                                                                   \
        e = hipFuncSetAttribute((const void*)k_dataset_dot_multi<Lv, Av, Wv, PPv, kDotTileMulti>,                          \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                     \
        if (e == hipSuccess)                                                                                               \
            hipLaunchKernelGGL((k_dataset_dot_multi<Lv, Av, Wv, PPv, kDotTileMulti>), grid, dim3(kDotThreads), lds, s,     \
                               a.entries, a.off, a.T, a.n_tl, a.lm, a.B, a.Bp, a.t0, a.n, a.partial, mt);                  \
    } while (0)
    if (variant == 0) { if (lanes == 2) BI_DM(2, 3, 2, 4); else if (lanes == 8) BI_DM(8, 1, 2, 4); else BI_DM(4, 2, 2, 4); }
    else if (variant == 1) { if (lanes == 2) BI_DM(2, 3, 2, 2); else if (lanes == 8) BI_DM(8, 1, 2, 2); else BI_DM(4, 2, 2, 2); }
    else if (variant == 2) { if (lanes == 4) BI_DM(4, 3, 4, 4); else BI_DM(8, 2, 4, 4); }
    else { if (lanes == 4) BI_DM(4, 3, 4, 2); else BI_DM(8, 2, 4, 2); }
#undef BI_DM
    return e;
}

void launch_dataset_finish_multi(bi_ctx* c, hipStream_t s, int PP, int np, const ToyFinishArgs& a) {
    const dim3 grid((unsigned)((a.n + kPartBlock - 1) / kPartBlock), (unsigned)np);
#define BI_FM(PPv)                                                                                                          \
    hipLaunchKernelGGL((k_dataset_finish_multi<PPv>), grid, dim3(kThreads), 0, s, a.partial, a.nbx, a.colmap, a.mu, a.mu_flags, a.lgsum, \
                       a.t0, a.n, a.out, a.out_stride, a.blocks_done, a.done, a.seq)
    if (PP == 2) BI_FM(2); else BI_FM(4);
#undef BI_FM
}

void launch_fill_rows(bi_ctx* c, double* out, int64_t out_stride, const int32_t* rows, int n_rows, int64_t n, double v) {
    hipLaunchKernelGGL(k_fill_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, out, out_stride, rows, n_rows, n, v);
}
