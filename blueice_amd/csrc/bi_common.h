// bi_common.h -- what every translation unit of libblueice_hip includes: the runtime, the context / plan objects, the
// device helpers, and the launchers through which the main translation unit (blueice_hip.hip: the C ABI, planning, the
// small kernels) reaches the heavy template families, each of which is compiled in its own translation unit so that a
// clean build runs on several cores (blueice_amd/build.py):
//     tu_morph.hip        k_morph_reduce (values, gradients, unbinned), k_morph_single        bi_k_morph.h
//                         k_morph_sets (unbinned work items with an event set each)          bi_k_sets.h
//     tu_scan.hip         k_scan_mfma, k_scan_valid                                          bi_k_scan.h
//     tu_scan_sorted.hip  k_scan_sorted                                                      bi_scan_sorted.h
//     tu_grad.hip         k_grad_mfma, k_morph_bbgrad                                        bi_k_grad_mfma.h, bi_k_bbgrad.h
//     tu_scan_bb.hip      k_scan_bb (Beeston-Barlow scans on the matrix cores)               bi_k_scan_bb.h
//     tu_hess.hip         k_morph_hess (value + gradient + Hessian of one point per item)    bi_k_hess.h
//     tu_gof.hip          k_morph_gof (deviance + Pearson chi2 of one point per item), k_morph_expect   bi_k_gof.h
//     tu_real.hip         k_morph_real (half-deviance + gradient against real-valued counts), k_real_expect   bi_k_real.h
//     tu_factored.hip     k_morph_factored (value + gradient sums of one point of a source-wise model per item)   bi_k_factored.h
//     tu_factored_curv.hip, tu_factored_fisher.hip   k_factored_curv, observed and Fisher form (Hessian and expected-information sums of
//                         one point of a source-wise model per item)                         bi_k_factored_curv.h
//     tu_sourcewise_expect.hip, tu_sourcewise_gof.hip   k_sourcewise_expect (the per-bin expectation of a source-wise model, written
//                         out), k_sourcewise_gof (its deviance + Pearson chi2 per item)      bi_k_sourcewise.h
//     tu_sourcewise_real.hip   k_sourcewise_real (half-deviance + gradient sums of one point of a source-wise model against
//                         real-valued counts per item)                                       bi_k_sourcewise_real.h
//     tu_sourcewise_plan.hip   k_sourcewise_plan (staged points of a source-wise model -> status words and k_morph_factored's
//                         descriptors, on the device)                                        bi_k_sourcewise_plan.h
//     tu_sourcewise_nonempty.hip   k_sourcewise_nonempty (value + gradient sums of one point of a source-wise model over the
//                         non-empty bins of its dataset), k_sourcewise_gather (the compacted copies)   bi_k_sourcewise_nonempty.h
//     tu_sourcewise_events.hip   k_sourcewise_events (value + gradient sums of one point of a source-wise model over the events of
//                         its event set: the unbinned likelihood)                           bi_k_sourcewise_events.h
//     tu_sourcewise_events_curv.hip   k_sourcewise_events_curv (the Hessian's sums of one point of a source-wise model over the events
//                         of its event set, in k_factored_curv's Gram panels)                bi_k_sourcewise_events_curv.h
//     tu_sourcewise_sim.hip   k_sourcewise_pmf, k_sourcewise_sim_counts, _room, _first, _events (event-level toys of a source-wise
//                         model: per-source pmf rows, counts, layout and the events themselves)   bi_k_sourcewise_sim.h
//     tu_sourcewise_scan.hip   k_sourcewise_scan_key, _cut, _groups, _fill (the planner's per-point descriptors -> the 16-point work
//                         items of k_scan_mfma, on the device)                               bi_k_sourcewise_scan.h
//     tu_sampler.hip      k_stretch_propose, k_stretch_accept (ensemble sampler half-steps)      bi_k_sampler.h
//     tu_grid.hip         k_grid_points, k_grid_reduce, k_grid_finish (gridded likelihoods)      bi_k_grid.h
//     tu_coarse.hip       k_morph_coarse, k_morph_coarse_jac, k_coarse_finish, k_coarse_list (coarse views: projections, rebinning, their derivatives)   bi_k_coarse.h
//     tu_sourcewise_coarse.hip   k_sourcewise_coarse (coarse views of a source-wise model; finished by tu_coarse.hip's kernels)   bi_k_sourcewise_coarse.h
//     tu_sourcewise_coarse_jac.hip   k_sourcewise_coarse_jac (the per-cell sums behind the derivatives of those views)   bi_k_sourcewise_coarse_jac.h
//     tu_fisher.hip       k_morph_fisher (expected information of one point per item, no data)   bi_k_fisher.h
//     tu_toys.hip         the toy-MC evaluation kernels (k_morph_logmu*, k_dataset_dot*, k_dataset_finish*, k_tm_*)   bi_k_toys.h
//     tu_prim.hip         the hand-written sorts and scans (behind plain functions)                  bi_prim.h
// bi_k_item.h is the device skeleton the per-point item kernels share (tile walk, column sums, block reduction, expectation
// chain): included by bi_k_hess.h, bi_k_fisher.h, bi_k_real.h, bi_k_gof.h, bi_k_bbgrad.h, bi_k_sets.h, bi_k_coarse.h,
// bi_k_factored.h and (through it) bi_k_factored_curv.h and bi_k_sourcewise_real.h, and bi_k_sourcewise.h (which shares gof_terms, bi_k_gof_terms.h, with bi_k_gof.h; bi_k_sourcewise_coarse.h and
// bi_k_sourcewise_coarse_jac.h include it).
// gfx950 only; no kernel is defined in two translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/blueice_hip.h"

#define BI_VERSION "blueice_hip 0.1 (gfx950)"

#include "bi_wait.h"
#include "bi_context.h"
#include "bi_log_table.h"
#include "bi_dev_common.h"

namespace {

struct EventScope {
    bi_ctx* c;
    size_t idx = (size_t)-1;
    explicit EventScope(bi_ctx* ctx) : c(ctx) {       // (kernels on the context's second stream are only launched when profiling is off)
        if (!c->profiling) return;
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            c->ev_pool.emplace_back(a, b);
        }
        idx = c->ev_used++;
        (void)hipEventRecord(c->ev_pool[idx].first, c->stream);
    }
    ~EventScope() {
        if (idx != (size_t)-1) (void)hipEventRecord(c->ev_pool[idx].second, c->stream);
    }
};

}  // namespace

// ---- launchers of the kernel families (defined in tu_*.hip) ----------------------------------------------------------
// k_morph_reduce<G, BB, NT, MODE>: G points per cell pass (1, 2, 4, 8, 16); MODE 0 binned / 2 unbinned by the context
void launch_morph_g(bi_ctx* c, int G, const LaunchArgs& a, dim3 grid, bool bb, bool nt);
// ... MODE 1 / 3: value + gradient columns of one point (G = 2, 4, 8, 16 columns)
void launch_morph_grad(bi_ctx* c, int G, const LaunchArgs& a, dim3 grid, bool nt);
// k_morph_sets<G, MODE>: unbinned work items that each have their own event set (item_cnt = the set's events); G = 1 values
void launch_morph_sets(bi_ctx* c, int G, const LaunchArgs& a, dim3 grid);
// k_morph_single<BB, NT, MODE, FUSE>: the single-point call
void launch_morph_single(bi_ctx* c, bool bb, bool nt, bool fuse, dim3 grid, const LaunchArgs& a, const SingleDesc& d);
// k_morph_bbgrad<G, DZ, NT>: value + gradient with Beeston-Barlow; BI_ERR_INVALID for a column count without a variant
int launch_morph_bbgrad(bi_ctx* c, int G, int DZ, const LaunchArgs& a, dim3 grid, bool nt);
// k_morph_hess<G, DM, UNB, NT>: value, gradient and Hessian of one point per item; BI_ERR_INVALID for a (G, DM) without a variant
int launch_morph_hess(bi_ctx* c, int G, int DM, const HessArgs& a, dim3 grid, bool nt);
// k_morph_fisher<G, DM, NT>: the expected information of one point per item (HessArgs, no counts read); G = 4, 8, 16 coefficient
// columns, DM first-order columns; BI_ERR_INVALID for a (G, DM) without a variant
int launch_morph_fisher(bi_ctx* c, int G, int DM, const HessArgs& a, dim3 grid, bool nt);
// k_morph_gof<NT>: half-deviance and Pearson chi2 of one (point, dataset) per item, HessArgs with ONE coefficient column
void launch_morph_gof(bi_ctx* c, const HessArgs& a, dim3 grid, bool nt);
// k_morph_expect: the per-bin expectation of n_items (<= 65 535) points, a.R groups of rows each
void launch_morph_expect(bi_ctx* c, const ExpectArgs& a, int64_t n_items);
// k_morph_real<G, NT>: half-deviance and its first derivatives of one (point, real-valued dataset) per item, G = 1 (value
// only), 4, 8 or 16 coefficient columns; BI_ERR_INVALID for another G
int launch_morph_real(bi_ctx* c, int G, const HessArgs& a, dim3 grid, bool nt);
// k_real_expect: the expectation of n_items (<= 65 535) truths into rows of the real-valued store
void launch_real_expect(bi_ctx* c, const RealExpectArgs& a, int64_t n_items);
// k_morph_factored<SC, EM, GRAD, NT>: value (and the gradient's partial sums) of one point of a source-wise model per item;
// SC = 2, 4, 8 source slots, EM = 1, 2, 3 own axes at most; BI_ERR_INVALID for another (SC, EM).  factored_slots: its result
// slots per item
int launch_morph_factored(bi_ctx* c, int SC, int EM, bool grad, const FactoredArgs& a, dim3 grid, bool nt);
inline int factored_slots(int SC, int EM, bool grad) { return grad ? 1 + SC * (1 + EM) : 1; }
// k_factored_curv<SC, EM, FISHER, PS, PANEL>: the Hessian's (fisher = false) or the expected information's sums of one point of a
// source-wise model per item, Gram panel `panel` of factored_curv_panels(SC, EM); BI_ERR_INVALID for another (SC, EM, panel).
// factored_curv_linear: the linear slots in front of panel 0's pairs; factored_curv_panel_rows: the Gram rows [lo, hi) of a panel
int launch_factored_curv_observed(bi_ctx* c, int SC, int EM, int panel, const FactoredArgs& a, dim3 grid);
int launch_factored_curv_fisher(bi_ctx* c, int SC, int EM, int panel, const FactoredArgs& a, dim3 grid);
inline int launch_factored_curv(bi_ctx* c, int SC, int EM, bool fisher, int panel, const FactoredArgs& a, dim3 grid) {
    return fisher ? launch_factored_curv_fisher(c, SC, EM, panel, a, grid) : launch_factored_curv_observed(c, SC, EM, panel, a, grid);
}
constexpr int factored_curv_linear(int SC, int EM, bool fisher) { return 1 + SC * (1 + EM) + (fisher ? 0 : SC * (EM * (EM - 1) / 2)); }
constexpr int factored_curv_panel_sources(int SC, int EM) { return SC * (1 + EM) <= 16 ? SC : EM == 2 ? 2 : 1; }
constexpr int factored_curv_panels(int SC, int EM) { return SC / factored_curv_panel_sources(SC, EM); }
// k_sourcewise_expect<SC, EM, PS, NT>: the per-bin expectation of n_items (<= 65 535) points of a source-wise model into a.out,
// one row per point or (per_source) one per source; k_sourcewise_gof<SC, EM, NT>: half-deviance and Pearson chi2 of one point
// per item (two result slots).  BI_ERR_INVALID for an (SC, EM) without a variant, as launch_morph_factored
int launch_sourcewise_expect(bi_ctx* c, int SC, int EM, bool per_source, const SourcewiseExpectArgs& a, int64_t n_items, bool nt);
int launch_sourcewise_gof(bi_ctx* c, int SC, int EM, const FactoredArgs& a, dim3 grid, bool nt);
// k_sourcewise_real<SC, EM, GRAD, NT>: the half-deviance (and the gradient's partial sums) of one point of a source-wise model
// against the real-valued dataset a.counts + a.item_cnt[item] per item; classes and result slots (factored_slots) as
// launch_morph_factored
int launch_sourcewise_real(bi_ctx* c, int SC, int EM, bool grad, const FactoredArgs& a, dim3 grid, bool nt);
// k_sourcewise_plan<SC>: the status words and k_morph_factored's value-order descriptors of a.n staged points of a source-wise model,
// one thread per (point, source slot); BI_ERR_INVALID for another SC than 2, 4, 8
int launch_sourcewise_plan(bi_ctx* c, int SC, const SourcewisePlanArgs& a);
// ... k_sourcewise_plan<SC, NE = true>: the same for k_sourcewise_nonempty (rows, counts and tiles of the dataset's compacted copy,
// slot_lg = sum_s lambda_s + lgsum; a.g.rowsum and a.g.ne_* set)
int launch_sourcewise_plan_nonempty(bi_ctx* c, int SC, const SourcewisePlanArgs& a);
// ... k_sourcewise_plan<SC, false, EV = true>: the same for k_sourcewise_events (rows at the event set's columns, the set's number
// of events and tiles, slot_lg = sum_s r_s; a.ev_first, a.ev_n, a.ev_cols set, a.g.T the number of sets; a rejected point: tiles 0)
int launch_sourcewise_plan_events(bi_ctx* c, int SC, const SourcewisePlanArgs& a);
// k_sourcewise_nonempty<SC, EM, GRAD>: the sums of one point of a source-wise model over the non-empty bins of its dataset per item;
// classes and result slots (factored_slots) as launch_morph_factored.  grid.x: the largest block count of the launch's items
int launch_sourcewise_nonempty(bi_ctx* c, int SC, int EM, bool grad, const SourcewiseNonemptyArgs& a, dim3 grid);
// k_sourcewise_gather: the compacted copies of grid.z datasets from a.t0 on
void launch_sourcewise_gather(bi_ctx* c, const SourcewiseGatherArgs& a, dim3 grid);
// k_sourcewise_events<SC, EM, GRAD>: the sums of one point of a source-wise model over the events of its event set per item; classes
// and result slots (factored_slots) as launch_morph_factored.  grid.x: the largest block count of the launch's items
int launch_sourcewise_events(bi_ctx* c, int SC, int EM, bool grad, const SourcewiseEventsArgs& a, dim3 grid);
// k_sourcewise_events_curv<SC, EM, PS, PANEL>: the Hessian's sums of one point of a source-wise model over the events of its event
// set per item, Gram panel `panel` of factored_curv_panels(SC, EM); a.coef holds launch_factored_curv's observed-form columns.
// BI_ERR_INVALID for another (SC, EM, panel).  grid.x: the largest block count of the launch's items
int launch_sourcewise_events_curv(bi_ctx* c, int SC, int EM, int panel, const SourcewiseEventsArgs& a, dim3 grid);
// event toys of a source-wise model (bi_k_sourcewise_sim.h; no launcher times its kernel, the host half bi_sourcewise_sim.h opens
// the EventScopes).  k_sourcewise_pmf<SC, EM>: the pmf rows of n_items (<= 65 535) truths, BI_ERR_INVALID for an (SC, EM) without
// a variant; then the counts and rooms of all (toy, source), the per-(toy, source) starts, and the events of a range of columns
int launch_sourcewise_pmf(bi_ctx* c, int SC, int EM, const SourcewisePmfArgs& a, int64_t n_items);
void launch_sourcewise_sim_counts(bi_ctx* c, const SourcewiseSimArgs& a);
void launch_sourcewise_sim_room(bi_ctx* c, const SourcewiseSimArgs& a);
void launch_sourcewise_sim_first(bi_ctx* c, const SourcewiseSimArgs& a);
void launch_sourcewise_sim_events(bi_ctx* c, const SourcewiseSimArgs& a);
// the scan planner of source-wise points (bi_k_sourcewise_scan.h; no launcher times its kernel, the host half bi_sourcewise_scan.h
// opens the EventScope): sort keys of a.n points; groups of equal keys cut every `cut` points; group tables and counts; the
// descriptors of the a.n_valid sorted positions in front of the rejected points
void launch_sourcewise_scan_key(bi_ctx* c, const SourcewiseScanArgs& a);
void launch_sourcewise_scan_cut(bi_ctx* c, int64_t* gstart, int64_t n, int64_t cut);
void launch_sourcewise_scan_groups(bi_ctx* c, const SourcewiseScanArgs& a);
void launch_sourcewise_scan_fill(bi_ctx* c, const SourcewiseScanArgs& a);
// k_scan_mfma<CB, KG, MASK, PROD>: rows in bin order; prod = the compacted rows' product form (CB = 2 only)
void launch_scan_mfma(bi_ctx* c, int cb, bool prod, int NS, dim3 grid, const ScanArgs& a);
// k_scan_valid<4, KG, MASK>: the validity pass of split scans
void launch_scan_valid(bi_ctx* c, int NS, dim3 grid, const ValidArgs& a);
// k_scan_sorted<KG, MASK>: rows ordered by count, KG = ceil(NS / 4) in 1 .. 8
void launch_scan_sorted(bi_ctx* c, int NS, dim3 grid, const ScanArgs& a);
// blocks of a scan kernel variant one CU holds at a time (hipOccupancyMaxActiveBlocksPerMultiprocessor; 0 = unknown):
// (valid, CB, 4-stream groups 1 << kg, masked) / k_scan_sorted with KG groups
int occupancy_scan(bool valid, int cb, int kg, bool mask);
int occupancy_scan_sorted(int KG, bool mask);
// k_grad_mfma<KG, MASK>
void launch_grad_mfma(bi_ctx* c, int NS, dim3 grid, const GradMfmaArgs& a);
// k_scan_bb<KGT>: Beeston-Barlow scans on the matrix cores; scan_bb_variant: the KGT for (streams into U, corners), 0 = none fits
int scan_bb_variant(int n0, int nc);
void launch_scan_bb(bi_ctx* c, int kgt, dim3 grid, const BbScanArgs& a);
int occupancy_scan_bb(int kgt);
// k_stretch_propose / k_stretch_accept: one half-step of bi_sample_stretch (h = -1: stage the start positions)
void launch_stretch_propose(bi_ctx* c, const StretchArgs& a);
void launch_stretch_accept(bi_ctx* c, const StretchArgs& a);
// k_stretch_start_density: the start walkers' log likelihoods (ll_prop) -> their log densities ll + p (ll)
void launch_stretch_start_density(bi_ctx* c, const StretchArgs& a);
// k_grid_points: the points [g0, g0 + n) of a tensor-product grid into the resident planner's layouts, with their additive terms
void launch_grid_points(bi_ctx* c, const GridArgs& a);
// k_grid_reduce: the chunk's results folded into the per-cell state; k_grid_init / k_grid_finish: the state's start and the outputs
void launch_grid_reduce(bi_ctx* c, const GridArgs& a);
void launch_grid_init(bi_ctx* c, const GridArgs& a);
void launch_grid_finish(bi_ctx* c, const GridArgs& a);
// k_morph_coarse + k_coarse_finish: the expectation (or a row of counts) of n_items (<= 65 535) items summed over the groups of a coarse binning
void launch_morph_coarse(bi_ctx* c, const CoarseArgs& a, int64_t n_items);
// k_morph_coarse_jac<G> + k_coarse_finish: the same with G = 4, 8 or 16 coefficient columns per corner row (a.R = G; a.coef [items][NS][G]);
// BI_ERR_INVALID for another G
int launch_morph_coarse_jac(bi_ctx* c, int G, const CoarseArgs& a, int64_t n_items);
// k_coarse_finish or (a.wide) k_coarse_finish_wide over a.partial: what the two launchers above end with, and launch_sourcewise_coarse
void launch_coarse_finish(bi_ctx* c, const CoarseArgs& a);
// k_sourcewise_coarse<SC, EM, PS> + k_coarse_finish: the expectation of n_items (<= 65 535) points of a source-wise model summed over
// the groups of a coarse binning, a.g.R = 1 (the total) or S (per source: PS); BI_ERR_INVALID for an (SC, EM) without a variant
int launch_sourcewise_coarse(bi_ctx* c, int SC, int EM, bool per_source, const SourcewiseCoarseArgs& a, int64_t n_items);
// k_sourcewise_coarse_jac<SC, EM> + k_coarse_finish: the sums of mu_b and of the basis columns tau_s,b, ups_s,j,b of n_items (<= 65 535)
// points of a source-wise model over the groups of a coarse binning; a.g.R = K live columns, slot -> group by a.group;
// BI_ERR_INVALID for an (SC, EM) without a variant
int launch_sourcewise_coarse_jac(bi_ctx* c, int SC, int EM, const SourcewiseCoarseJacArgs& a, int64_t n_items);
// k_coarse_list + k_coarse_table: the non-empty-bin lists of n (<= 65 535) datasets into the cells, out [n][C] (device memory)
void launch_coarse_list(bi_ctx* c, const CoarseListArgs& a, int64_t n, double* out);
// ---- the toy-MC evaluation kernels (bi_k_toys.h).  No launcher times its kernel: the host half (bi_toys.h) opens the EventScopes.
// k_csr_tile_offsets, k_tm_counts (16 / a.width entries per group), k_tm_scatter<a.width bytes per entry>
void launch_csr_tile_offsets(bi_ctx* c, const TileListArgs& a);
void launch_tm_counts(bi_ctx* c, const TileListArgs& a);
void launch_tm_scatter(bi_ctx* c, const TileListArgs& a);
// k_morph_logmu on nmu blocks (store_mu = 1: the expectation itself, for the toy generator), or with pd != NULL k_morph_logmu_desc
void launch_morph_logmu(bi_ctx* c, int nmu, const LaunchArgs& a, const PointDesc* pd, double* logmu, int store_mu);
// the row kernels: k_dataset_dot (dense counts, grid = blocks per group x groups of kDotGroup datasets), k_dataset_dot_csr (n blocks)
void launch_dataset_dot(bi_ctx* c, dim3 grid, const double* counts, const double* logmu, int64_t Bp, int n_tiles, int64_t t0, int64_t n, double* partial);
void launch_dataset_dot_csr(bi_ctx* c, int64_t n, const int32_t* nz_idx, const double* nz_n, const int64_t* nz_off, const double* logmu, int64_t t0, double* partial);
// k_dataset_dot_tiled<L, AHEAD, W>: the variant follows the context's tm_width and dot_lanes; grid (a.n_tl, by).  ..._resident: blocks
// of that variant one CU holds at a time (dot_blocks_per_cu if set, else asked from the runtime once)
int dataset_dot_tiled_resident(bi_ctx* c);
void launch_dataset_dot_tiled(bi_ctx* c, unsigned by, const ToyDotArgs& a);
// k_dataset_finish (blocks of 256 datasets) / k_dataset_finish_tiled (blocks of 64 datasets, publishes a.done when set)
void launch_dataset_finish(bi_ctx* c, const ToyFinishArgs& a);
void launch_dataset_finish_tiled(bi_ctx* c, const ToyFinishArgs& a);
// the multi-point form, on stream s (the context's or its second one): k_morph_logmu_multi<GC, NT> (GC = 4 or 8 rows per group),
// k_dataset_dot_multi<L, AHEAD, W, PP, kDotTileMulti> (variant by tmm_width, PP and toy_points_lanes; grid (a.n_tl, by, np passes);
// the error of the LDS attribute, if any) and k_dataset_finish_multi<PP> (blocks of kPartBlock datasets x np passes)
void launch_morph_logmu_multi(bi_ctx* c, hipStream_t s, int GC, bool nt, dim3 grid, const LaunchArgs& a, const int32_t* meta, double* lm);
hipError_t launch_dataset_dot_multi(bi_ctx* c, hipStream_t s, int PP, unsigned by, int np, const ToyDotArgs& a, const MuTotals& mt);
void launch_dataset_finish_multi(bi_ctx* c, hipStream_t s, int PP, int np, const ToyFinishArgs& a);
// k_fill_rows: out[rows[r]][0 .. n) = v
void launch_fill_rows(bi_ctx* c, double* out, int64_t out_stride, const int32_t* rows, int n_rows, int64_t n, double v);
