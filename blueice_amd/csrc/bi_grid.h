// bi_grid.h -- the host loop of the gridded likelihood (bi_grid_reduce): the context's likelihood on a tensor-product grid of
// F variables, reduced over the last F - n_keep of them on the device.  The grid is never held anywhere: k_grid_points writes
// one chunk of it into the layouts the resident planner reads, the planner and the evaluation kernels of
// bi_plan_points_resident / bi_run_plan take the points where they lie, k_grid_reduce folds the chunk's result vector and
// status words into the per-cell state in HBM, and the three output arrays are copied to the host once, at the end.  The
// variables' map, the chunk's rows and their evaluation are ResidentPoints' (bi_varmap.h), shared with bi_sampler.h, whose
// header says what a chunk costs on the host: the planner's counts, the status OR, making and destroying the plan.
// (The reference's counterpart is the Python double loop of blueice/inference.py:424-432, one scalar call per grid point.)
// bi_grid_reduce_sourcewise is the same loop over a source-wise model (bi_factored.h): grid_reduce takes the evaluation step as a
// parameter -- the resident planner for the grid model, PlannedItems::queue (route 0, bi_sourcewise_plan.h) or ScanItems::queue
// (route 1, the matrix-core scan route of bi_sourcewise_scan.h) for the source-wise one, which keep their buffers across the
// chunks and leave the planner's status words where the reduction reads them.
#pragma once

#include <functional>

namespace {

constexpr int64_t kGridDefaultChunk = (int64_t)1 << 20, kGridMaxChunk = (int64_t)1 << 26, kGridMaxCells = (int64_t)1 << 24,
                  kGridMaxPoints = (int64_t)1 << 48;
constexpr int64_t kGridWaveCell = 256;      // cells of up to this many points are reduced by one wave each, larger ones by a block

struct GridState {
    ScratchBuf m, s, best, arg, n_excl, nan_flag, out_lm, out_prof, out_arg;
};

int grid_state_begin(bi_ctx* c, GridState& st, GridArgs& a, int64_t cells) {
    const size_t n = (size_t)cells;
    int rc;
    if ((rc = dev_alloc(c, st.m, n * 8)) || (rc = dev_alloc(c, st.s, n * 8)) || (rc = dev_alloc(c, st.best, n * 8)) ||
        (rc = dev_alloc(c, st.arg, n * 8)) || (rc = dev_alloc(c, st.n_excl, n * 8)) || (rc = dev_alloc(c, st.nan_flag, n * 4)) ||
        (rc = dev_alloc(c, st.out_lm, n * 8)) || (rc = dev_alloc(c, st.out_prof, n * 8)) || (rc = dev_alloc(c, st.out_arg, n * 8)))
        return rc;
    a.cells = cells;
    a.m = (double*)st.m.p; a.s = (double*)st.s.p; a.best = (double*)st.best.p;
    a.arg = (int64_t*)st.arg.p; a.n_excl = (int64_t*)st.n_excl.p; a.nan_flag = (int32_t*)st.nan_flag.p;
    a.out_lm = (double*)st.out_lm.p; a.out_prof = (double*)st.out_prof.p; a.out_arg = (int64_t*)st.out_arg.p;
    launch_grid_init(c, a);
    HIP_TRY(c, hipGetLastError());
    return BI_OK;
}

// the cells that the chunk [g0, g0 + n) touches, and how they are dealt to the blocks
void grid_chunk_cells(GridArgs& a) {
    a.cell0 = a.g0 / a.R;
    a.n_cells = (a.g0 + a.n - 1) / a.R - a.cell0 + 1;
    a.cpb = a.R <= kGridWaveCell ? 4 : 1;
}

// the outputs from the state, one copy each; excluded: the sum of the cells' counts (or NULL)
int grid_state_end(bi_ctx* c, GridArgs& a, double* log_marginal, double* profile, int64_t* argmax, int64_t* excluded) {
    const size_t n = (size_t)a.cells;
    launch_grid_finish(c, a);
    HIP_TRY(c, hipGetLastError());
    std::vector<int64_t> h_excl(excluded ? n : 0);
    HIP_TRY(c, hipMemcpyAsync(log_marginal, a.out_lm, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(profile, a.out_prof, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(argmax, a.out_arg, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (excluded) HIP_TRY(c, hipMemcpyAsync(h_excl.data(), a.n_excl, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (excluded) *excluded = std::accumulate(h_excl.begin(), h_excl.end(), (int64_t)0);
    return BI_OK;
}

// The loop of bi_grid_reduce and bi_grid_reduce_sourcewise: chunks of the grid written by k_grid_points, evaluated by `step`, folded
// by k_grid_reduce.  step(pts, n, counters, reduce) evaluates the first n staged points into pts.llp, calls reduce(status words)
// once -- that launches the reduction and returns the launch's error -- and releases what it made.  model_d, model_S: the
// model's axes and sources as ResidentPoints::bind takes them (< 0: the grid model's).
using GridFold = std::function<hipError_t(const int32_t*)>;

template <class Step>
int grid_reduce(bi_ctx* c, const char* who, int model_d, int model_S, int64_t E, const int64_t* dataset, GridArgs a, int64_t n_total,
                const int32_t* var_kind, const int32_t* var_index, const double* z0, const double* scale0, const double* unit, const double* nodes,
                const double* term, const double* logw, int64_t chunk, double* log_marginal, double* profile, int64_t* argmax, int64_t* counters,
                Step&& step) {
    const size_t nn = (size_t)n_total;
    const int64_t G = E * a.GK;
    if (chunk == 0) chunk = kGridDefaultChunk;
    chunk = std::min(chunk, G);
    const size_t nc = (size_t)chunk;
    ResidentPoints pts;
    ScratchBuf b_nodes, b_term, b_logw, b_p, b_q;
    int rc;
    // (host copies that live until the uploads have been waited for)
    const std::vector<double> h_nodes(nodes, nodes + nn), h_term = host_copy(term, term ? nn : 0, 0.0), h_logw = host_copy(logw, logw ? nn : 0, 0.0);
    if ((rc = pts.bind(c, a, E, chunk, a.F, var_kind, var_index, z0, scale0, unit, dataset, model_d, model_S)) || (rc = dev_upload(c, b_nodes, h_nodes)) ||
        (term && (rc = dev_upload(c, b_term, h_term))) || (logw && (rc = dev_upload(c, b_logw, h_logw))))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((term && (rc = dev_alloc(c, b_p, nc * sizeof(double)))) || (logw && (rc = dev_alloc(c, b_q, nc * sizeof(double))))) return rc;
    a.nodes = (const double*)b_nodes.p;
    a.term = term ? (const double*)b_term.p : nullptr;
    a.logw = logw ? (const double*)b_logw.p : nullptr;
    a.p = term ? (double*)b_p.p : nullptr;
    a.q = logw ? (double*)b_q.p : nullptr;
    a.ll = (const double*)pts.llp.p;
    GridState st;
    if ((rc = grid_state_begin(c, st, a, G / a.R))) return rc;
    if (counters) counters[0] = counters[1] = counters[2] = counters[3] = 0;

    for (a.g0 = 0; a.g0 < G; a.g0 += chunk) {
        a.n = std::min(chunk, G - a.g0);
        grid_chunk_cells(a);
        launch_grid_points(c, a);
        HIP_TRY(c, hipGetLastError());                          // (nothing is launched after a failed launch)
        hipError_t e = hipSuccess;
        const GridFold fold = [&](const int32_t* status) {
            if (counters) ++counters[0];
            a.st = status;
            launch_grid_reduce(c, a);
            return e = hipGetLastError();
        };
        if ((rc = step(pts, a.n, counters, fold))) return rc;
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s (reduce): %s", who, hipGetErrorString(e));
    }
    return grid_state_end(c, a, log_marginal, profile, argmax, counters ? &counters[2] : nullptr);
}

// the grid model's step: the resident planner and bi_run_plan; the plan goes once the reduction has been queued
int grid_step_plan(bi_ctx* c, ResidentPoints& pts, int64_t n, int64_t* counters, const GridFold& fold) {
    bi_plan* plan = nullptr;
    int rc = pts.evaluate(c, n, "bi_grid_reduce", &plan, counters);
    if (rc) return rc;
    (void)fold((const int32_t*)plan->status.p);
    bi_plan_destroy(c, plan);                                   // (waits for the stream: the reduction reads the plan's status words)
    return BI_OK;
}

// The source-wise model's step: route 0 PlannedItems::queue (one work item per point, bi_sourcewise_plan.h), route 1
// ScanItems::queue (the matrix-core scan route, bi_sourcewise_scan.h); both leave the planner's status words where they were
// written, and nothing is made per chunk.  The buffers are sized by the first chunk, the largest.
struct GridStepSourcewise {
    bi_ctx* c;
    int route;
    PlannedItems points;
    ScanItems scan;
    bool ready = false;
    const char* who;
    GridStepSourcewise(bi_ctx* ctx, int r, const char* w = "bi_grid_reduce_sourcewise") : c(ctx), route(r), points(ctx), scan(ctx), who(w) {}

    int operator()(ResidentPoints& pts, int64_t n, int64_t* counters, const GridFold& fold) {
        int rc;
        if (!ready && (rc = route == 1 ? scan.init(n) : points.init(n))) return rc;
        ready = true;
        const double* zp = c->fac.d > 0 ? (const double*)pts.zp.p : nullptr;
        int64_t launches = 0;
        if (route == 1) {
            int64_t ctr[5] = {0, 0, 0, 0, 0};
            if ((rc = scan.queue(n, zp, (const double*)pts.rsp.p, (const int64_t*)pts.dsp.p, (double*)pts.llp.p, who, ctr))) return rc;
            launches = ctr[3];
        } else if ((rc = points.queue(n, zp, (const double*)pts.rsp.p, (const int64_t*)pts.dsp.p, (double*)pts.llp.p, who, &launches)))
            return rc;
        if (counters) { counters[1] += n; counters[3] += launches; }
        (void)fold((const int32_t*)(route == 1 ? scan.pt.status.p : points.status.p));
        return BI_OK;
    }
};

// true: a * b fits below `limit` (a, b >= 1), and *out = a * b
bool grid_mul(int64_t a, int64_t b, int64_t limit, int64_t* out) {
    if (a > limit / b) return false;
    *out = a * b;
    return *out <= limit;
}

// The argument checks the two entry points share, reported under `who`, and the grid's shape into a / n_total; d, S: the model's
int grid_check_args(bi_ctx* c, const char* who, int d, int S, int64_t E, int F, int n_keep, const int32_t* var_kind, const int32_t* var_index,
                    const double* z0, const double* scale0, const double* unit, const int32_t* n_nodes, const double* nodes, const double* term,
                    const double* logw, int64_t chunk, const double* log_marginal, const double* profile, const int64_t* argmax, GridArgs& a,
                    int64_t& n_total) {
    int rc;
    if (F < 1 || F > kGridMaxVars) return fail(c, BI_ERR_INVALID, "%s: need 1 <= F <= %d variables (got %d)", who, kGridMaxVars, F);
    if (n_keep < 0 || n_keep > F) return fail(c, BI_ERR_INVALID, "%s: n_keep must lie in [0, F = %d] (got %d)", who, F, n_keep);
    if (E < 1) return fail(c, BI_ERR_INVALID, "%s: need E >= 1 (got %lld)", who, (long long)E);
    if (chunk < 0 || chunk > kGridMaxChunk) return fail(c, BI_ERR_INVALID, "%s: chunk must lie in [0, 2^26] (got %lld)", who, (long long)chunk);
    if (!var_kind || !var_index || !scale0 || !unit || (d > 0 && !z0) || !n_nodes || !nodes || !log_marginal || !profile || !argmax)
        return fail(c, BI_ERR_INVALID, "%s: NULL argument", who);
    a.F = F; a.n_keep = n_keep;
    for (int j = 0; j < F; ++j) {
        if ((rc = check_variable(c, who, j, var_kind, var_index, true, d, S))) return rc;
        if (n_nodes[j] < 1) return fail(c, BI_ERR_INVALID, "%s: variable %d has %d nodes: need at least 1", who, j, (int)n_nodes[j]);
        a.n_nodes[j] = n_nodes[j];
    }
    int64_t K = 1, R = 1, cells = 0, G = 0;
    for (int j = 0; j < F; ++j) {
        a.node_off[j] = n_total;
        n_total += n_nodes[j];
        if (!grid_mul(j < n_keep ? K : R, n_nodes[j], kGridMaxPoints, j < n_keep ? &K : &R))
            return fail(c, BI_ERR_INVALID, "%s: the grid has more than 2^48 points", who);
    }
    if (!grid_mul(E, K, kGridMaxCells, &cells))
        return fail(c, BI_ERR_INVALID, "%s: E * K (%lld dataset entries x %lld kept points) is more than 2^24 cells", who, (long long)E, (long long)K);
    if (!grid_mul(cells, R, kGridMaxPoints, &G)) return fail(c, BI_ERR_INVALID, "%s: the grid has more than 2^48 points", who);
    for (int64_t stride = 1, j = F - 1; j >= 0; --j) {
        a.stride[j] = stride;
        stride *= n_nodes[j];
    }
    a.R = R; a.GK = K * R;
    for (int64_t i = 0; i < n_total; ++i) {
        if (!std::isfinite(nodes[i])) return fail(c, BI_ERR_INVALID, "%s: node %lld is not finite (%g)", who, (long long)i, nodes[i]);
        if (term && !(term[i] < std::numeric_limits<double>::infinity()))
            return fail(c, BI_ERR_INVALID, "%s: term %lld is %g: a term is finite or -inf", who, (long long)i, term[i]);
        if (logw && !(logw[i] < std::numeric_limits<double>::infinity()))
            return fail(c, BI_ERR_INVALID, "%s: logw %lld is %g: a log weight is finite or -inf", who, (long long)i, logw[i]);
    }
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_grid_reduce(bi_ctx* c, int64_t E, const int64_t* dataset, int F, int n_keep, const int32_t* var_kind, const int32_t* var_index,
                   const double* z0, const double* scale0, const double* unit, const int32_t* n_nodes, const double* nodes,
                   const double* term, const double* logw, int64_t chunk, double* log_marginal, double* profile, int64_t* argmax,
                   int64_t* counters) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    c->plan_refused = 0;
    GridArgs a{};
    int64_t n_total = 0;
    if ((rc = grid_check_args(c, "bi_grid_reduce", c->d, c->S, E, F, n_keep, var_kind, var_index, z0, scale0, unit, n_nodes, nodes, term, logw, chunk,
                              log_marginal, profile, argmax, a, n_total)))
        return rc;
    if ((rc = check_single_set(c, "bi_grid_reduce", "dataset entry", E, dataset)) ||
        (rc = check_entry_datasets(c, "bi_grid_reduce", "entry", E, dataset, c->T)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        return grid_reduce(c, "bi_grid_reduce", -1, -1, E, dataset, a, n_total, var_kind, var_index, z0, scale0, unit, nodes, term, logw, chunk,
                           log_marginal, profile, argmax, counters,
                           [&](ResidentPoints& pts, int64_t n, int64_t* ctr, const GridFold& fold) { return grid_step_plan(c, pts, n, ctr, fold); });
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "bi_grid_reduce: out of host memory");
    }
}

int bi_grid_reduce_sourcewise(bi_ctx* c, int64_t E, const int64_t* dataset, int F, int n_keep, const int32_t* var_kind, const int32_t* var_index,
                              const double* z0, const double* scale0, const double* unit, const int32_t* n_nodes, const double* nodes,
                              const double* term, const double* logw, int64_t chunk, int route, double* log_marginal, double* profile,
                              int64_t* argmax, int64_t* counters) {
    const char* who = "bi_grid_reduce_sourcewise";
    int rc = fac_check(c, who, true);
    if (rc) return rc;
    GridArgs a{};
    int64_t n_total = 0;
    if ((rc = grid_check_args(c, who, c->fac.d, c->fac.S, E, F, n_keep, var_kind, var_index, z0, scale0, unit, n_nodes, nodes, term, logw, chunk,
                              log_marginal, profile, argmax, a, n_total)) ||
        (rc = check_entry_datasets(c, who, "entry", E, dataset, c->fac.T)))
        return rc;
    if (route < -1 || route > 1) return fail(c, BI_ERR_INVALID, "%s: route is -1 (the scan route where the model is eligible), 0 (points) or 1 (scan), not %d", who, route);
    if (route < 0) route = sourcewise_scan_refusal(c) == 0 ? 1 : 0;
    if (route == 1 && (rc = sourcewise_scan_check(c, who))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        GridStepSourcewise step(c, route);
        rc = grid_reduce(c, who, c->fac.d, c->fac.S, E, dataset, a, n_total, var_kind, var_index, z0, scale0, unit, nodes, term, logw, chunk,
                         log_marginal, profile, argmax, counters, step);
        if (rc) (void)hipStreamSynchronize(c->stream);          // (the step's buffers go with the scope)
        if (counters) counters[4] = route;
        return rc;
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "%s: out of host memory", who);
    }
}

// ... on the event store (bi_sourcewise_events.h): the same loop, PlannedItems in its event mode
int bi_grid_reduce_sourcewise_events(bi_ctx* c, int64_t E, const int64_t* dataset, int F, int n_keep, const int32_t* var_kind,
                                     const int32_t* var_index, const double* z0, const double* scale0, const double* unit, const int32_t* n_nodes,
                                     const double* nodes, const double* term, const double* logw, int64_t chunk, int route, double* log_marginal,
                                     double* profile, int64_t* argmax, int64_t* counters) {
    const char* who = "bi_grid_reduce_sourcewise_events";
    int rc = events_routes_check(c, who, "bi_grid_reduce_sourcewise");
    if (rc) return rc;
    GridArgs a{};
    int64_t n_total = 0;
    if ((rc = grid_check_args(c, who, c->fac.d, c->fac.S, E, F, n_keep, var_kind, var_index, z0, scale0, unit, n_nodes, nodes, term, logw, chunk,
                              log_marginal, profile, argmax, a, n_total)) ||
        (rc = check_entry_datasets(c, who, "entry", E, dataset, c->fac.ev_T)))
        return rc;
    if (route < -1 || route > 1) return fail(c, BI_ERR_INVALID, "%s: route is -1 (the route this store is evaluated on: 0), 0 (points) or 1 (scan), not %d", who, route);
    if (route == 1)
        return fail(c, BI_ERR_INVALID, "%s: route 1 is not available: the matrix-core scan route does not read the event store (route 0 or -1)", who);
    route = 0;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        GridStepSourcewise step(c, route, who);
        rc = grid_reduce(c, who, c->fac.d, c->fac.S, E, dataset, a, n_total, var_kind, var_index, z0, scale0, unit, nodes, term, logw, chunk,
                         log_marginal, profile, argmax, counters, step);
        if (rc) (void)hipStreamSynchronize(c->stream);          // (the step's buffers go with the scope)
        if (counters) counters[4] = route;
        return rc;
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "%s: out of host memory", who);
    }
}

// the reduction kernels of bi_grid_reduce on caller data: t [cells][R] in the place of ll + p, q [cells][R] or NULL, folded in
// chunks of `chunk` values (0: all at once)
int bi_selftest_grid_reduce(bi_ctx* c, int64_t cells, int64_t R, int64_t chunk, const double* t, const double* q, double* log_marginal,
                            double* profile, int64_t* argmax) {
    if (!c || cells < 1 || cells > kGridMaxCells || R < 1 || R > ((int64_t)1 << 28) / cells || chunk < 0 || !t || !log_marginal || !profile || !argmax)
        return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t G = cells * R;
    if (chunk == 0 || chunk > G) chunk = G;
    ScratchBuf dt, dq;
    int rc;
    if ((rc = dev_alloc(c, dt, (size_t)G * 8)) || (q && (rc = dev_alloc(c, dq, (size_t)G * 8)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(dt.p, t, (size_t)G * 8, hipMemcpyHostToDevice, c->stream));
    if (q) HIP_TRY(c, hipMemcpyAsync(dq.p, q, (size_t)G * 8, hipMemcpyHostToDevice, c->stream));
    GridArgs a{};
    a.R = R;
    GridState st;
    if ((rc = grid_state_begin(c, st, a, cells))) return rc;
    for (a.g0 = 0; a.g0 < G; a.g0 += chunk) {
        a.n = std::min(chunk, G - a.g0);
        grid_chunk_cells(a);
        a.ll = (const double*)dt.p + a.g0;
        a.q = q ? (double*)dq.p + a.g0 : nullptr;
        launch_grid_reduce(c, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            return fail(c, BI_ERR_HIP, "bi_selftest_grid_reduce: %s", hipGetErrorString(e));
        }
    }
    rc = grid_state_end(c, a, log_marginal, profile, argmax, nullptr);
    if (rc) (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // extern "C"
