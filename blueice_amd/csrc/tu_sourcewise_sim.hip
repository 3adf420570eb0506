// tu_sourcewise_sim.hip -- translation unit of the event-toy kernels of a source-wise model (bi_k_sourcewise_sim.h):
// k_sourcewise_pmf<SC, EM>, k_sourcewise_sim_counts, _room, _first, _events.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_sim.h"

namespace {

template <int SC>
int launch_pmf_sc(bi_ctx* c, int EM, const SourcewisePmfArgs& a, dim3 grid) {
    switch (EM) {
        case 1: hipLaunchKernelGGL((k_sourcewise_pmf<SC, 1>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 2: hipLaunchKernelGGL((k_sourcewise_pmf<SC, 2>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 3: hipLaunchKernelGGL((k_sourcewise_pmf<SC, 3>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_pmf(bi_ctx* c, int SC, int EM, const SourcewisePmfArgs& a, int64_t n_items) {
    const dim3 grid((unsigned)a.f.n_tiles, (unsigned)n_items);
    switch (SC) {
        case 2: return launch_pmf_sc<2>(c, EM, a, grid);
        case 4: return launch_pmf_sc<4>(c, EM, a, grid);
        case 8: return launch_pmf_sc<8>(c, EM, a, grid);
    }
    return BI_ERR_INVALID;
}

void launch_sourcewise_sim_counts(bi_ctx* c, const SourcewiseSimArgs& a) {
    hipLaunchKernelGGL(k_sourcewise_sim_counts, dim3((unsigned)((a.T * a.sim.S + 255) / 256)), dim3(256), 0, c->stream, a);
}

void launch_sourcewise_sim_room(bi_ctx* c, const SourcewiseSimArgs& a) {
    hipLaunchKernelGGL(k_sourcewise_sim_room, dim3((unsigned)((a.T + 1 + 255) / 256)), dim3(256), 0, c->stream, a);
}

void launch_sourcewise_sim_first(bi_ctx* c, const SourcewiseSimArgs& a) {
    hipLaunchKernelGGL(k_sourcewise_sim_first, dim3((unsigned)((a.T + 255) / 256)), dim3(256), 0, c->stream, a);
}

void launch_sourcewise_sim_events(bi_ctx* c, const SourcewiseSimArgs& a) {
    hipLaunchKernelGGL(k_sourcewise_sim_events, dim3((unsigned)((a.ncols + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}
