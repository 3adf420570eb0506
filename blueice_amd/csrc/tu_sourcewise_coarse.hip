// tu_sourcewise_coarse.hip -- translation unit of k_sourcewise_coarse<SC, EM, PS> (bi_k_sourcewise_coarse.h): the expectation of a
// source-wise model summed over the groups of a coarse binning.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_coarse.h"

namespace {

template <int SC, int EM>
void launch_coarse_v(bi_ctx* c, bool per_source, const SourcewiseCoarseArgs& a, dim3 grid) {
    if (per_source) hipLaunchKernelGGL((k_sourcewise_coarse<SC, EM, true>), grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_sourcewise_coarse<SC, EM, false>), grid, dim3(kThreads), 0, c->stream, a);
    launch_coarse_finish(c, a.g);
}

template <int SC>
int launch_coarse_sc(bi_ctx* c, int EM, bool per_source, const SourcewiseCoarseArgs& a, dim3 grid) {
    switch (EM) {
        case 1: launch_coarse_v<SC, 1>(c, per_source, a, grid); return BI_OK;
        case 2: launch_coarse_v<SC, 2>(c, per_source, a, grid); return BI_OK;
        case 3: launch_coarse_v<SC, 3>(c, per_source, a, grid); return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_coarse(bi_ctx* c, int SC, int EM, bool per_source, const SourcewiseCoarseArgs& a, int64_t n_items) {
    EventScope ev(c);
    const dim3 grid((unsigned)(a.g.CR * a.g.nsplit * a.g.n_xt), 1, (unsigned)n_items);
    switch (SC) {
        case 2: return launch_coarse_sc<2>(c, EM, per_source, a, grid);
        case 4: return launch_coarse_sc<4>(c, EM, per_source, a, grid);
        case 8: return launch_coarse_sc<8>(c, EM, per_source, a, grid);
    }
    return BI_ERR_INVALID;
}
