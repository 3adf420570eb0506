// tu_sourcewise_coarse_jac.hip -- translation unit of k_sourcewise_coarse_jac<SC, EM> (bi_k_sourcewise_coarse_jac.h): the sums of a
// source-wise model's basis columns over the groups of a coarse binning, from which the host forms the derivatives of every
// cell.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_coarse_jac.h"

namespace {

template <int SC>
int launch_coarse_jac_sc(bi_ctx* c, int EM, const SourcewiseCoarseJacArgs& a, dim3 grid) {
    switch (EM) {
        case 1: hipLaunchKernelGGL((k_sourcewise_coarse_jac<SC, 1>), grid, dim3(kThreads), 0, c->stream, a); break;
        case 2: hipLaunchKernelGGL((k_sourcewise_coarse_jac<SC, 2>), grid, dim3(kThreads), 0, c->stream, a); break;
        case 3: hipLaunchKernelGGL((k_sourcewise_coarse_jac<SC, 3>), grid, dim3(kThreads), 0, c->stream, a); break;
        default: return BI_ERR_INVALID;
    }
    launch_coarse_finish(c, a.g);
    return BI_OK;
}

}  // namespace

int launch_sourcewise_coarse_jac(bi_ctx* c, int SC, int EM, const SourcewiseCoarseJacArgs& a, int64_t n_items) {
    EventScope ev(c);
    const dim3 grid((unsigned)(a.g.CR * a.g.nsplit * a.g.n_xt), 1, (unsigned)n_items);
    switch (SC) {
        case 2: return launch_coarse_jac_sc<2>(c, EM, a, grid);
        case 4: return launch_coarse_jac_sc<4>(c, EM, a, grid);
        case 8: return launch_coarse_jac_sc<8>(c, EM, a, grid);
    }
    return BI_ERR_INVALID;
}
