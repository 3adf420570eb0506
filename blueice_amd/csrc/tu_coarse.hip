// tu_coarse.hip -- translation unit of the coarse-view kernels k_morph_coarse, k_morph_coarse_jac<G>, k_coarse_finish(_wide),
// k_coarse_list and k_coarse_table (bi_k_coarse.h).  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_coarse.h"

// (no EventScope of its own: the launcher of the kernel that wrote a.partial holds one around the pair)
void launch_coarse_finish(bi_ctx* c, const CoarseArgs& a) {
    if (a.wide) hipLaunchKernelGGL(k_coarse_finish_wide, dim3((unsigned)a.n_out), dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(k_coarse_finish, dim3((unsigned)((a.n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

void launch_morph_coarse(bi_ctx* c, const CoarseArgs& a, int64_t n_items) {
    EventScope ev(c);
    const dim3 grid((unsigned)(a.CR * a.nsplit * a.n_xt), (unsigned)a.R, (unsigned)n_items);
    hipLaunchKernelGGL(k_morph_coarse, grid, dim3(kThreads), 0, c->stream, a);
    launch_coarse_finish(c, a);
}

// G coefficient columns per corner row (a.R = G: the finish kernels take the columns for groups); BI_ERR_INVALID for a G
// without a variant
int launch_morph_coarse_jac(bi_ctx* c, int G, const CoarseArgs& a, int64_t n_items) {
    if (a.R != G || (G != 4 && G != 8 && G != 16)) return BI_ERR_INVALID;
    EventScope ev(c);
    const dim3 grid((unsigned)(a.CR * a.nsplit * a.n_xt), 1, (unsigned)n_items);
    if (G == 4) hipLaunchKernelGGL(k_morph_coarse_jac<4>, grid, dim3(kThreads), 0, c->stream, a);
    else if (G == 8) hipLaunchKernelGGL(k_morph_coarse_jac<8>, grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(k_morph_coarse_jac<16>, grid, dim3(kThreads), 0, c->stream, a);
    launch_coarse_finish(c, a);
    return BI_OK;
}

void launch_coarse_list(bi_ctx* c, const CoarseListArgs& a, int64_t n, double* out) {
    EventScope ev(c);
    hipLaunchKernelGGL(k_coarse_list, dim3(64, (unsigned)n), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_coarse_table, dim3((unsigned)((n * a.C + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                       (const unsigned long long*)a.table, n * a.C, out);
}
