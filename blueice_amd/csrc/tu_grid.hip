// tu_grid.hip -- translation unit of the gridded likelihood's kernels k_grid_points / k_grid_init / k_grid_reduce /
// k_grid_finish (bi_k_grid.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_grid.h"

// one thread per point of the chunk
void launch_grid_points(bi_ctx* c, const GridArgs& a) {
    hipLaunchKernelGGL(k_grid_points, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

// one block (cpb = 1) or one wave (cpb = 4) per cell the chunk touches
void launch_grid_reduce(bi_ctx* c, const GridArgs& a) {
    hipLaunchKernelGGL(k_grid_reduce, dim3((unsigned)((a.n_cells + a.cpb - 1) / a.cpb)), dim3(kThreads), 0, c->stream, a);
}

void launch_grid_init(bi_ctx* c, const GridArgs& a) {
    hipLaunchKernelGGL(k_grid_init, dim3((unsigned)((a.cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

void launch_grid_finish(bi_ctx* c, const GridArgs& a) {
    hipLaunchKernelGGL(k_grid_finish, dim3((unsigned)((a.cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}
