// tu_sampler.hip -- translation unit of the ensemble sampler's kernels k_stretch_propose / k_stretch_start_density /
// k_stretch_accept (bi_k_sampler.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sampler.h"

// n = E * W / 2 threads (h = 0, 1), E * W with h = -1 (the start positions)
void launch_stretch_propose(bi_ctx* c, const StretchArgs& a) {
    const int64_t n = a.h < 0 ? a.E * a.W : a.E * (a.W / 2);
    hipLaunchKernelGGL(k_stretch_propose, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

void launch_stretch_start_density(bi_ctx* c, const StretchArgs& a) {
    const int64_t n = a.E * a.W;
    hipLaunchKernelGGL(k_stretch_start_density, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

void launch_stretch_accept(bi_ctx* c, const StretchArgs& a) {
    const int64_t n = a.E * (a.W / 2);
    hipLaunchKernelGGL(k_stretch_accept, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}
