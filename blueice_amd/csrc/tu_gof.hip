// tu_gof.hip -- translation unit of the goodness-of-fit kernels k_morph_gof<NT> and k_morph_expect (bi_k_gof.h).  See
// bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_gof.h"

void launch_morph_gof(bi_ctx* c, const HessArgs& a, dim3 grid, bool nt) {
    EventScope ev(c);
    if (nt) hipLaunchKernelGGL((k_morph_gof<true>), grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_morph_gof<false>), grid, dim3(kThreads), 0, c->stream, a);
}

void launch_morph_expect(bi_ctx* c, const ExpectArgs& a, int64_t n_items) {
    EventScope ev(c);
    const dim3 grid((unsigned)((a.B + kThreads - 1) / kThreads), (unsigned)a.R, (unsigned)n_items);
    hipLaunchKernelGGL(k_morph_expect, grid, dim3(kThreads), 0, c->stream, a);
}
