// tu_sourcewise_nonempty.hip -- translation unit of the source-wise model's non-empty-bin form: k_sourcewise_nonempty<SC, EM, GRAD>
// and k_sourcewise_gather (bi_k_sourcewise_nonempty.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_nonempty.h"

namespace {

template <int SC, int EM>
void launch_nonempty_v(bi_ctx* c, bool grad, const SourcewiseNonemptyArgs& a, dim3 grid) {
    if (grad) hipLaunchKernelGGL((k_sourcewise_nonempty<SC, EM, true>), grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_sourcewise_nonempty<SC, EM, false>), grid, dim3(kThreads), 0, c->stream, a);
}

template <int SC>
int launch_nonempty_sc(bi_ctx* c, int EM, bool grad, const SourcewiseNonemptyArgs& a, dim3 grid) {
    switch (EM) {
        case 1: launch_nonempty_v<SC, 1>(c, grad, a, grid); return BI_OK;
        case 2: launch_nonempty_v<SC, 2>(c, grad, a, grid); return BI_OK;
        case 3: launch_nonempty_v<SC, 3>(c, grad, a, grid); return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_nonempty(bi_ctx* c, int SC, int EM, bool grad, const SourcewiseNonemptyArgs& a, dim3 grid) {
    EventScope ev(c);
    switch (SC) {
        case 2: return launch_nonempty_sc<2>(c, EM, grad, a, grid);
        case 4: return launch_nonempty_sc<4>(c, EM, grad, a, grid);
        case 8: return launch_nonempty_sc<8>(c, EM, grad, a, grid);
    }
    return BI_ERR_INVALID;
}

void launch_sourcewise_gather(bi_ctx* c, const SourcewiseGatherArgs& a, dim3 grid) {
    EventScope ev(c);
    hipLaunchKernelGGL(k_sourcewise_gather, grid, dim3(kThreads), 0, c->stream, a);
}
