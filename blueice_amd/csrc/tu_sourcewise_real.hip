// tu_sourcewise_real.hip -- translation unit of k_sourcewise_real<SC, EM, GRAD, NT> (bi_k_sourcewise_real.h): half-deviance of one
// point of a source-wise model against a real-valued dataset per item, and its gradient's sums.  See bi_common.h for how the
// library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_real.h"

namespace {

template <int SC, int EM>
void launch_sw_real_v(bi_ctx* c, bool grad, const FactoredArgs& a, dim3 grid, bool nt) {
    if (grad) {
        if (nt) hipLaunchKernelGGL((k_sourcewise_real<SC, EM, true, true>), grid, dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((k_sourcewise_real<SC, EM, true, false>), grid, dim3(kThreads), 0, c->stream, a);
    } else {
        if (nt) hipLaunchKernelGGL((k_sourcewise_real<SC, EM, false, true>), grid, dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((k_sourcewise_real<SC, EM, false, false>), grid, dim3(kThreads), 0, c->stream, a);
    }
}

template <int SC>
int launch_sw_real_sc(bi_ctx* c, int EM, bool grad, const FactoredArgs& a, dim3 grid, bool nt) {
    switch (EM) {
        case 1: launch_sw_real_v<SC, 1>(c, grad, a, grid, nt); return BI_OK;
        case 2: launch_sw_real_v<SC, 2>(c, grad, a, grid, nt); return BI_OK;
        case 3: launch_sw_real_v<SC, 3>(c, grad, a, grid, nt); return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_real(bi_ctx* c, int SC, int EM, bool grad, const FactoredArgs& a, dim3 grid, bool nt) {
    EventScope ev(c);
    switch (SC) {
        case 2: return launch_sw_real_sc<2>(c, EM, grad, a, grid, nt);
        case 4: return launch_sw_real_sc<4>(c, EM, grad, a, grid, nt);
        case 8: return launch_sw_real_sc<8>(c, EM, grad, a, grid, nt);
    }
    return BI_ERR_INVALID;
}
