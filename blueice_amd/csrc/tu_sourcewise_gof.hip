// tu_sourcewise_gof.hip -- translation unit of k_sourcewise_gof<SC, EM, NT> (bi_k_sourcewise.h): half-deviance and Pearson's chi2
// of one point of a source-wise model per item.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise.h"

namespace {

template <int SC>
int launch_gof_sc(bi_ctx* c, int EM, const FactoredArgs& a, dim3 grid, bool nt) {
    switch (EM) {
        case 1:
            if (nt) hipLaunchKernelGGL((k_sourcewise_gof<SC, 1, true>), grid, dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL((k_sourcewise_gof<SC, 1, false>), grid, dim3(kThreads), 0, c->stream, a);
            return BI_OK;
        case 2:
            if (nt) hipLaunchKernelGGL((k_sourcewise_gof<SC, 2, true>), grid, dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL((k_sourcewise_gof<SC, 2, false>), grid, dim3(kThreads), 0, c->stream, a);
            return BI_OK;
        case 3:
            if (nt) hipLaunchKernelGGL((k_sourcewise_gof<SC, 3, true>), grid, dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL((k_sourcewise_gof<SC, 3, false>), grid, dim3(kThreads), 0, c->stream, a);
            return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_gof(bi_ctx* c, int SC, int EM, const FactoredArgs& a, dim3 grid, bool nt) {
    EventScope ev(c);
    switch (SC) {
        case 2: return launch_gof_sc<2>(c, EM, a, grid, nt);
        case 4: return launch_gof_sc<4>(c, EM, a, grid, nt);
        case 8: return launch_gof_sc<8>(c, EM, a, grid, nt);
    }
    return BI_ERR_INVALID;
}
