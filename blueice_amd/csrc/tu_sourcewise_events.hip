// tu_sourcewise_events.hip -- translation unit of the source-wise model's event store: k_sourcewise_events<SC, EM, GRAD>
// (bi_k_sourcewise_events.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_events.h"

namespace {

template <int SC, int EM>
void launch_events_v(bi_ctx* c, bool grad, const SourcewiseEventsArgs& a, dim3 grid) {
    if (grad) hipLaunchKernelGGL((k_sourcewise_events<SC, EM, true>), grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_sourcewise_events<SC, EM, false>), grid, dim3(kThreads), 0, c->stream, a);
}

template <int SC>
int launch_events_sc(bi_ctx* c, int EM, bool grad, const SourcewiseEventsArgs& a, dim3 grid) {
    switch (EM) {
        case 1: launch_events_v<SC, 1>(c, grad, a, grid); return BI_OK;
        case 2: launch_events_v<SC, 2>(c, grad, a, grid); return BI_OK;
        case 3: launch_events_v<SC, 3>(c, grad, a, grid); return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_events(bi_ctx* c, int SC, int EM, bool grad, const SourcewiseEventsArgs& a, dim3 grid) {
    EventScope ev(c);
    switch (SC) {
        case 2: return launch_events_sc<2>(c, EM, grad, a, grid);
        case 4: return launch_events_sc<4>(c, EM, grad, a, grid);
        case 8: return launch_events_sc<8>(c, EM, grad, a, grid);
    }
    return BI_ERR_INVALID;
}
