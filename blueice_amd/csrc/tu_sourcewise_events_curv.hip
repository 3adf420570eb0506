// tu_sourcewise_events_curv.hip -- translation unit of the curvature kernel over the source-wise model's event store,
// k_sourcewise_events_curv<SC, EM, PS, PANEL> (bi_k_sourcewise_events_curv.h): the classes with at most 16 basis columns as one
// launch, <8, 2> in four panels of two sources and <8, 3> in eight panels of one.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_events_curv.h"

namespace {

template <int SC, int EM, int PANEL>
int launch_events_curv_panel(bi_ctx* c, int panel, const SourcewiseEventsArgs& a, dim3 grid) {
    constexpr int PS = factored_curv_panel_sources(SC, EM);
    if (panel == PANEL) {
        hipLaunchKernelGGL((k_sourcewise_events_curv<SC, EM, PS, PANEL>), grid, dim3(kThreads), 0, c->stream, a);
        return BI_OK;
    }
    if constexpr (PANEL + 1 < factored_curv_panels(SC, EM)) return launch_events_curv_panel<SC, EM, PANEL + 1>(c, panel, a, grid);
    return BI_ERR_INVALID;
}

template <int SC>
int launch_events_curv_sc(bi_ctx* c, int EM, int panel, const SourcewiseEventsArgs& a, dim3 grid) {
    switch (EM) {
        case 1: return launch_events_curv_panel<SC, 1, 0>(c, panel, a, grid);
        case 2: return launch_events_curv_panel<SC, 2, 0>(c, panel, a, grid);
        case 3: return launch_events_curv_panel<SC, 3, 0>(c, panel, a, grid);
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_events_curv(bi_ctx* c, int SC, int EM, int panel, const SourcewiseEventsArgs& a, dim3 grid) {
    EventScope ev(c);
    if (panel < 0) return BI_ERR_INVALID;
    switch (SC) {
        case 2: return launch_events_curv_sc<2>(c, EM, panel, a, grid);
        case 4: return launch_events_curv_sc<4>(c, EM, panel, a, grid);
        case 8: return launch_events_curv_sc<8>(c, EM, panel, a, grid);
    }
    return BI_ERR_INVALID;
}
