// tu_sourcewise_plan.hip -- translation unit of the source-wise model's device planner k_sourcewise_plan<SC>
// (bi_k_sourcewise_plan.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_plan.h"

int launch_sourcewise_plan(bi_ctx* c, int SC, const SourcewisePlanArgs& a) {
    EventScope ev(c);
    const dim3 grid((unsigned)((a.n * SC + kThreads - 1) / kThreads));
    switch (SC) {
        case 2: hipLaunchKernelGGL(k_sourcewise_plan<2>, grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 4: hipLaunchKernelGGL(k_sourcewise_plan<4>, grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 8: hipLaunchKernelGGL(k_sourcewise_plan<8>, grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
    }
    return BI_ERR_INVALID;
}

int launch_sourcewise_plan_events(bi_ctx* c, int SC, const SourcewisePlanArgs& a) {
    EventScope ev(c);
    const dim3 grid((unsigned)((a.n * SC + kThreads - 1) / kThreads));
    switch (SC) {
        case 2: hipLaunchKernelGGL((k_sourcewise_plan<2, false, true>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 4: hipLaunchKernelGGL((k_sourcewise_plan<4, false, true>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 8: hipLaunchKernelGGL((k_sourcewise_plan<8, false, true>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
    }
    return BI_ERR_INVALID;
}

int launch_sourcewise_plan_nonempty(bi_ctx* c, int SC, const SourcewisePlanArgs& a) {
    EventScope ev(c);
    const dim3 grid((unsigned)((a.n * SC + kThreads - 1) / kThreads));
    switch (SC) {
        case 2: hipLaunchKernelGGL((k_sourcewise_plan<2, true>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 4: hipLaunchKernelGGL((k_sourcewise_plan<4, true>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
        case 8: hipLaunchKernelGGL((k_sourcewise_plan<8, true>), grid, dim3(kThreads), 0, c->stream, a); return BI_OK;
    }
    return BI_ERR_INVALID;
}
