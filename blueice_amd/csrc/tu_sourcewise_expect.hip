// tu_sourcewise_expect.hip -- translation unit of k_sourcewise_expect<SC, EM, PS, NT> (bi_k_sourcewise.h): the per-bin expectation
// of a source-wise model, written out.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise.h"

namespace {

template <int SC, int EM>
void launch_expect_v(bi_ctx* c, bool per_source, const SourcewiseExpectArgs& a, dim3 grid, bool nt) {
    if (per_source) {
        if (nt) hipLaunchKernelGGL((k_sourcewise_expect<SC, EM, true, true>), grid, dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((k_sourcewise_expect<SC, EM, true, false>), grid, dim3(kThreads), 0, c->stream, a);
    } else {
        if (nt) hipLaunchKernelGGL((k_sourcewise_expect<SC, EM, false, true>), grid, dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((k_sourcewise_expect<SC, EM, false, false>), grid, dim3(kThreads), 0, c->stream, a);
    }
}

template <int SC>
int launch_expect_sc(bi_ctx* c, int EM, bool per_source, const SourcewiseExpectArgs& a, dim3 grid, bool nt) {
    switch (EM) {
        case 1: launch_expect_v<SC, 1>(c, per_source, a, grid, nt); return BI_OK;
        case 2: launch_expect_v<SC, 2>(c, per_source, a, grid, nt); return BI_OK;
        case 3: launch_expect_v<SC, 3>(c, per_source, a, grid, nt); return BI_OK;
    }
    return BI_ERR_INVALID;
}

}  // namespace

int launch_sourcewise_expect(bi_ctx* c, int SC, int EM, bool per_source, const SourcewiseExpectArgs& a, int64_t n_items, bool nt) {
    EventScope ev(c);
    const dim3 grid((unsigned)a.f.n_tiles, (unsigned)n_items);
    switch (SC) {
        case 2: return launch_expect_sc<2>(c, EM, per_source, a, grid, nt);
        case 4: return launch_expect_sc<4>(c, EM, per_source, a, grid, nt);
        case 8: return launch_expect_sc<8>(c, EM, per_source, a, grid, nt);
    }
    return BI_ERR_INVALID;
}
