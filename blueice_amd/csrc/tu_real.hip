// tu_real.hip -- translation unit of the real-valued-counts kernels k_morph_real<G, NT> and k_real_expect (bi_k_real.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_real.h"

namespace {

template <int G>
void launch_real_g(bi_ctx* c, const HessArgs& a, dim3 grid, bool nt) {
    if (nt) hipLaunchKernelGGL((k_morph_real<G, true>), grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_morph_real<G, false>), grid, dim3(kThreads), 0, c->stream, a);
}

}  // namespace

int launch_morph_real(bi_ctx* c, int G, const HessArgs& a, dim3 grid, bool nt) {
    EventScope ev(c);
    switch (G) {
        case 1: launch_real_g<1>(c, a, grid, nt); return BI_OK;
        case 4: launch_real_g<4>(c, a, grid, nt); return BI_OK;
        case 8: launch_real_g<8>(c, a, grid, nt); return BI_OK;
        case 16: launch_real_g<16>(c, a, grid, nt); return BI_OK;
    }
    return BI_ERR_INVALID;
}

void launch_real_expect(bi_ctx* c, const RealExpectArgs& a, int64_t n_items) {
    EventScope ev(c);
    const dim3 grid((unsigned)((a.B + kThreads - 1) / kThreads), (unsigned)n_items);
    hipLaunchKernelGGL(k_real_expect, grid, dim3(kThreads), 0, c->stream, a);
}
