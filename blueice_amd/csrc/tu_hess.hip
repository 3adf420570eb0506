// tu_hess.hip -- translation unit of the Hessian kernel k_morph_hess<G, DM, UNB, NT> (bi_k_hess.h) and its instantiation
// table.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_hess.h"

// G coefficient columns (padded 1 + D + second-order columns), DM first-order columns (padded D); BI_ERR_INVALID for a
// pair without a variant
int launch_morph_hess(bi_ctx* c, int G, int DM, const HessArgs& a, dim3 grid, bool nt) {
    EventScope ev(c);
#define BI_HESS(GG, MM)                                                                                                 \
    do {                                                                                                                \
        if (c->unbinned) hipLaunchKernelGGL((k_morph_hess<GG, MM, true, false>), grid, dim3(kThreads), 0, c->stream, a); \
        else if (nt) hipLaunchKernelGGL((k_morph_hess<GG, MM, false, true>), grid, dim3(kThreads), 0, c->stream, a);     \
        else hipLaunchKernelGGL((k_morph_hess<GG, MM, false, false>), grid, dim3(kThreads), 0, c->stream, a);            \
    } while (0)
    if (G == 8 && DM == 4) BI_HESS(8, 4);
    else if (G == 8 && DM == 8) BI_HESS(8, 8);
    else if (G == 16 && DM == 4) BI_HESS(16, 4);
    else if (G == 16 && DM == 8) BI_HESS(16, 8);
    else if (G == 16 && DM == 16) BI_HESS(16, 16);
    else if (G == 32 && DM == 8) BI_HESS(32, 8);
    else if (G == 32 && DM == 16) BI_HESS(32, 16);
    else if (G == 64 && DM == 8) BI_HESS(64, 8);
    else return BI_ERR_INVALID;
#undef BI_HESS
    return BI_OK;
}
