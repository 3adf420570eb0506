// tu_fisher.hip -- translation unit of the expected-information kernel k_morph_fisher<G, DM, NT> (bi_k_fisher.h) and its
// instantiation table.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_fisher.h"

// G coefficient columns (padded 1 + D), DM first-order columns (padded D); BI_ERR_INVALID for a pair without a variant
int launch_morph_fisher(bi_ctx* c, int G, int DM, const HessArgs& a, dim3 grid, bool nt) {
    EventScope ev(c);
#define BI_FISHER(GG, MM)                                                                                     \
    do {                                                                                                      \
        if (nt) hipLaunchKernelGGL((k_morph_fisher<GG, MM, true>), grid, dim3(kThreads), 0, c->stream, a);     \
        else hipLaunchKernelGGL((k_morph_fisher<GG, MM, false>), grid, dim3(kThreads), 0, c->stream, a);       \
    } while (0)
    if (G == 4 && DM == 4) BI_FISHER(4, 4);
    else if (G == 8 && DM == 4) BI_FISHER(8, 4);
    else if (G == 8 && DM == 8) BI_FISHER(8, 8);
    else if (G == 16 && DM == 8) BI_FISHER(16, 8);
    else if (G == 16 && DM == 16) BI_FISHER(16, 16);
    else return BI_ERR_INVALID;
#undef BI_FISHER
    return BI_OK;
}
