// tu_factored_fisher.hip -- translation unit of the Fisher form of the source-wise model's curvature kernel,
// k_factored_curv<SC, EM, true, PS, PANEL> (bi_k_factored_curv.h), panelled as the observed form in tu_factored_curv.hip.
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_factored_curv.h"

int launch_factored_curv_fisher(bi_ctx* c, int SC, int EM, int panel, const FactoredArgs& a, dim3 grid) {
    return launch_curv_form<true>(c, SC, EM, panel, a, grid);
}
