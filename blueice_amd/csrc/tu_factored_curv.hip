// tu_factored_curv.hip -- translation unit of the observed form of the source-wise model's curvature kernel,
// k_factored_curv<SC, EM, false, PS, PANEL> (bi_k_factored_curv.h): the classes with at most 16 basis columns as one launch, <8, 2>
// in four panels of two sources and <8, 3> in eight panels of one.  The Fisher form is tu_factored_fisher.hip's, so that the two
// compile side by side.  See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_factored_curv.h"

int launch_factored_curv_observed(bi_ctx* c, int SC, int EM, int panel, const FactoredArgs& a, dim3 grid) {
    return launch_curv_form<false>(c, SC, EM, panel, a, grid);
}
