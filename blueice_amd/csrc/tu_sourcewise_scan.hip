// tu_sourcewise_scan.hip -- translation unit of the scan planner of source-wise points: k_sourcewise_scan_key, k_sourcewise_scan_cut,
// k_sourcewise_scan_groups and k_sourcewise_scan_fill (bi_k_sourcewise_scan.h).
// See bi_common.h for how the library is split.
#include "bi_common.h"
#include "bi_k_sourcewise_scan.h"

void launch_sourcewise_scan_key(bi_ctx* c, const SourcewiseScanArgs& a) {
    hipLaunchKernelGGL(k_sourcewise_scan_key, dim3((unsigned)((a.n * a.SC + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

void launch_sourcewise_scan_cut(bi_ctx* c, int64_t* gstart, int64_t n, int64_t cut) {
    hipLaunchKernelGGL(k_sourcewise_scan_cut, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, gstart, n, cut);
}

void launch_sourcewise_scan_groups(bi_ctx* c, const SourcewiseScanArgs& a) {
    hipLaunchKernelGGL(k_sourcewise_scan_groups, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
}

void launch_sourcewise_scan_fill(bi_ctx* c, const SourcewiseScanArgs& a) {
    const size_t lds = (size_t)a.NR * kSwScanFillPitch * sizeof(double) + (size_t)kSwScanFillThreads * sizeof(int64_t);
    hipLaunchKernelGGL(k_sourcewise_scan_fill, dim3((unsigned)((a.n_valid + kSwScanFillThreads - 1) / kSwScanFillThreads)),
                       dim3(kSwScanFillThreads), lds, c->stream, a);
}
