// bi_k_sourcewise_coarse.h -- coarse views of a source-wise model: its expectation summed over tensor-product groups of fine
// bins (bi_sourcewise_set_coarse_binning, bi_sourcewise_expected_coarse; host half bi_sourcewise_coarse.h).  Translation unit
// tu_sourcewise_coarse.hip.
//
// k_sourcewise_coarse<SC, EM, PS>: the blocks, the lanes and the order of every sum are k_morph_coarse's (bi_k_coarse.h): one
//   block per (item, coarse row, share, x-tile), lanes along the last analysis axis (fine bin b = r L + x, 8-byte loads of
//   consecutive doubles), TY = 256 / TX sub-rows that walk the fine rows lo + ty, lo + ty + TY, ... of the block's share in list
//   order, the TY sums of a column added in ty order through LDS, partial[item][R][coarse row][share][x] -- so k_coarse_finish
//   and k_coarse_finish_wide serve unchanged, and TX, n_xt, nsplit and wide are coarse_geometry's (bi_coarse.h): the binning and
//   the CU count alone, never the number of points.
//   What differs is the fine bin's expectation.  The grid kernel forms one flat sum over corner rows that lie at stride S; here
//   a source's rows are a contiguous run of 2^e_s, and tau_s and mu are formed by sourcewise_chain_bin (bi_k_sourcewise.h):
//   sourcewise_chain's statements for one bin per lane, so mu_b has the bits every other source-wise kernel forms.
//     PS = false   one per-lane sum of mu_b; R = 1.
//     PS = true    SC per-lane sums of r_s * tau_s,b (the single multiply k_sourcewise_expect writes), all formed in the same
//                  block, so a point's rows are read once; the sums of the a.g.R = S sources the model has go out as R groups.
//                  LDS: SC x 256 doubles, 16 KiB at most.
// No floating-point atomic anywhere; a repeated identical call is bitwise identical, and a point's cells do not depend on the
// batch it came in.  Registers, LDS and scratch of the 18 instantiations: profiles/sourcewise_coarse_kernel_resources.txt (no
// scratch in any).
#pragma once

#include "bi_k_sourcewise.h"

namespace {

template <int SC, int EM, bool PS>
__global__ __launch_bounds__(kThreads) void k_sourcewise_coarse(SourcewiseCoarseArgs x) {
    const FactoredArgs& a = x.f;
    const CoarseArgs& g = x.g;
    constexpr int NSUM = PS ? SC : 1;
    const int TX = 1 << g.tx_shift, TY = kThreads >> g.tx_shift;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.tx_shift;      // (TX >= 64: ty is wave-uniform)
    unsigned bx = blockIdx.x;
    const int xt = (int)(bx % (unsigned)g.n_xt);
    bx /= (unsigned)g.n_xt;
    const int split = (int)(bx % (unsigned)g.nsplit);
    const int64_t crow = bx / (unsigned)g.nsplit;
    const int64_t item = blockIdx.z;
    const int64_t* __restrict__ rowoff = a.rowoff + item * a.NR;
    const double* __restrict__ coef = a.coef + item * a.NR * (1 + EM);
    const double* __restrict__ rate = a.rates + item * SC;
    const int64_t xr = (int64_t)xt * TX + tx;
    const bool live = xr < g.Lx;
    const int64_t lo = g.row_off[crow], n = g.row_off[crow + 1] - lo;
    const int64_t per = (n + g.nsplit - 1) / g.nsplit;
    const int64_t i0 = (int64_t)split * per, i1 = i0 + per < n ? i0 + per : n;

    double sum[NSUM];
#pragma unroll
    for (int s = 0; s < NSUM; ++s) sum[s] = 0.0;
    if (live)
        for (int64_t i = i0 + ty; i < i1; i += TY) {
            double tau[SC], mu;
            sourcewise_chain_bin<SC, EM>(a, rowoff, coef, rate, (int64_t)g.row_list[lo + i] * g.L + g.x_lo + xr, tau, mu);
            if constexpr (PS) {
#pragma unroll
                for (int s = 0; s < SC; ++s) sum[s] += rate[s] * tau[s];
            } else {
                sum[0] += mu;
            }
        }

    const int64_t column = g.CR * g.nsplit * g.Lx;                              // from one group's partials to the next one's
    double* __restrict__ out = g.partial + (item * g.R * column + (crow * g.nsplit + split) * g.Lx + xr);
    if (TY == 1) {
        if (live) {
#pragma unroll
            for (int s = 0; s < NSUM; ++s)
                if (s < g.R) out[s * column] = sum[s];
        }
        return;
    }
    __shared__ double s_acc[NSUM][kThreads];
#pragma unroll
    for (int s = 0; s < NSUM; ++s) s_acc[s][threadIdx.x] = sum[s];
    __syncthreads();
    if (ty == 0 && live) {
#pragma unroll
        for (int s = 0; s < NSUM; ++s) {
            if (s < g.R) {
                double t = s_acc[s][tx];
                for (int j = 1; j < TY; ++j) t += s_acc[s][j * TX + tx];
                out[s * column] = t;
            }
        }
    }
}

}  // namespace
