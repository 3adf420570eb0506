// bi_k_sourcewise_coarse_jac.h -- the first derivatives of the coarse views of a source-wise model: per cell the sums the host
// contracts into d mu_C / d theta (bi_sourcewise_expected_coarse_jacobian; host half bi_sourcewise_coarse.h).  Translation unit
// tu_sourcewise_coarse_jac.hip.
//
// k_sourcewise_coarse_jac<SC, EM>: the blocks, the lanes, the shares, the sub-row walk and the partial layout are
//   k_sourcewise_coarse's (bi_k_sourcewise_coarse.h): one block per (item, coarse row, share, x-tile), lanes along the last
//   analysis axis with 8-byte loads, TY = 256 / TX sub-rows, geometry from coarse_geometry (the binning and the device alone).
//   Per fine bin, one pass over the item's rows with FacBatch's descriptors of order 1 (coef [NR][1 + EM]) forms, in
//   k_morph_factored's statement order (bi_k_factored.h),
//       tau_s   = sum_c w_c p_{s,c,b}             from coef[..][0]
//       ups_s,j = sum_c d_j w_c p_{s,c,b}         from coef[..][1 + j]
//       mu      = sum_s r_s tau_s                 exactly as sourcewise_chain_bin forms it (bi_k_sourcewise.h)
//   and adds them to per-lane sums in registers, in k_morph_factored's slot layout:
//       [0] sum mu_b       [1 + s] sum tau_s,b       [1 + SC + s EM + j] sum ups_s,j,b
//   Slot 0 goes through the chain and the order of additions of k_sourcewise_coarse<SC, EM, false>, so mu_C has the bits of
//   bi_sourcewise_expected_coarse's total.  The number of axes d does not enter the per-bin work: the chain rule to d mu_C / d z
//   is the host's, per cell.
//   The TY sums of every slot go through LDS in ty order.  With up to 33 slots one buffer would be 67 KB; the slots are reduced
//   in passes of kJacPass = 16 over one [16][256] buffer (32 KB, k_morph_coarse_jac<16>'s footprint) with a barrier between
//   passes.  TY == 1 needs no LDS.
//   Only the K = 1 + S + sum_s e_s live slots are written: slot q goes to group x.group[q] (>= 0) of an R = K call,
//   partial[item][K][coarse row][share][x], so k_coarse_finish, k_coarse_finish_wide and coarse_chunk serve unchanged; a padding
//   slot (s >= S or j >= e_s: group -1) is never written.  The map is uniform per launch and lies in the kernel arguments.
// No floating-point atomic anywhere and no per-bin derivative is ever written; a repeated identical call is bitwise identical,
// and a point's cells do not depend on the batch it came in.  Every index into the sums is a compile-time constant (the loops
// over slots are fully unrolled), so all nine classes -- <8, 3> with its 33 sums included -- run without scratch and in one
// launch: profiles/sourcewise_coarse_jacobian_kernel_resources.txt.
#pragma once

#include "bi_k_sourcewise.h"

namespace {

constexpr int kJacPass = 16;        // slots per pass through LDS

template <int SC, int EM>
__global__ __launch_bounds__(kThreads) void k_sourcewise_coarse_jac(SourcewiseCoarseJacArgs x) {
    const FactoredArgs& a = x.f;
    const CoarseArgs& g = x.g;
    constexpr int NC = 1 << EM, W = 1 + EM, NSL = 1 + SC * W;
    static_assert(SC <= 8 && NSL <= kCoarseJacSlots, "FactoredArgs::e holds 8 sources; SourcewiseCoarseJacArgs::group holds 33 slots");
    const int TX = 1 << g.tx_shift, TY = kThreads >> g.tx_shift;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.tx_shift;      // (TX >= 64: ty is wave-uniform)
    unsigned bx = blockIdx.x;
    const int xt = (int)(bx % (unsigned)g.n_xt);
    bx /= (unsigned)g.n_xt;
    const int split = (int)(bx % (unsigned)g.nsplit);
    const int64_t crow = bx / (unsigned)g.nsplit;
    const int64_t item = blockIdx.z;
    const int64_t* __restrict__ rowoff = a.rowoff + item * a.NR;
    const double* __restrict__ coef = a.coef + item * a.NR * W;
    const double* __restrict__ rate = a.rates + item * SC;
    const int64_t xr = (int64_t)xt * TX + tx;
    const bool live = xr < g.Lx;
    const int64_t lo = g.row_off[crow], n = g.row_off[crow + 1] - lo;
    const int64_t per = (n + g.nsplit - 1) / g.nsplit;
    const int64_t i0 = (int64_t)split * per, i1 = i0 + per < n ? i0 + per : n;

    double sum[NSL];
#pragma unroll
    for (int q = 0; q < NSL; ++q) sum[q] = 0.0;
    if (live)
        for (int64_t i = i0 + ty; i < i1; i += TY) {
            const int64_t bin = (int64_t)g.row_list[lo + i] * g.L + g.x_lo + xr;
            double mu = 0.0;
            int k = 0;                  // the source's first row: uniform
#pragma unroll
            for (int s = 0; s < SC; ++s) {
                double tau = 0.0, ups[EM];
#pragma unroll
                for (int j = 0; j < EM; ++j) ups[j] = 0.0;
                const int nc = a.e[s] < 0 ? 0 : 1 << a.e[s];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c < nc) {
                        const double p = a.ps[rowoff[k + c] + bin];
                        const double* q = coef + (int64_t)(k + c) * W;
                        tau = fma(q[0], p, tau);
#pragma unroll
                        for (int j = 0; j < EM; ++j) ups[j] = fma(q[1 + j], p, ups[j]);
                    }
                }
                k += nc;
                mu = fma(rate[s], tau, mu);
                sum[1 + s] += tau;
#pragma unroll
                for (int j = 0; j < EM; ++j) sum[1 + SC + s * EM + j] += ups[j];
            }
            sum[0] += mu;
        }

    const int64_t column = g.CR * g.nsplit * g.Lx;                              // from one group's partials to the next one's
    double* __restrict__ out = g.partial + (item * g.R * column + (crow * g.nsplit + split) * g.Lx + xr);
    if (TY == 1) {
        if (live) {
#pragma unroll
            for (int q = 0; q < NSL; ++q)
                if (x.group[q] >= 0) out[x.group[q] * column] = sum[q];
        }
        return;
    }
    constexpr int NB = NSL < kJacPass ? NSL : kJacPass;
    __shared__ double s_acc[NB][kThreads];
#pragma unroll
    for (int q0 = 0; q0 < NSL; q0 += NB) {
        if (q0 > 0) __syncthreads();            // (the pass before has read the buffer)
#pragma unroll
        for (int q = q0; q < q0 + NB && q < NSL; ++q) s_acc[q - q0][threadIdx.x] = sum[q];
        __syncthreads();
        if (ty == 0 && live) {
#pragma unroll
            for (int q = q0; q < q0 + NB && q < NSL; ++q) {
                if (x.group[q] >= 0) {
                    double t = s_acc[q - q0][tx];
                    for (int j = 1; j < TY; ++j) t += s_acc[q - q0][j * TX + tx];
                    out[x.group[q] * column] = t;
                }
            }
        }
    }
}

}  // namespace
