// bi_k_coarse.h -- coarse views on the device: the morphed expectation, and the data, summed over tensor-product groups of
// fine bins (bi_set_coarse_binning, bi_expected_coarse, bi_coarse_counts; host half bi_coarse.h).  Translation unit
// tu_coarse.hip.
//
// A fine bin is b = r L + x: x its index on the LAST analysis axis (L fine bins), r its row over the leading axes.  The host
// lists, once per binning, the fine rows of every coarse row (CSR, left-out rows absent) and the boundaries of the column
// groups.  No bin tensor is written in between: mu_b exists in a register only.
//
// k_morph_coarse: one block per (item, group of rows r, coarse row, share, x-tile).  Lanes lie along x, so every load of a
//   template row is a run of consecutive doubles -- whatever the coarsening, "first axis summed, last axis kept fine" included
//   -- read with 8-byte loads (r L is not 16-byte aligned in general).  The 256 threads are TY = 256 / TX sub-rows of
//   TX = 64, 128 or 256 lanes (the smallest that covers the Lx live columns, or 256 with several x-tiles): sub-row ty walks
//   the fine rows lo + ty, lo + ty + TY, ... of the block's share in list order, forms
//       mu_b = sum_k a_k row_k[r L + x]       (item_chain, bi_k_item.h: k_morph_expect's bits)
//   and adds it to its lane's sum; the TY sums of a column are then added in ty order through LDS, and the block writes
//   partial[item][r][coarse row][share][x].  A share without rows writes zeros.
// k_morph_coarse_jac<G>: the first derivatives of the same cells, J_C = d mu_C / d theta (bi_expected_coarse_jacobian).  The
//   blocks, the lanes and the order of every sum are k_morph_coarse's; a block handles all G = 4, 8 or 16 columns, so a
//   point's corner rows are read once for all of them.  Per fine bin the G = 1 + D padded coefficient columns of
//   PointDerivs::first_order (bi_items.h; D = d_eff + S) are formed as item_columns forms them (bi_k_item.h):
//       col_g = sum_k coef[k][g] row_k[r L + x]      0 -> mu_b, 1 .. d_eff -> d mu_b / d z, then d mu_b / d rate_scale_s
//   and added to G per-lane sums in registers; the TY sums of every column go through LDS in ty order, and column g is written
//   as group g of an R = G call, partial[item][g][coarse row][share][x]: the finish kernels below are unchanged.  Column 0 is
//   k_morph_coarse's chain and order, so mu_C has the bits of bi_expected_coarse's total.  No per-bin derivative is written.
// k_coarse_finish: one thread per output cell: the shares in order, inside a share the columns of the cell's group in order.
// k_coarse_finish_wide: one block per output cell, for binnings whose cells gather many partials (everything summed: 10^5).
// There is no floating-point atomic anywhere: every sum runs in a fixed order and a repeated identical call is bitwise
// identical.  The order depends on the launch parameters TX (hence TY), nsplit and wide, which the host derives from the binning
// and the device's CU count alone (bi_coarse.h: coarse_geometry) -- not from the number of points of the call, so a point's
// result does not depend on the batch it came in.
// Dense counts go through the same two kernels with NS = 1, a_0 = 1 and the counts row as the "template" (1.0 n + 0.0 = n
// exactly; sums of integer counts below 2^53 are exact in any order, real-valued ones are summed in the order above).
//
// k_coarse_list: datasets that exist as non-empty-bin lists only (device-generated toys): one thread per list entry adds its
//   count to a zeroed 64-bit INTEGER table with an integer atomic -- generated counts are integers by construction, so the
//   order of addition cannot change the result; k_coarse_table turns the table into doubles.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), no scratch in any of them:
//     k_morph_coarse    34 VGPRs, 86 SGPRs, 2048 bytes of LDS (the TY sums of every column), 8 waves per SIMD
//     k_morph_coarse_jac<4>    38 VGPRs,  96 SGPRs,  8192 bytes of LDS (G x 256 doubles), 8 waves per SIMD
//     k_morph_coarse_jac<8>    60 VGPRs, 104 SGPRs, 16384 bytes of LDS, 7 waves per SIMD
//     k_morph_coarse_jac<16>   87 VGPRs, 106 SGPRs, 32768 bytes of LDS, 5 waves per SIMD (profiles/coarse_jacobian_kernel_resources.txt)
//     k_coarse_finish   16 VGPRs, 25 SGPRs, no LDS
//     k_coarse_finish_wide   20 VGPRs, 44 SGPRs, 32 bytes of LDS (the four waves' sums)
//     k_coarse_list     21 VGPRs, 43 SGPRs, no LDS
//     k_coarse_table     6 VGPRs, 12 SGPRs, no LDS
#pragma once

#include "bi_k_item.h"

namespace {

__global__ __launch_bounds__(kThreads) void k_morph_coarse(CoarseArgs a) {
    const int TX = 1 << a.tx_shift, TY = kThreads >> a.tx_shift;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> a.tx_shift;      // (TX >= 64: ty is wave-uniform)
    unsigned bx = blockIdx.x;
    const int xt = (int)(bx % (unsigned)a.n_xt);
    bx /= (unsigned)a.n_xt;
    const int split = (int)(bx % (unsigned)a.nsplit);
    const int64_t crow = bx / (unsigned)a.nsplit;
    const int r = blockIdx.y;
    const int64_t item = blockIdx.z;
    const int64_t* __restrict__ rowoff = a.rowoff + item * a.NS;
    const double* __restrict__ coef = a.coef + item * a.NS;
    const int step = a.R > 1 ? a.S : 1, k0 = a.R > 1 ? r : 0;
    const int64_t xr = (int64_t)xt * TX + tx;
    const bool live = xr < a.Lx;
    const int64_t lo = a.row_off[crow], n = a.row_off[crow + 1] - lo;
    const int64_t per = (n + a.nsplit - 1) / a.nsplit;
    const int64_t i0 = (int64_t)split * per, i1 = i0 + per < n ? i0 + per : n;

    double acc = 0.0;
    if (live)
        for (int64_t i = i0 + ty; i < i1; i += TY) {
            acc += item_chain<8>(coef, rowoff, a.ps, (int64_t)a.row_list[lo + i] * a.L + a.x_lo + xr, k0, a.NS, step);
        }

    double* __restrict__ out = a.partial + ((((item * a.R + r) * a.CR + crow) * a.nsplit + split) * a.Lx + xr);
    if (TY == 1) {
        if (live) *out = acc;
        return;
    }
    __shared__ double s_acc[kThreads];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (ty == 0 && live) {
        double s = s_acc[tx];
        for (int j = 1; j < TY; ++j) s += s_acc[j * TX + tx];
        *out = s;
    }
}

// The same blocks with G coefficient columns per corner row instead of one: a.coef [items][NS][G] (see the header comment).
// Column g of a block goes to partial[item][g][coarse row][share][x]: group g of an R = G call, for the finish kernels.
template <int G>
__global__ __launch_bounds__(kThreads) void k_morph_coarse_jac(CoarseArgs a) {
    const int TX = 1 << a.tx_shift, TY = kThreads >> a.tx_shift;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> a.tx_shift;
    unsigned bx = blockIdx.x;
    const int xt = (int)(bx % (unsigned)a.n_xt);
    bx /= (unsigned)a.n_xt;
    const int split = (int)(bx % (unsigned)a.nsplit);
    const int64_t crow = bx / (unsigned)a.nsplit;
    const int64_t item = blockIdx.z;
    const int64_t* __restrict__ rowoff = a.rowoff + item * a.NS;
    const double* __restrict__ coef = a.coef + item * a.NS * G;
    const int64_t xr = (int64_t)xt * TX + tx;
    const bool live = xr < a.Lx;
    const int64_t lo = a.row_off[crow], n = a.row_off[crow + 1] - lo;
    const int64_t per = (n + a.nsplit - 1) / a.nsplit;
    const int64_t i0 = (int64_t)split * per, i1 = i0 + per < n ? i0 + per : n;

    double sum[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = 0.0;
    if (live)
        for (int64_t i = i0 + ty; i < i1; i += TY) {
            double acc[G];
            item_columns<G, false>(a, rowoff, coef, (int64_t)a.row_list[lo + i] * a.L + a.x_lo + xr, acc);
#pragma unroll
            for (int g = 0; g < G; ++g) sum[g] += acc[g];
        }

    const int64_t column = a.CR * a.nsplit * a.Lx;                              // from one column's partials to the next one's
    double* __restrict__ out = a.partial + (item * G * column + (crow * a.nsplit + split) * a.Lx + xr);
    if (TY == 1) {
        if (live) {
#pragma unroll
            for (int g = 0; g < G; ++g) out[g * column] = sum[g];
        }
        return;
    }
    __shared__ double s_acc[G][kThreads];
#pragma unroll
    for (int g = 0; g < G; ++g) s_acc[g][threadIdx.x] = sum[g];
    __syncthreads();
    if (ty == 0 && live) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            double s = s_acc[g][tx];
            for (int j = 1; j < TY; ++j) s += s_acc[g][j * TX + tx];
            out[g * column] = s;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_coarse_finish(CoarseArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= a.n_out) return;
    const int64_t cx = idx % a.Cx, q = idx / a.Cx;                   // q = (item R + r) CR + coarse row
    const int64_t x0 = a.xb[cx] - a.x_lo, x1 = a.xb[cx + 1] - a.x_lo;
    const double* __restrict__ p = a.partial + q * a.nsplit * a.Lx;
    double s = 0.0;
    for (int sp = 0; sp < a.nsplit; ++sp, p += a.Lx)
        for (int64_t x = x0; x < x1; ++x) s += p[x];
    a.out[idx] = s;
}

// the same sum for cells of many partials (a.wide: shares x widest column group >= kCoarseWide, bi_coarse.h): one block per
// cell.  The cell's partials, numbered j = share * width + column, are dealt to the threads j = t, t + 256, ... (consecutive
// lanes read consecutive columns), every thread adds its own in ascending j, then the wave's shuffle tree and the four waves
// in order.  Which of the two finish kernels runs is a property of the binning, like TX and nsplit.
__global__ __launch_bounds__(kThreads) void k_coarse_finish_wide(CoarseArgs a) {
    const int64_t idx = blockIdx.x;
    const int64_t cx = idx % a.Cx, q = idx / a.Cx;
    const int64_t x0 = a.xb[cx] - a.x_lo, w = a.xb[cx + 1] - a.xb[cx];
    const double* __restrict__ p = a.partial + q * a.nsplit * a.Lx + x0;
    const int64_t n = (int64_t)a.nsplit * w;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += kThreads) s += p[(j / w) * a.Lx + j % w];
    __shared__ double s_sum[kThreads / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
#pragma unroll
        for (int v = 1; v < kThreads / 64; ++v) t += s_sum[v];
        a.out[idx] = t;
    }
}

__global__ __launch_bounds__(kThreads) void k_coarse_list(CoarseListArgs a) {
    const int64_t i = blockIdx.y, t = a.dataset[i];
    const int64_t lo = a.nz_off[t], hi = a.nz_off[t + 1];
    for (int64_t e = lo + (int64_t)blockIdx.x * kThreads + threadIdx.x; e < hi; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = a.nz_idx[e];
        const int32_t cr = a.row_map[b / a.L], cx = a.x_map[b % a.L];
        if (cr >= 0 && cx >= 0) atomicAdd(a.table + (i * a.C + (int64_t)cr * a.Cx + cx), (unsigned long long)a.nz_n[e]);
    }
}

__global__ __launch_bounds__(kThreads) void k_coarse_table(const unsigned long long* __restrict__ table, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = (double)table[i];
}

}  // namespace
