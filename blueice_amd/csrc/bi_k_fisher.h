// bi_k_fisher.h -- the expected-information kernel k_morph_fisher<G, DM, NT>: the Fisher information of ONE point per work
// item in one pass over its corner rows, no data read.  Translation unit tu_fisher.hip.
//
// Coefficient columns (host-built, bi_fisher.h; PointDerivs::first_order, the columns of k_morph_real and the first-order
// columns of k_morph_hess): column 0 gives mu_b, columns 1 .. D the first derivatives d_q mu_b (effective shape axes, then
// rate scales).  Per bin, with inv = 1 / mu_b:
//     sum[0]     += mu_b                                        the total expectation
//     sum[1 + q] += 1 where mu_b == 0 and d_q mu_b != 0         bins in which the information on q is unbounded, q < D
//     gram[qr]   += (inv d_q mu_b) d_r mu_b                     q >= r, both < D, only where mu_b > 0
// A bin with mu_b == 0 takes inv = 0: with every slope 0 (padding, bins no template fills) it adds 0.0 to every sum and no
// 0 * inf is formed; with a non-zero slope it is left out of the Gram sums and counted.  The counts are whole numbers in a
// double, exact far beyond any number of bins, and reduced like every other slot.  A negative or nan mu_b makes sum[0] nan:
// the host half reports the point's whole matrix as nan then.  The result slots of an item are k_morph_hess's,
// [G columns][DM (DM + 1) / 2 Gram pairs].  Tile walk, column sums and block reduction: bi_k_item.h; dense rows only.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): profiles/fisher_kernel_resources.txt; no scratch in any
// variant.
#pragma once

#include "bi_k_item.h"

namespace {

template <int DM>
constexpr int fisher_pairs() { return DM * (DM + 1) / 2; }

template <int G, int DM, bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_fisher(HessArgs a) {
    constexpr int NP = fisher_pairs<DM>();
    static_assert(DM <= G, "the first-order columns are a part of the G columns");
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NS;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NS * G;
    const int n_tiles = a.item_tiles[item];
    const int D = a.D;

    double sum[G], gram[NP];
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) gram[q] = 0.0;

    for (ItemTiles w(a, n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int half = 0; half < kBinsPerThread; ++half) {
            const int64_t bin = (int64_t)tile * kTile + half * kThreads + threadIdx.x;
            double acc[G];
            item_columns<G, NT>(a, rowoff, coef, bin, acc);
            const double mu = acc[0];
            sum[0] += mu >= 0.0 ? mu : __builtin_nan("");
            const bool empty = mu == 0.0;
            const double inv = mu > 0.0 ? 1.0 / mu : 0.0;
#pragma unroll
            for (int q = 0; q < DM; ++q)
                if (q + 1 < G) sum[1 + q] += (empty && acc[1 + q] != 0.0) ? 1.0 : 0.0;
#pragma unroll
            for (int q = 0; q < DM; ++q) {
                if (q + 1 < G && q < D) {
                    const double t = inv * acc[1 + q];
#pragma unroll
                    for (int r = 0; r <= q; ++r) gram[q * (q + 1) / 2 + r] = fma(t, acc[1 + r], gram[q * (q + 1) / 2 + r]);
                }
            }
        }
    }

    item_reduce_store(sum, gram, item, a.partial, a.pflags);
}

}  // namespace
