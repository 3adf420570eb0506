// bi_k_gof.h -- goodness of fit on the device.  Translation unit tu_gof.hip.
//
// k_morph_gof<NT>: the half-deviance and Pearson's chi2 of ONE (point, dataset) per work item in one pass over the corner
// rows of the point's cell: tile walk and block reduction of bi_k_item.h around a row loop of its own, one coefficient
// column, a_k = w_corner r_source, and two sums.  Per bin, mu = sum_k a_k row_k[b]:
//     slot 0 (half-deviance)   n > 0: (mu - n) - n log(mu / n)      n = 0: mu
//     slot 1 (Pearson)         n > 0: (n - mu)^2 / mu               n = 0: mu
// Both forms are free of cancellation between large numbers: the deviance is NOT formed as a difference of two
// log-likelihoods of size ~N (that costs log10(N / D) digits).  n = 0 and mu = 0 gives 0 in both, no 0 / 0; n > 0 and
// mu = 0 gives +inf in both.  Where poisson_term (bi_dev_common.h) gives nan (mu negative or nan, n nan) both terms are nan,
// where it gives -inf (n negative or not an integer) both are +inf.  Rows and counts are either the dense [Bp] ones (NT: the
// nontemporal loads of rows read once) or the compacted non-empty bins of the item's dataset; the empty bins of that form
// enter through the slot constants (bi_gof.h).  Two bins per thread, one 16-byte load per row and lane.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 62 VGPRs and 86 SGPRs in both instantiations, no scratch,
// 4160 bytes of LDS (the logarithm's table and the block reduction), 8 waves per SIMD.
//
// k_morph_expect: the expectation itself, out[item][r][b] = sum over the rows of group r of a_k row_k[b] (item_chain,
// bi_k_item.h) from the dense template tensor: one group (every row: mu_b) or one group per source (mu_{s,b}).  14 VGPRs, no
// scratch, no LDS.
#pragma once

#include "bi_k_item.h"
#include "bi_k_gof_terms.h"      // gof_terms: the per-bin forms, shared with k_sourcewise_gof (bi_k_sourcewise.h)

namespace {

template <bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_gof(HessArgs a) {
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NS;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NS;
    const double* __restrict__ cnt = a.counts + a.item_cnt[item];
    const int n_tiles = a.item_tiles[item];
    log_table_load();

    double sum[2] = {0.0, 0.0};      // half-deviance, Pearson
    for (ItemTiles w(a, n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
        const int64_t bin0 = (int64_t)tile * kTile + threadIdx.x * kBinsPerThread;
        const double2 n = stream_load<NT>(cnt + bin0);
        double mu0 = 0.0, mu1 = 0.0;
#pragma unroll 8
        for (int k = 0; k < a.NS; ++k) {
            const double2 v = stream_load<NT>(a.ps + rowoff[k] + bin0);
            const double c = coef[k];
            mu0 = fma(c, v.x, mu0);
            mu1 = fma(c, v.y, mu1);
        }
        gof_terms(n.x, mu0, sum[0], sum[1]);
        gof_terms(n.y, mu1, sum[0], sum[1]);
    }

    item_reduce_store(sum, item, a.partial, a.pflags);
}

__global__ __launch_bounds__(kThreads) void k_morph_expect(ExpectArgs a) {
    const int64_t bin = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (bin >= a.B) return;
    const int r = blockIdx.y;
    const int64_t item = blockIdx.z;
    const int64_t* __restrict__ rowoff = a.rowoff + item * a.NS;
    const double* __restrict__ coef = a.coef + item * a.NS;
    a.out[(item * a.R + r) * a.B + bin] = item_chain<4>(coef, rowoff, a.ps, bin, a.R > 1 ? r : 0, a.NS, a.R > 1 ? a.S : 1);
}

}  // namespace
