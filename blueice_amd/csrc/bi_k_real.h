// bi_k_real.h -- real-valued counts on the device (Asimov data, weighted histograms).  Translation unit tu_real.hip.
//
// k_morph_real<G, NT>: the half-deviance of ONE (point, real-valued dataset) per work item and its first derivatives, in one
// pass over the corner rows of the point's cell -- k_morph_gof's cancellation-free sum (bi_k_gof.h) with k_morph_hess's
// coefficient columns (bi_k_hess.h): column 0 gives mu_b, columns 1 .. G - 1 the first derivatives d_q mu_b.  Per bin
//     slot 0      n > 0: (mu - n) - n log(mu / n)        n = 0: mu
//     slot q      n > 0: d_q mu (1 - n / mu)             n = 0: d_q mu
// n is any real number >= 0 (bi_set_real_counts / bi_set_asimov_counts admit nothing else): there is no integer test.
// n > 0 and mu = 0 gives +inf in slot 0, mu negative or nan gives nan; the derivative slots of such an item are whatever
// the arithmetic makes of them, and the host half (bi_real.h) reports nan for them.  mu_b is column 0 of item_columns, the
// fma chain of item_chain (bi_k_item.h) with a_k = w_corner r_source: at the truth of an Asimov dataset mu_b == n_b
// bit for bit, mu / n == 1.0, bin_log(1.0) == 0.0 and 1 - n / mu == 0.0, so slot 0 and every derivative slot are 0.0
// exactly.  Tile walk, column sums and block reduction: bi_k_item.h (2 G doubles of sums and columns); dense rows only.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), both NT instantiations alike:
//     G = 1 (value only)   38 VGPRs,  78 SGPRs, 4128 bytes of LDS
//     G = 4                50 VGPRs, 105 SGPRs, 4224 bytes
//     G = 8                67 VGPRs, 106 SGPRs, 4352 bytes
//     G = 16               99 VGPRs, 106 SGPRs, 4608 bytes
// no scratch in any of them (LDS: the logarithm's table and the block reduction's 4 x G sums).
//
// k_real_expect: the Asimov datasets themselves, out[item][Bp] = mu_b of truth `item`: k_morph_expect's host-built
// coefficients through the same item_chain, written with the store's row stride, and bad[item] = 1 + a bin whose expectation
// is negative or nan (any one of them; 0: none).
#pragma once

#include "bi_k_item.h"

namespace {

template <int G, bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_real(HessArgs a) {
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NS;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NS * G;
    const double* __restrict__ cnt = a.counts + a.item_cnt[item];
    const int n_tiles = a.item_tiles[item];
    log_table_load();

    double sum[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = 0.0;

    for (ItemTiles w(a, n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int half = 0; half < kBinsPerThread; ++half) {
            const int64_t bin = (int64_t)tile * kTile + half * kThreads + threadIdx.x;
            const double n = NT ? __builtin_nontemporal_load(cnt + bin) : cnt[bin];
            double acc[G];
            item_columns<G, NT>(a, rowoff, coef, bin, acc);
            const double mu = acc[0];
            double dev = mu, f = 1.0;
            if (n > 0.0) {
                dev = (mu - n) - n * bin_log(mu / n);      // mu = 0: +inf
                f = 1.0 - n / mu;
            }
            if (!(mu >= 0.0)) dev = __builtin_nan("");
            sum[0] += dev;
#pragma unroll
            for (int g = 1; g < G; ++g) sum[g] = fma(f, acc[g], sum[g]);
        }
    }

    item_reduce_store(sum, item, a.partial, a.pflags);
}

__global__ __launch_bounds__(kThreads) void k_real_expect(RealExpectArgs a) {
    const int64_t bin = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (bin >= a.B) return;
    const int64_t item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + item * a.NS;
    const double* __restrict__ coef = a.coef + item * a.NS;
    const double mu = item_chain<4>(coef, rowoff, a.ps, bin, 0, a.NS, 1);
    a.out[item * a.Bp + bin] = mu;
    if (!(mu >= 0.0)) a.bad[item] = bin + 1;       // (any of the offending bins: the lanes' stores of one word race harmlessly)
}

}  // namespace
