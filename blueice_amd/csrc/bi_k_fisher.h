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
// [G columns][DM (DM + 1) / 2 Gram pairs], its block reduction and the order of its partials too; k_finish reduces them.
// One bin in flight per thread, the tile's 512 bins in two passes of 256, dense rows only.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): profiles/fisher_kernel_resources.txt; no scratch in any
// variant.
#pragma once

namespace {

template <int DM>
constexpr int fisher_pairs() { return DM * (DM + 1) / 2; }

template <int G, int DM, bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_fisher(HessArgs a) {
    constexpr int NP = fisher_pairs<DM>();
    constexpr int NSL = G + NP;
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

    const int chunks = (a.chunks > 1 && n_tiles >= 64 * a.chunks) ? a.chunks : 1;
    const int per_chunk = (n_tiles + chunks - 1) / chunks;
    for (int lt = blockIdx.x; lt < per_chunk * chunks; lt += gridDim.x) {
        const int tile = chunks > 1 ? (lt % chunks) * per_chunk + lt / chunks : lt;
        if (tile >= n_tiles) continue;
        // the tile's 512 bins in two passes of 256 consecutive bins, every row element read once
#pragma unroll 1
        for (int half = 0; half < kBinsPerThread; ++half) {
            const int64_t bin = (int64_t)tile * kTile + half * kThreads + threadIdx.x;
            double acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.0;
#pragma unroll 4
            for (int k = 0; k < a.NS; ++k) {
                const double* p = a.ps + rowoff[k] + bin;
                const double v = NT ? __builtin_nontemporal_load(p) : *p;
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = fma(coef[k * G + g], v, acc[g]);
            }
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

    // block reduction: wave sums, then the four waves in order
    __shared__ double s_sum[kThreads / 64][NSL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double s = wave_sum(sum[g]);
        if (lane == 0) s_sum[wave][g] = s;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const double s = wave_sum(gram[q]);
        if (lane == 0) s_sum[wave][G + q] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < NSL; j += kThreads) {
        double s = s_sum[0][j];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) s += s_sum[w][j];
        const int64_t o = ((int64_t)item * gridDim.x + blockIdx.x) * NSL + j;
        a.partial[o] = s;
        a.pflags[o] = 0u;
    }
}

}  // namespace
