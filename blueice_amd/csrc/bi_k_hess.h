// bi_k_hess.h -- the Hessian kernel k_morph_hess<G, DM, UNB, NT>: value, gradient and second derivatives of ONE point per
// work item in one pass over its corner rows.  Translation unit tu_hess.hip.
//
// Coefficient columns (host-built, bi_hess.h): column 0 gives mu_b, columns 1 .. D the first derivatives d_q mu_b
// (effective shape axes, then rate scales), the next ones the non-zero second derivatives d_qr mu_b (the morph is
// multilinear inside a cell, so each is another fixed combination of the same rows).  Per bin, with f = n / mu - 1,
// inv = 1 / mu, wn = n (binned; zero-count bins: f = -1, wn = 0) or f = inv = 1 / lambda, wn = 1 (unbinned events; an event
// on the outlier clamp: f = inv = 0):
//     sum[0]   += the log-likelihood term
//     sum[g]   += f * acc[g]                                    every derivative column (first and second order)
//     gram[qr] -= wn * (inv * acc[1 + q]) * (inv * acc[1 + r])   q >= r, both < D
// The result slots of an item are [G columns][DM (DM + 1) / 2 Gram pairs].  Tile walk, column sums and block reduction:
// bi_k_item.h; what is written here is the per-bin mathematics.
#pragma once

#include "bi_k_item.h"

namespace {

template <int DM>
constexpr int hess_pairs() { return DM * (DM + 1) / 2; }

template <int G, int DM, bool UNB, bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_hess(HessArgs a) {
    constexpr int NP = hess_pairs<DM>();
    static_assert(DM <= G, "the first-order columns are a part of the G columns");
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NS;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NS * G;
    const double* __restrict__ cnt = UNB ? nullptr : a.counts + a.item_cnt[item];
    const int n_tiles = a.item_tiles[item];
    const int D = a.D;
    log_table_load();

    double sum[G], gram[NP];
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) gram[q] = 0.0;

    for (ItemTiles w(a, n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
        // one bin in flight per thread (the G columns and the Gram sums already hold ~2 G + DM^2 / 2 doubles)
#pragma unroll 1
        for (int half = 0; half < kBinsPerThread; ++half) {
            const int64_t bin = (int64_t)tile * kTile + half * kThreads + threadIdx.x;
            double n = 0.0;
            if constexpr (!UNB) n = NT ? __builtin_nontemporal_load(cnt + bin) : cnt[bin];
            double acc[G];
            item_columns<G, NT>(a, rowoff, coef, bin, acc);
            // f: the weight of every derivative column; inv, wn: the Gram term is -wn (inv d_q mu)(inv d_r mu), with the first
            // derivatives scaled by inv before the product (1 / lambda^2 alone overflows for densities below 1e-154)
            double f, inv, wn;
            if constexpr (UNB) {
                if (bin >= a.B) continue;
                double lam = acc[0];
                const bool clamped = a.outlier != 0.0 && !(lam > 0.0);
                if (clamped) lam = a.outlier;
                sum[0] += bin_log(lam);
                f = inv = clamped ? 0.0 : 1.0 / lam;
                wn = 1.0;
            } else {
                const double mu = acc[0];
                sum[0] += poisson_term(n, mu);
                inv = n != 0.0 ? 1.0 / mu : 0.0;
                f = n * inv - 1.0;
                wn = n;
            }
#pragma unroll
            for (int g = 1; g < G; ++g) sum[g] = fma(f, acc[g], sum[g]);
#pragma unroll
            for (int q = 0; q < DM; ++q)
                if (q + 1 < G) acc[1 + q] *= inv;
#pragma unroll
            for (int q = 0; q < DM; ++q) {
                if (q + 1 < G && q < D) {
                    const double t = -wn * acc[1 + q];
#pragma unroll
                    for (int r = 0; r <= q; ++r) gram[q * (q + 1) / 2 + r] = fma(t, acc[1 + r], gram[q * (q + 1) / 2 + r]);
                }
            }
        }
    }

    item_reduce_store(sum, gram, item, a.partial, a.pflags);
}

}  // namespace
