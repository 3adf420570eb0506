// bi_k_sourcewise_nonempty.h -- k_sourcewise_nonempty<SC, EM, GRAD>: the sums of ONE point of a source-wise model over the NON-EMPTY
// bins of its dataset, and k_sourcewise_gather, which makes the compacted copies it streams.  Translation unit
// tu_sourcewise_nonempty.hip; host half bi_sourcewise_nonempty.h.
//
// With templates >= 0 and rates in [0, inf) mu_b >= 0 in every bin, so the only per-bin terms of the Poisson log likelihood that
// are not linear in the templates are those of the bins with n_b != 0 (the list Z_t of dataset t, ascending bins):
//     ll = sum_{b in Z} n_b log mu_b  -  sum_s lambda_s  -  sum_b lgamma(n_b + 1),      lambda_s = r_s sum_c w_c R_{s,c}
// with R_{s,c} the total of anchor row (s, c) over all bins.  The kernel adds up the first sum; the second and third are one
// number per item, which k_finish subtracts (slot_lg).  Per listed bin, k_morph_factored's fma chains statement for statement:
//     tau_s   = sum_c w_c p_{s,c,b}                 one fma per corner, from 0.0
//     ups_s,j = sum_c d_j w_c p_{s,c,b}             (GRAD)
//     mu      = sum_s r_s tau_s                     one fma per source, from 0.0
//     g       = n (1 / mu)                          (n = 0: 0 -- the padding behind the list)
// and the result slots of an item
//     [0]                      sum_Z n log mu       (-inf where mu = 0 or n is no integer: poisson_term's rules)
//     [1 + s]                  sum_Z g tau_s        (GRAD)
//     [1 + SC + s EM + j]      sum_Z g ups_s,j      (GRAD)
// The host subtracts N_s = sum_c w_c R_{s,c} and d_j N_s from the gradient slots and applies FacBatch::gradient's chain rule.
//
// The rows are those of the item's dataset's compacted copy ([rows][np_t], zeros behind the list: a padded bin has n = 0 and
// every template 0, and contributes exactly +0.0 to every slot), so the number of tiles is PER ITEM (item_tiles).  An item's
// tiles are walked by min(tiles, max_blocks) blocks -- its list's length alone decides, not the launch: the grid is (the largest
// block count of the launch, items), a block beyond its item's own count posts +0.0 with a clear flag and is gone, and the
// others stride by the item's count, not by gridDim.x (ListTiles).  k_finish then adds the same partials in the same lanes
// whatever else was launched beside the item; +0.0 changes no bit of a sum that started from +0.0.
// Classes (SC, EM) and bins in flight per thread are k_morph_factored's (factored_vec), for both GRAD variants: a values-only
// call has the bits of the call with the gradient.  No nontemporal loads: the compacted rows are meant to be read again from
// cache.  No floating-point atomics.  Registers, LDS and scratch of every instantiation:
// profiles/sourcewise_nonempty_kernel_resources.txt (no scratch in any).
#pragma once

#include "bi_k_factored.h"

namespace {

// n log mu of a listed bin under poisson_term's rules: mu not >= 0 or n nan -> nan; n negative or no integer -> -inf; n = 0
// (padding) -> +0.0 whatever mu is; mu = 0 under n > 0 -> -inf
__device__ __forceinline__ double listed_term(double n, double mu) {
    double t = n > 0.0 ? n * bin_log(mu) : 0.0;
    if (!(mu >= 0.0) || n != n) t = __builtin_nan("");
    else if (n < 0.0 || n != floor(n)) t = -__builtin_inf();
    return t;
}

template <int SC, int EM, bool GRAD>
__global__ __launch_bounds__(kThreads) void k_sourcewise_nonempty(SourcewiseNonemptyArgs a) {
    constexpr int NC = 1 << EM, W = 1 + EM, V = factored_vec<SC, EM>();
    constexpr int NSL = GRAD ? 1 + SC * W : 1;
    static_assert(SC <= 8 && kBinsPerThread == 2, "SourcewiseNonemptyArgs::e holds 8 sources; a tile is two bins per thread");
    const int item = blockIdx.y;
    if constexpr (!GRAD) {
        // items planned on the device: a rejected point posts nothing (its perm is -1: k_finish skips it)
        if (a.live && !a.live[item]) return;
    }
    const int n_tiles = a.item_tiles[item];
    const int nbx = min(n_tiles, a.max_blocks);
    if ((int)blockIdx.x >= nbx) {           // not one of this item's blocks: +0.0 and a clear flag for k_finish
        if (threadIdx.x < NSL) {
            const int64_t o = ((int64_t)item * gridDim.x + blockIdx.x) * NSL + threadIdx.x;
            a.partial[o] = 0.0;
            a.pflags[o] = 0u;
        }
        return;
    }
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NR;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * W;
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const double* __restrict__ cnt = a.counts + a.item_cnt[item];
    log_table_load();

    double sum[NSL];
#pragma unroll
    for (int g = 0; g < NSL; ++g) sum[g] = 0.0;

    for (ListTiles w(a, n_tiles, nbx); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int part = 0; part < kBinsPerThread / V; ++part) {
            // V = 2: the thread's two neighbouring bins, one 16-byte load per row; V = 1: one bin of each half of the tile
            const int64_t bin = (int64_t)tile * kTile + (V == 2 ? 2 * (int)threadIdx.x : part * kThreads + (int)threadIdx.x);
            double n[V];
            if constexpr (V == 2) {
                const double2 t = stream_load<false>(cnt + bin);
                n[0] = t.x; n[1] = t.y;
            } else {
                n[0] = cnt[bin];
            }
            double tau[SC][V], ups[GRAD ? SC : 1][EM][V], mu[V];
#pragma unroll
            for (int v = 0; v < V; ++v) mu[v] = 0.0;
            int k = 0;                  // the source's first row: uniform
#pragma unroll
            for (int s = 0; s < SC; ++s) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    tau[s][v] = 0.0;
                    if constexpr (GRAD) {
#pragma unroll
                        for (int j = 0; j < EM; ++j) ups[s][j][v] = 0.0;
                    }
                }
                const int nc = a.e[s] < 0 ? 0 : 1 << a.e[s];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c < nc) {
                        const double* src = a.ps + rowoff[k + c] + bin;
                        const double* q = coef + (int64_t)(k + c) * W;
                        double p[V];
                        if constexpr (V == 2) {
                            const double2 t = stream_load<false>(src);
                            p[0] = t.x; p[1] = t.y;
                        } else {
                            p[0] = *src;
                        }
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            tau[s][v] = fma(q[0], p[v], tau[s][v]);
                            if constexpr (GRAD) {
#pragma unroll
                                for (int j = 0; j < EM; ++j) ups[s][j][v] = fma(q[1 + j], p[v], ups[s][j][v]);
                            }
                        }
                    }
                }
                k += nc;
                const double r = rate[s];
#pragma unroll
                for (int v = 0; v < V; ++v) mu[v] = fma(r, tau[s][v], mu[v]);
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                sum[0] += listed_term(n[v], mu[v]);
                if constexpr (GRAD) {
                    const double inv = n[v] != 0.0 ? 1.0 / mu[v] : 0.0;
                    const double g = n[v] * inv;
#pragma unroll
                    for (int s = 0; s < SC; ++s) {
                        sum[1 + s] = fma(g, tau[s][v], sum[1 + s]);
#pragma unroll
                        for (int j = 0; j < EM; ++j) sum[1 + SC + s * EM + j] = fma(g, ups[s][j][v], sum[1 + SC + s * EM + j]);
                    }
                }
            }
        }
    }

    item_reduce_store(sum, item, a.partial, a.pflags);
}

// The compacted copies: one thread per (compact bin j, row, dataset); row == rows is the dataset's counts.  Behind the list
// (j >= nnz) zeros.  gridDim.y may be smaller than rows + 1 (the rows are strided).
__global__ __launch_bounds__(kThreads) void k_sourcewise_gather(SourcewiseGatherArgs a) {
    const int64_t t = a.t0 + blockIdx.z;
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t np = a.ne_np[t];
    if (j >= np) return;
    const int64_t lo = a.nz_off[t], nnz = a.nz_off[t + 1] - lo;
    const bool listed = j < nnz;
    const int64_t bin = listed ? a.nz_idx[lo + j] : 0;
    for (int64_t row = blockIdx.y; row <= a.rows; row += gridDim.y) {
        if (row == a.rows) a.out_cnt[a.ne_cnt_off[t] + j] = listed ? a.nz_n[lo + j] : 0.0;
        else a.out_ps[a.ne_off[t] + row * np + j] = listed ? a.ps[row * a.Bp + bin] : 0.0;
    }
}

}  // namespace
