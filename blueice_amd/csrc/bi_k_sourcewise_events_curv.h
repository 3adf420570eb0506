// bi_k_sourcewise_events_curv.h -- k_sourcewise_events_curv<SC, EM, PS, PANEL>: the sums from which the host half
// (bi_eval_sourcewise_events_hess, bi_sourcewise_events.h) forms the Hessian of ONE point of a source-wise model over the EVENTS of
// its event set.  Translation unit tu_sourcewise_events_curv.hip.
//
// k_factored_curv's observed form (bi_k_factored_curv.h) inside k_sourcewise_events' walk (bi_k_sourcewise_events.h): the event
// likelihood is the binned observed form with n = 1 per event, no lgamma and N_s = 1.  Per event e, the basis columns by
// k_factored_curv's fma chains from the coef columns w, d_j w, d_j d_k w (WC = 1 + EM + NX per row):
//     tau_s, ups_s,j, chi_s,x                       one fma per corner, from 0.0;  x = k (k - 1) / 2 + j for j < k < EM
//     lam = sum_s r_s tau_s                         one fma per source, from 0.0; a source whose tau_s is nan leaves the event: its
//                                                   tau, ups and chi count as +0.0 there (k_sourcewise_events does the same)
//     clamped = outlier != 0 and not (lam > 0):     lam := outlier, g := 0;   otherwise g = 1 / lam
// and over the live events of the item's set (a column behind the set's N_t is masked BY INDEX, item_n)
//     [0]                           sum_e log lam          } bit for bit the slots of k_sourcewise_events<SC, EM, true>: the same
//     [1 + s], [1 + SC + s EM + j]  sum_e g tau_s, g ups   } chains, events per thread in the same order, blocks per item
//     [1 + K + s NX + x]            sum_e g chi_s,x        NX = EM (EM - 1) / 2
//     Q_ab = sum_e ((g u_a) g) u_b                         a >= b over u = (tau_s, ups_s,j), K = SC (1 + EM); no g^2 is formed
// The Gram is split into k_factored_curv's panels of PS whole sources (factored_curv_panels, factored_curv_panel_sources): panel
// PANEL accumulates the rows of its sources against all columns b <= a, recomputing every basis column (lam needs them all); the
// linear slots are panel 0's, the other panels post their pairs alone.  At most 136 pair accumulators per thread, every register
// index a compile-time constant.  One event in flight per thread; the thread's events are 2 t, 2 t + 1 of a tile where
// factored_vec<SC, EM>() == 2 and t, t + 256 otherwise, which is what fixes the bits of the shared slots.
// The tile walk is ListTiles: min(tiles of the item's set, max_blocks) blocks, a block beyond the item's own count posts +0.0 with
// a clear flag.  Plain loads, no floating-point atomics; the block reduction is item_reduce_store.
// Registers of every instantiation: profiles/sourcewise_events_curv_kernel_resources.txt.
#pragma once

#include "bi_k_factored_curv.h"

namespace {

template <int SC, int EM, int PS, int PANEL>
__global__ __launch_bounds__(kThreads) void k_sourcewise_events_curv(SourcewiseEventsArgs a) {
    constexpr int NC = 1 << EM, W = 1 + EM, NX = EM * (EM - 1) / 2, WC = W + NX, V = factored_vec<SC, EM>();
    constexpr int K = SC * W, A0 = curv_row0(EM, PS, PANEL), A1 = curv_row0(EM, PS, PANEL + 1), NP = curv_pairs(EM, PS, PANEL);
    constexpr bool LIN = PANEL == 0;
    constexpr int NL = LIN ? factored_curv_linear(SC, EM, false) : 1, NXA = (LIN && NX > 0) ? NX : 1;
    constexpr int NSL = (LIN ? NL : 0) + NP;
    static_assert(SC <= 8 && SC % PS == 0 && A1 <= K && kBinsPerThread == 2, "panels of whole sources; a tile is two events per thread");
    static_assert(NP <= 136, "at most 136 pair accumulators per thread");
    static_assert(NSL <= kThreads, "one thread per result slot");
    const int item = blockIdx.y;
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
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * WC;
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const int64_t n_events = a.item_n[item];
    const double outlier = a.outlier;
    log_table_load();

    double sum[NL], gram[NP];
#pragma unroll
    for (int g = 0; g < NL; ++g) sum[g] = 0.0;
#pragma unroll
    for (int g = 0; g < NP; ++g) gram[g] = 0.0;

    for (ListTiles w(a, n_tiles, nbx); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int part = 0; part < kBinsPerThread; ++part) {
            const int64_t ev = (int64_t)tile * kTile + (V == 2 ? 2 * (int)threadIdx.x + part : part * kThreads + (int)threadIdx.x);
            double u[K], chi[SC][NXA], lam = 0.0;
            int k = 0;                  // the source's first row: uniform
#pragma unroll
            for (int s = 0; s < SC; ++s) {
#pragma unroll
                for (int j = 0; j < W; ++j) u[s * W + j] = 0.0;
#pragma unroll
                for (int x = 0; x < NXA; ++x) chi[s][x] = 0.0;
                const int nc = a.e[s] < 0 ? 0 : 1 << a.e[s];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c < nc) {
                        const double p = a.ps[rowoff[k + c] + ev];
                        const double* q = coef + (int64_t)(k + c) * WC;
#pragma unroll
                        for (int j = 0; j < W; ++j) u[s * W + j] = fma(q[j], p, u[s * W + j]);
                        if constexpr (LIN && NX > 0) {
#pragma unroll
                            for (int x = 0; x < NX; ++x) chi[s][x] = fma(q[W + x], p, chi[s][x]);
                        }
                    }
                }
                k += nc;
                const double r = rate[s];
                if (u[s * W] != u[s * W]) {         // a nan corner: the source leaves this event (nansum)
#pragma unroll
                    for (int j = 0; j < W; ++j) u[s * W + j] = 0.0;
#pragma unroll
                    for (int x = 0; x < NXA; ++x) chi[s][x] = 0.0;
                } else {
                    lam = fma(r, u[s * W], lam);
                }
            }
            double l = lam;
            const bool clamped = outlier != 0.0 && !(l > 0.0);
            if (clamped) l = outlier;
            const double lg = bin_log(l);
            if (ev < n_events) {                    // (by index: a padded column holds zeros and would take the clamp)
                const double g = clamped ? 0.0 : 1.0 / l;
                if constexpr (LIN) {
                    sum[0] += lg;
#pragma unroll
                    for (int s = 0; s < SC; ++s) {
                        sum[1 + s] = fma(g, u[s * W], sum[1 + s]);
#pragma unroll
                        for (int j = 0; j < EM; ++j) sum[1 + SC + s * EM + j] = fma(g, u[s * W + 1 + j], sum[1 + SC + s * EM + j]);
#pragma unroll
                        for (int x = 0; x < NX; ++x) sum[1 + K + s * NX + x] = fma(g, chi[s][x], sum[1 + K + s * NX + x]);
                    }
                }
#pragma unroll
                for (int r = A0; r < A1; ++r) {
                    const double t = (g * u[r]) * g;
#pragma unroll
                    for (int b = 0; b <= r; ++b) gram[curv_tri(r) - curv_tri(A0) + b] = fma(t, u[b], gram[curv_tri(r) - curv_tri(A0) + b]);
                }
            }
        }
    }

    if constexpr (LIN) item_reduce_store(sum, gram, item, a.partial, a.pflags);
    else item_reduce_store(gram, item, a.partial, a.pflags);
}

}  // namespace
