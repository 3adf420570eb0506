// bi_k_sourcewise_events.h -- k_sourcewise_events<SC, EM, GRAD>: the sums of ONE point of a source-wise model over the EVENTS of
// its event set: the extended unbinned likelihood with one anchor grid per source.  Translation unit tu_sourcewise_events.hip;
// host half bi_sourcewise_events.h.
//
// The event store holds, per anchor row of the model, the pdf value of every event ([rows][columns]; set t at the columns
// [first_t, first_t + N_t), padded to whole tiles).  Per event e, k_morph_factored's fma chains statement for statement:
//     tau_s   = sum_c w_c p_{s,c,e}                 one fma per corner, from 0.0
//     ups_s,j = sum_c d_j w_c p_{s,c,e}             (GRAD)
//     lam     = sum_s r_s tau_s                     one fma per source, from 0.0; a source whose tau_s is nan is left out of the
//                                                   event (numpy.nansum): its tau_s and ups_s,j count as +0.0 there
//     clamped = outlier != 0 and not (lam > 0):     lam := outlier, g := 0;   otherwise g = 1 / lam
// and the result slots of an item (k_sourcewise_nonempty's layout)
//     [0]                      sum_e log lam        (the host subtracts sum_s r_s, one number per item: k_finish's slot_lg)
//     [1 + s]                  sum_e g tau_s        (GRAD; the host subtracts 1: the integral of a pdf, exactly)
//     [1 + SC + s EM + j]      sum_e g ups_s,j      (GRAD; nothing to subtract: the integral does not move)
//
// A column behind the set's N_t events is masked BY INDEX (item_n): it holds zeros in every row and would otherwise take the
// outlier clamp.  It contributes exactly +0.0 to every slot.
// The tile walk is k_sourcewise_nonempty's (ListTiles): min(tiles of the item's set, max_blocks) blocks, the set's length alone
// decides, a block beyond the item's own count posts +0.0 with a clear flag.  Classes (SC, EM) and events in flight per thread
// are k_morph_factored's (factored_vec), for both GRAD variants: a values-only call has the bits of the call with the gradient.
// No nontemporal loads (the store is meant to be read again from cache), no floating-point atomics.  Registers, LDS and scratch
// of every instantiation: profiles/sourcewise_events_kernel_resources.txt (no scratch in any).
#pragma once

#include "bi_k_factored.h"

namespace {

template <int SC, int EM, bool GRAD>
__global__ __launch_bounds__(kThreads) void k_sourcewise_events(SourcewiseEventsArgs a) {
    constexpr int NC = 1 << EM, W = 1 + EM, V = factored_vec<SC, EM>();
    constexpr int NSL = GRAD ? 1 + SC * W : 1;
    static_assert(SC <= 8 && kBinsPerThread == 2, "SourcewiseEventsArgs::e holds 8 sources; a tile is two events per thread");
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
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * W;
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const int64_t n_events = a.item_n[item];
    const double outlier = a.outlier;
    log_table_load();

    double sum[NSL];
#pragma unroll
    for (int g = 0; g < NSL; ++g) sum[g] = 0.0;

    for (ListTiles w(a, n_tiles, nbx); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int part = 0; part < kBinsPerThread / V; ++part) {
            // V = 2: the thread's two neighbouring events, one 16-byte load per row; V = 1: one event of each half of the tile
            const int64_t ev = (int64_t)tile * kTile + (V == 2 ? 2 * (int)threadIdx.x : part * kThreads + (int)threadIdx.x);
            double tau[SC][V], ups[GRAD ? SC : 1][EM][V], lam[V];
#pragma unroll
            for (int v = 0; v < V; ++v) lam[v] = 0.0;
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
                        const double* src = a.ps + rowoff[k + c] + ev;
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
                for (int v = 0; v < V; ++v) {
                    if (tau[s][v] != tau[s][v]) {       // a nan corner: the source leaves this event (nansum)
                        tau[s][v] = 0.0;
                        if constexpr (GRAD) {
#pragma unroll
                            for (int j = 0; j < EM; ++j) ups[s][j][v] = 0.0;
                        }
                    } else {
                        lam[v] = fma(r, tau[s][v], lam[v]);
                    }
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                double l = lam[v];
                const bool clamped = outlier != 0.0 && !(l > 0.0);
                if (clamped) l = outlier;
                const double lg = bin_log(l);
                if (ev + v < n_events) {                // (by index: a padded column holds zeros and would take the clamp)
                    sum[0] += lg;
                    if constexpr (GRAD) {
                        const double g = clamped ? 0.0 : 1.0 / l;
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
    }

    item_reduce_store(sum, item, a.partial, a.pflags);
}

}  // namespace
