// bi_k_sourcewise_real.h -- k_sourcewise_real<SC, EM, GRAD, NT>: the half-deviance of ONE (point of a source-wise model,
// real-valued dataset) per work item, and the partial sums its gradient is made of.  Translation unit tu_sourcewise_real.hip;
// host half bi_sourcewise_real.h.
//
// The walk is k_morph_factored's (bi_k_factored.h), statement by statement: the item's rows are its sources' corner rows back
// to back, per bin b
//     tau_s   = sum_c w_c p_{s,c,b}                 one fma per corner, from 0.0
//     ups_s,j = sum_c d_j w_c p_{s,c,b}             (GRAD) j < EM
//     mu      = sum_s r_s tau_s                     one fma per source, from 0.0
// so mu_b here has the bits of the mu_b of k_morph_factored and of sourcewise_chain (bi_k_sourcewise.h), which is what
// k_sourcewise_expect writes into an Asimov dataset.  The per-bin terms are k_morph_real's (bi_k_real.h), n any real number >= 0
// (bi_sourcewise_set_real_counts / bi_sourcewise_set_asimov_counts admit nothing else; there is no integer test):
//     dev     = n > 0: (mu - n) - n log(mu / n)     n = 0: mu          (mu = 0 under n > 0: +inf; mu negative or nan: nan)
//     f       = n > 0: 1 - n / mu                   n = 0: 1
// and the result slots of an item are
//     [0]                      sum_b dev
//     [1 + s]                  sum_b f tau_s                        (GRAD)
//     [1 + SC + s EM + j]      sum_b f ups_s,j                      (GRAD)
// from which the host forms the gradient with FacBatch::gradient's chain rule (bi_factored.h: it is linear in the slots).  At
// the truth of an Asimov dataset mu_b == n_b bit for bit, mu / n == 1.0, bin_log(1.0) == 0.0 and 1 - n / mu == 0.0: slot 0 and
// every gradient slot are 0.0 exactly.  The derivative slots of an item whose slot 0 is not finite are whatever the arithmetic
// makes of them; the host reports nan for them.
//
// Register discipline and bins in flight are k_morph_factored's as well: tau and ups stay in registers until mu is complete,
// every index into them a compile-time constant; two bins per thread from one 16-byte load per row where factored_vec<SC, EM>()
// says so (SC (1 + EM) <= 16), one bin in flight otherwise -- in BOTH GRAD variants of a class, since which bins a thread adds
// up fixes the bits of slot 0 and a value-only call must give the bits of the call with the gradient.  With that choice no
// class spills (profiles/sourcewise_real_kernel_resources.txt: no scratch in any instantiation), so no class departs from it.
// No floating-point atomics; tile walk and block reduction are bi_k_item.h's, so a repeated call is bitwise identical, and with
// the host's fixed number of blocks per item a point's bits do not depend on the batch it is evaluated in.
#pragma once

#include "bi_k_factored.h"

namespace {

template <int SC, int EM, bool GRAD, bool NT>
__global__ __launch_bounds__(kThreads) void k_sourcewise_real(FactoredArgs a) {
    constexpr int NC = 1 << EM, W = 1 + EM, V = factored_vec<SC, EM>();
    constexpr int NSL = GRAD ? 1 + SC * W : 1;
    static_assert(SC <= 8 && kBinsPerThread == 2, "FactoredArgs::e holds 8 sources; a tile is two bins per thread");
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NR;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * W;
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const double* __restrict__ cnt = a.counts + a.item_cnt[item];
    log_table_load();

    double sum[NSL];
#pragma unroll
    for (int g = 0; g < NSL; ++g) sum[g] = 0.0;

    for (ItemTiles w(a, a.n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int part = 0; part < kBinsPerThread / V; ++part) {
            // V = 2: the thread's two neighbouring bins, one 16-byte load per row; V = 1: one bin of each half of the tile
            const int64_t bin = (int64_t)tile * kTile + (V == 2 ? 2 * (int)threadIdx.x : part * kThreads + (int)threadIdx.x);
            double n[V];
            if constexpr (V == 2) {
                const double2 t = stream_load<NT>(cnt + bin);
                n[0] = t.x; n[1] = t.y;
            } else {
                n[0] = NT ? __builtin_nontemporal_load(cnt + bin) : cnt[bin];
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
                            const double2 t = stream_load<NT>(src);
                            p[0] = t.x; p[1] = t.y;
                        } else {
                            p[0] = NT ? __builtin_nontemporal_load(src) : *src;
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
                double dev = mu[v], f = 1.0;
                if (n[v] > 0.0) {
                    dev = (mu[v] - n[v]) - n[v] * bin_log(mu[v] / n[v]);      // mu = 0: +inf
                    f = 1.0 - n[v] / mu[v];
                }
                if (!(mu[v] >= 0.0)) dev = __builtin_nan("");
                sum[0] += dev;
                if constexpr (GRAD) {
#pragma unroll
                    for (int s = 0; s < SC; ++s) {
                        sum[1 + s] = fma(f, tau[s][v], sum[1 + s]);
#pragma unroll
                        for (int j = 0; j < EM; ++j) sum[1 + SC + s * EM + j] = fma(f, ups[s][j][v], sum[1 + SC + s * EM + j]);
                    }
                }
            }
        }
    }

    item_reduce_store(sum, item, a.partial, a.pflags);
}

}  // namespace
