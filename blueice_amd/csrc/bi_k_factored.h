// bi_k_factored.h -- k_morph_factored<SC, EM, GRAD, NT>: the binned Poisson log-likelihood of ONE point of a source-wise model
// per work item, and the partial sums its gradient is made of.  Translation unit tu_factored.hip; host half bi_factored.h.
//
// A source-wise model keeps one anchor grid per source, over the e_s <= EM axes that source owns.  An item's rows are its
// sources' corner rows back to back (source s: 1 << e_s of them, first own axis = most significant corner bit); per row the
// host supplies w_c and d w_c / d (own axis j), per source the rate r_s = M_s(z) rs_s.  Per bin b
//     tau_s   = sum_c w_c p_{s,c,b}                 one fma per corner, from 0.0
//     ups_s,j = sum_c d_j w_c p_{s,c,b}             (GRAD) j < EM; the host pads d_j w_c with zeros for j >= e_s
//     mu      = sum_s r_s tau_s                     one fma per source, from 0.0
//     f       = n / mu - 1                          (n = 0: -1)
// and the result slots of an item are
//     [0]                      sum_b poisson_term(n, mu)            (the host subtracts sum_b lgamma(n + 1))
//     [1 + s]                  sum_b f tau_s                        (GRAD)
//     [1 + SC + s EM + j]      sum_b f ups_s,j                      (GRAD)
// from which the host forms d ll / d rs_s = M_s [1 + s] and d ll / d z_i by the chain rule, in a fixed order.  That is
// sum_s 2^e_s (1 + e_s) fma per bin whatever the number of axes d, against NS (1 + d + S) of the dense coefficient columns.
//
// tau and ups stay in registers until mu is complete: every index into them is a compile-time constant (the loops over the SC
// source slots, the 1 << EM corners and the EM axes are fully unrolled; a source with fewer corners skips the others on a
// branch that is uniform for the whole launch: e[] lies in the kernel arguments).  The row offsets, coefficients and rates are
// uniform per item, read through scalar loads.  Two bins per thread from one 16-byte load per row where tau and ups of both
// fit comfortably (SC (1 + EM) <= 16 doubles per bin), one bin in flight otherwise, as k_morph_real.  The choice is made by
// (SC, EM) alone, for the values-only variants too, although those would have the registers for two bins at every class:
// which bins a thread adds up is what fixes the bits of ll, and a call without the gradient must give the bits of the call with
// it (include/blueice_hip.h).  What the 16-byte loads would be worth for values-only calls at <8, 2> and <8, 3> is not measured.
// No floating-point atomics; tile walk and block reduction are bi_k_item.h's, so a repeated call is bitwise identical, and with
// the host's fixed number of blocks per item a point's bits do not depend on the batch it is evaluated in.
// Registers, LDS and scratch of every instantiation: profiles/factored_kernel_resources.txt (no scratch in any).
#pragma once

#include "bi_k_item.h"

namespace {

template <int SC, int EM>
constexpr int factored_vec() { return SC * (1 + EM) <= 16 ? 2 : 1; }

template <int SC, int EM, bool GRAD, bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_factored(FactoredArgs a) {
    constexpr int NC = 1 << EM, W = 1 + EM, V = factored_vec<SC, EM>();
    constexpr int NSL = GRAD ? 1 + SC * W : 1;
    static_assert(SC <= 8 && kBinsPerThread == 2, "FactoredArgs::e holds 8 sources; a tile is two bins per thread");
    const int item = blockIdx.y;
    if constexpr (!GRAD) {
        // items planned on the device (a.live; NULL on every host path): a rejected point reads none of its descriptors, streams
        // no row and posts no partial (its perm is -1: k_finish skips it).  Uniform for the block; the register counts of
        // profiles/factored_kernel_resources.txt are those of the kernel without this line.
        if (a.live && !a.live[item]) return;
    }
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
                sum[0] += poisson_term(n[v], mu[v]);
                if constexpr (GRAD) {
                    const double inv = n[v] != 0.0 ? 1.0 / mu[v] : 0.0;
                    const double f = n[v] * inv - 1.0;
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
