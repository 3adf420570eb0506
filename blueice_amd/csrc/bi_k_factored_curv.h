// bi_k_factored_curv.h -- k_factored_curv<SC, EM, FISHER, PS, PANEL>: the sums from which the host half (bi_factored_curv.h) forms
// the Hessian (FISHER = false, reads counts) or the expected information (FISHER = true, no data) of ONE point of a source-wise
// model per work item.  Translation units tu_factored_curv.hip (observed form) and tu_factored_fisher.hip (Fisher form).
//
// Every first and second derivative of mu_b = sum_s r_s tau_s,b is a fixed combination of a few per-source basis columns,
// because source s is multilinear over its e_s <= EM own axes (notation of bi_k_factored.h):
//     tau_s    = sum_c w_c p_{s,c,b}
//     ups_s,j  = sum_c d_j w_c p_{s,c,b}                    j < EM
//     chi_s,x  = sum_c d_j d_k w_c p_{s,c,b}                x = k (k - 1) / 2 + j for j < k < EM (observed form only; d_jj = 0)
// The first-order basis is u_a, a = s (1 + EM) + (0: tau_s, 1 + j: ups_s,j), K = SC (1 + EM) columns (padded source slots and
// axes are zero columns).  With f = n / mu - 1 (n = 0: -1) and inv = 1 / mu (n = 0: 0) the observed form sums
//     [0]                           sum_b poisson_term(n, mu)         } bit for bit the slots of k_morph_factored<SC, EM, true>:
//     [1 + s], [1 + SC + s EM + j]  sum_b f tau_s, sum_b f ups_s,j    } the same fma chains, bins per thread and order of bins
//     [1 + K + s NX + x]            sum_b f chi_s,x                   NX = EM (EM - 1) / 2
//     Q_ab = sum_b ((n inv u_a) inv) u_b                              a >= b; no 1 / mu^2 is formed (it overflows in far tails)
// and the Fisher form (inv = 1 / mu where mu > 0, else 0)
//     [0]                           sum_b mu_b                        (nan where some mu_b is negative or nan)
//     [1 + s]                       bins with mu_b == 0 and M_s tau_s != 0                          (d mu_b / d rs_s)
//     [1 + SC + s EM + j]           bins with mu_b == 0 and d mu_b / d z_i != 0, i the axis of slot (s, j), in the slot the host
//                                   marked as the axis' leader (a.lead): the sum over every slot (t, k) of the same axis of
//                                   chain[t][1 + k] tau_t + r_t ups_t,k, formed inside the mu_b == 0 branch only
//     Q'_ab = sum_b (inv u_a) u_b                                     a >= b, the bins with mu_b > 0
// The Gram has K (K + 1) / 2 pairs, up to 528, which no thread can hold.  It is split into panels of PS whole sources: panel
// PANEL accumulates the rows a of its sources against all columns b <= a, recomputing every basis column (mu needs them all);
// the linear slots are panel 0's, the other panels post their pairs alone.  All indices into the register arrays are compile-time
// constants.  One bin in flight per thread; the thread's bins are 2 t, 2 t + 1 of a tile where factored_vec<SC, EM>() == 2 and
// t, t + 256 otherwise, which is what fixes the bits of the shared slots.  Dense rows, plain loads (the bits do not depend on the
// cache policy; a nontemporal variant would double the build for a call that is not on the fit's hot path).
// No floating-point atomics; tile walk and block reduction are bi_k_item.h's.
// Registers of every instantiation: profiles/factored_curv_kernel_resources.txt.  No scratch in any; the three largest observed
// panel-0 kernels park four more VGPRs in AGPRs beside the accumulators the compiler keeps there (reported as spill_v 4).
#pragma once

#include "bi_k_factored.h"

namespace {

// first Gram row of panel PANEL, and the pairs of rows [lo, hi) against all columns up to the row
constexpr int curv_row0(int EM, int PS, int PANEL) { return PANEL * PS * (1 + EM); }
constexpr int curv_tri(int a) { return a * (a + 1) / 2; }
constexpr int curv_pairs(int EM, int PS, int PANEL) { return curv_tri(curv_row0(EM, PS, PANEL + 1)) - curv_tri(curv_row0(EM, PS, PANEL)); }

template <int SC, int EM, bool FISHER, int PS, int PANEL>
__global__ __launch_bounds__(kThreads) void k_factored_curv(FactoredArgs a) {
    constexpr int NC = 1 << EM, W = 1 + EM, NX = FISHER ? 0 : EM * (EM - 1) / 2, WC = W + NX, V = factored_vec<SC, EM>();
    constexpr int K = SC * W, A0 = curv_row0(EM, PS, PANEL), A1 = curv_row0(EM, PS, PANEL + 1), NP = curv_pairs(EM, PS, PANEL);
    constexpr bool LIN = PANEL == 0;
    constexpr int NL = LIN ? factored_curv_linear(SC, EM, FISHER) : 1, NXA = (LIN && NX > 0) ? NX : 1;
    static_assert(SC <= 8 && SC % PS == 0 && A1 <= K && kBinsPerThread == 2, "panels of whole sources");
    static_assert(NP <= 136, "at most 136 pair accumulators per thread");
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NR;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * WC;
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const double* __restrict__ chain = FISHER ? a.chain + (int64_t)item * K : nullptr;   // [K] M_s, then rs_s dM_s,j (the counts' only reader)
    const double* __restrict__ cnt = FISHER ? nullptr : a.counts + a.item_cnt[item];
    if constexpr (!FISHER) log_table_load();

    double sum[NL], gram[NP];
#pragma unroll
    for (int g = 0; g < NL; ++g) sum[g] = 0.0;
#pragma unroll
    for (int g = 0; g < NP; ++g) gram[g] = 0.0;

    for (ItemTiles w(a, a.n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
#pragma unroll 1
        for (int part = 0; part < kBinsPerThread; ++part) {
            const int64_t bin = (int64_t)tile * kTile + (V == 2 ? 2 * (int)threadIdx.x + part : part * kThreads + (int)threadIdx.x);
            double u[K], chi[SC][NXA], mu = 0.0;
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
                        const double p = a.ps[rowoff[k + c] + bin];
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
                mu = fma(rate[s], u[s * W], mu);
            }
            double inv, wn;             // Gram pair a >= b: the row factor ((wn inv) u_a) inv (observed) or inv u_a, times u_b
            if constexpr (FISHER) {
                inv = mu > 0.0 ? 1.0 / mu : 0.0;
                wn = 1.0;
                if constexpr (LIN) {
                    sum[0] += mu >= 0.0 ? mu : __builtin_nan("");
                    if (mu == 0.0) {    // rare: bins nothing fills (every slope 0 as well) or bins in which the information is unbounded
#pragma unroll
                        for (int s = 0; s < SC; ++s) {
                            sum[1 + s] += chain[s * W] * u[s * W] != 0.0 ? 1.0 : 0.0;
#pragma unroll
                            for (int j = 0; j < EM; ++j) {
                                if ((a.lead >> (s * 3 + j)) & 1u) {         // uniform: the first slot of its axis
                                    const int ax = a.ax[s][j];
                                    double dv = 0.0;
#pragma unroll
                                    for (int t = s; t < SC; ++t) {
#pragma unroll
                                        for (int kk = 0; kk < EM; ++kk) {
                                            if (a.ax[t][kk] == ax) {        // uniform
                                                dv = fma(chain[t * W + 1 + kk], u[t * W], dv);
                                                dv = fma(rate[t], u[t * W + 1 + kk], dv);
                                            }
                                        }
                                    }
                                    sum[1 + SC + s * EM + j] += dv != 0.0 ? 1.0 : 0.0;
                                }
                            }
                        }
                    }
                }
            } else {
                const double n = cnt[bin];
                inv = n != 0.0 ? 1.0 / mu : 0.0;
                wn = n;
                if constexpr (LIN) {
                    sum[0] += poisson_term(n, mu);
                    const double f = n * inv - 1.0;
#pragma unroll
                    for (int s = 0; s < SC; ++s) {
                        sum[1 + s] = fma(f, u[s * W], sum[1 + s]);
#pragma unroll
                        for (int j = 0; j < EM; ++j) sum[1 + SC + s * EM + j] = fma(f, u[s * W + 1 + j], sum[1 + SC + s * EM + j]);
#pragma unroll
                        for (int x = 0; x < NX; ++x) sum[1 + K + s * NX + x] = fma(f, chi[s][x], sum[1 + K + s * NX + x]);
                    }
                }
            }
#pragma unroll
            for (int r = A0; r < A1; ++r) {
                const double t = FISHER ? inv * u[r] : ((wn * inv) * u[r]) * inv;
#pragma unroll
                for (int b = 0; b <= r; ++b) gram[curv_tri(r) - curv_tri(A0) + b] = fma(t, u[b], gram[curv_tri(r) - curv_tri(A0) + b]);
            }
        }
    }

    if constexpr (LIN) item_reduce_store(sum, gram, item, a.partial, a.pflags);
    else item_reduce_store(gram, item, a.partial, a.pflags);
}

}  // namespace

// ---- the launchers: panel `panel` of class (SC, EM); BI_ERR_INVALID where there is no such instantiation
namespace {

template <int SC, int EM, bool FISHER, int PANEL>
int launch_curv_panel(bi_ctx* c, int panel, const FactoredArgs& a, dim3 grid) {
    constexpr int PS = factored_curv_panel_sources(SC, EM);
    if (panel == PANEL) {
        hipLaunchKernelGGL((k_factored_curv<SC, EM, FISHER, PS, PANEL>), grid, dim3(kThreads), 0, c->stream, a);
        return BI_OK;
    }
    if constexpr (PANEL + 1 < factored_curv_panels(SC, EM)) return launch_curv_panel<SC, EM, FISHER, PANEL + 1>(c, panel, a, grid);
    return BI_ERR_INVALID;
}

template <int SC, bool FISHER>
int launch_curv_sc(bi_ctx* c, int EM, int panel, const FactoredArgs& a, dim3 grid) {
    switch (EM) {
        case 1: return launch_curv_panel<SC, 1, FISHER, 0>(c, panel, a, grid);
        case 2: return launch_curv_panel<SC, 2, FISHER, 0>(c, panel, a, grid);
        case 3: return launch_curv_panel<SC, 3, FISHER, 0>(c, panel, a, grid);
    }
    return BI_ERR_INVALID;
}

// every (SC, EM, panel) of one form: what a translation unit instantiates
template <bool FISHER>
int launch_curv_form(bi_ctx* c, int SC, int EM, int panel, const FactoredArgs& a, dim3 grid) {
    EventScope ev(c);
    if (panel < 0) return BI_ERR_INVALID;
    switch (SC) {
        case 2: return launch_curv_sc<2, FISHER>(c, EM, panel, a, grid);
        case 4: return launch_curv_sc<4, FISHER>(c, EM, panel, a, grid);
        case 8: return launch_curv_sc<8, FISHER>(c, EM, panel, a, grid);
    }
    return BI_ERR_INVALID;
}

}  // namespace
