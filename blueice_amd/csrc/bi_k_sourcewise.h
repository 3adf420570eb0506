// bi_k_sourcewise.h -- the per-bin expectation of a source-wise model, written out or summed into the goodness-of-fit forms.
// Translation units tu_sourcewise_expect.hip and tu_sourcewise_gof.hip; host half bi_sourcewise.h.
//
// sourcewise_chain<SC, EM, NT>: tau_s and mu of a thread's two neighbouring bins in exactly k_morph_factored's statement order
// (bi_k_factored.h) -- per source tau from 0.0 with one fma per corner, then mu = fma(r_s, tau_s, mu) from 0.0, sources
// ascending -- so mu_b here has the bits of the mu_b the likelihood kernel forms.  The descriptors are FacBatch's of order 0
// (bi_factored.h): row offsets, coef [NR][1 + EM] of which column 0 (w_c) is read, rates [SC]; all uniform per item and read
// through scalar loads.  Both kernels keep two bins in flight at every (SC, EM) class, one 16-byte load per row: without the
// gradient's ups columns a thread holds at most SC = 8 tau pairs.  sourcewise_chain_bin<SC, EM> restates the chain for one bin per
// thread (k_sourcewise_coarse, bi_k_sourcewise_coarse.h): the same statements, the same bits.
//
// k_sourcewise_expect<SC, EM, PS, NT>: grid (tile, item); out[item][0][b] = mu_b, or with PS out[item][s][b] = r_s tau_s,b (one
// multiply) for the sources the model has, one 16-byte store per row of stride Bp.  Nothing is reduced and no counts are read.
//
// k_sourcewise_gof<SC, EM, NT>: the tile walk and block reduction of bi_k_item.h around the chain and gof_terms (bi_k_gof_terms.h, k_morph_gof's):
// slot 0 the half-deviance, slot 1 Pearson's chi2 of the item's dataset.  No floating-point atomics; with the host's fixed
// number of blocks per item a point's bits do not depend on the batch it is evaluated in.
// Registers, LDS and scratch of every instantiation: profiles/sourcewise_toys_kernel_resources.txt (no scratch in any).
#pragma once

#include "bi_k_item.h"
#include "bi_k_gof_terms.h"

namespace {

template <int SC, int EM, bool NT>
__device__ __forceinline__ void sourcewise_chain(const FactoredArgs& a, const int64_t* __restrict__ rowoff, const double* __restrict__ coef,
                                                 const double* __restrict__ rate, int64_t bin, double (&tau)[SC][2], double (&mu)[2]) {
    constexpr int NC = 1 << EM, W = 1 + EM;
    static_assert(SC <= 8 && kBinsPerThread == 2, "FactoredArgs::e holds 8 sources; a tile is two bins per thread");
    mu[0] = mu[1] = 0.0;
    int k = 0;                  // the source's first row: uniform
#pragma unroll
    for (int s = 0; s < SC; ++s) {
        tau[s][0] = tau[s][1] = 0.0;
        const int nc = a.e[s] < 0 ? 0 : 1 << a.e[s];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < nc) {
                const double2 p = stream_load<NT>(a.ps + rowoff[k + c] + bin);
                const double w = coef[(int64_t)(k + c) * W];
                tau[s][0] = fma(w, p.x, tau[s][0]);
                tau[s][1] = fma(w, p.y, tau[s][1]);
            }
        }
        k += nc;
        const double r = rate[s];
        mu[0] = fma(r, tau[s][0], mu[0]);
        mu[1] = fma(r, tau[s][1], mu[1]);
    }
}

// The same chain for ONE bin per thread, statement for statement: k_sourcewise_coarse (bi_k_sourcewise_coarse.h), whose lanes lie
// along the last analysis axis at bins r L + x that are not 16-byte aligned in general (8-byte loads).
template <int SC, int EM>
__device__ __forceinline__ void sourcewise_chain_bin(const FactoredArgs& a, const int64_t* __restrict__ rowoff, const double* __restrict__ coef,
                                                     const double* __restrict__ rate, int64_t bin, double (&tau)[SC], double& mu) {
    constexpr int NC = 1 << EM, W = 1 + EM;
    static_assert(SC <= 8, "FactoredArgs::e holds 8 sources");
    mu = 0.0;
    int k = 0;                  // the source's first row: uniform
#pragma unroll
    for (int s = 0; s < SC; ++s) {
        tau[s] = 0.0;
        const int nc = a.e[s] < 0 ? 0 : 1 << a.e[s];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < nc) {
                const double p = a.ps[rowoff[k + c] + bin];
                const double w = coef[(int64_t)(k + c) * W];
                tau[s] = fma(w, p, tau[s]);
            }
        }
        k += nc;
        const double r = rate[s];
        mu = fma(r, tau[s], mu);
    }
}

template <int SC, int EM, bool PS, bool NT>
__global__ __launch_bounds__(kThreads) void k_sourcewise_expect(SourcewiseExpectArgs x) {
    const FactoredArgs& a = x.f;
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NR;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * (1 + EM);
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const int64_t bin = (int64_t)blockIdx.x * kTile + 2 * (int)threadIdx.x;       // (the grid has Bp / kTile tiles: bin + 1 < Bp)
    double tau[SC][2], mu[2];
    sourcewise_chain<SC, EM, NT>(a, rowoff, coef, rate, bin, tau, mu);
    double* __restrict__ out = x.out + (int64_t)item * x.R * x.Bp + bin;
    if constexpr (PS) {
#pragma unroll
        for (int s = 0; s < SC; ++s) {
            if (s < x.R) {
                const double r = rate[s];
                *reinterpret_cast<double2*>(out + (int64_t)s * x.Bp) = make_double2(r * tau[s][0], r * tau[s][1]);
            }
        }
    } else {
        *reinterpret_cast<double2*>(out) = make_double2(mu[0], mu[1]);
    }
}

template <int SC, int EM, bool NT>
__global__ __launch_bounds__(kThreads) void k_sourcewise_gof(FactoredArgs a) {
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NR;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * (1 + EM);
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const double* __restrict__ cnt = a.counts + a.item_cnt[item];
    log_table_load();

    double sum[2] = {0.0, 0.0};      // half-deviance, Pearson
    for (ItemTiles w(a, a.n_tiles); w.more(); w.step()) {
        const int tile = w.tile();
        if (tile < 0) continue;
        const int64_t bin = (int64_t)tile * kTile + 2 * (int)threadIdx.x;
        const double2 n = stream_load<NT>(cnt + bin);
        double tau[SC][2], mu[2];
        sourcewise_chain<SC, EM, NT>(a, rowoff, coef, rate, bin, tau, mu);
        gof_terms(n.x, mu[0], sum[0], sum[1]);
        gof_terms(n.y, mu[1], sum[0], sum[1]);
    }

    item_reduce_store(sum, item, a.partial, a.pflags);
}

}  // namespace
