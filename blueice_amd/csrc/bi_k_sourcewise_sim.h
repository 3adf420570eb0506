// bi_k_sourcewise_sim.h -- event-level toys of a source-wise model (translation unit tu_sourcewise_sim.hip; host half
// bi_sourcewise_sim.h).  The stream is bi_simulate_event_toys' (include/blueice_hip.h), drawn through the same device functions
// (bi_k_draw.h): toy D = toy0 + t of the seed's ensemble is keyed by toy_seed(seed, D), N_s ~ Poisson(r_s) through
// toy_event_count with k_sim_toy_counts' key, every event through sim_one_event on the running sums of its source's pmf row.
//
// k_sourcewise_pmf<SC, EM>: grid (tile, truth); out[truth][s][b] = max(tau_s,b, 0) vol_b with tau_s from sourcewise_chain's fma
// statements (bi_k_sourcewise.h: two bins per thread, one 16-byte load per corner row) and vol_b the product of the bin's widths,
// axis 0 first, from 1.0 -- k_sim_pmf's statements on what k_morph_store writes, in one pass over the truth's sum_s 2^e_s rows
// and without the S x B intermediate.  The rows of `out` have the stride B (sim_one_event's): 8-byte stores, the pad bins behind
// B are not written.
//
// k_sourcewise_sim_counts: N_{t,s} of all (t, s) from the rates of the toy's truth; k_sourcewise_sim_room: the columns a toy takes
// in the event store (whole tiles, at least one); k_sourcewise_sim_first: the first column of every (t, s) behind the exclusive
// scan of the rooms; k_sourcewise_sim_events: one thread per column of a sub-batch's toys -- the toy by bisection in set_first,
// the source from the per-toy starts, the event on the cdf rows of the toy's truth; padding columns get coordinate 0 and
// source -1.  A toy depends on (seed, D) and its truth alone: not on T, the launch geometry or the sub-batches.
// No floating-point atomics.  Registers, LDS and scratch of every instantiation: profiles/sourcewise_sim_kernel_resources.txt.
#pragma once

#include "bi_k_sourcewise.h"
#include "bi_k_draw.h"

namespace {

// the volume of bin b: k_sim_pmf's statements
__device__ __forceinline__ double sim_bin_volume(const SimArgs& a, const double* __restrict__ edges, int64_t b) {
    double vol = 1.0;
    int64_t rem = b;
    for (int ax = 0; ax < a.k; ++ax) {
        const int64_t i = rem / a.stride[ax];
        rem -= i * a.stride[ax];
        const double* __restrict__ e = edges + a.edge_off[ax];
        vol *= e[i + 1] - e[i];
    }
    return vol;
}

template <int SC, int EM>
__global__ __launch_bounds__(kThreads) void k_sourcewise_pmf(SourcewisePmfArgs x) {
    const FactoredArgs& a = x.f;
    const int item = blockIdx.y;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * a.NR;
    const double* __restrict__ coef = a.coef + (int64_t)item * a.NR * (1 + EM);
    const double* __restrict__ rate = a.rates + (int64_t)item * SC;
    const int64_t bin = (int64_t)blockIdx.x * kTile + 2 * (int)threadIdx.x;       // (the grid has Bp / kTile tiles: bin + 1 < Bp)
    if (bin >= x.B) return;                     // (uniform per thread from here on: nothing is reduced)
    double tau[SC][2], mu[2];
    sourcewise_chain<SC, EM, false>(a, rowoff, coef, rate, bin, tau, mu);
    const bool has1 = bin + 1 < x.B;
    const double vol0 = sim_bin_volume(x.sim, x.edges, bin);
    const double vol1 = has1 ? sim_bin_volume(x.sim, x.edges, bin + 1) : 0.0;
    double* __restrict__ out = x.out + (int64_t)item * x.sim.S * x.B + bin;
#pragma unroll
    for (int s = 0; s < SC; ++s) {
        if (s < x.sim.S) {
            const double v0 = tau[s][0] * vol0, v1 = tau[s][1] * vol1;
            out[(int64_t)s * x.B] = v0 > 0.0 ? v0 : 0.0;
            if (has1) out[(int64_t)s * x.B + 1] = v1 > 0.0 ? v1 : 0.0;
        }
    }
}

// N_{t,s} ~ Poisson(r_s at the toy's truth): k_sim_toy_counts with a truth per toy
__global__ __launch_bounds__(256) void k_sourcewise_sim_counts(SourcewiseSimArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = a.sim.S;
    if (i >= a.T * S) return;
    const int64_t t = i / S;
    const int s = (int)(i - t * S);
    const double M = a.rates[(int64_t)a.truth[t] * a.rate_stride + s];
    const uint64_t ts = toy_seed(a.seed, (uint64_t)(a.toy0 + t));
    a.n[i] = (M > 0.0 && M < kSimMaxRate) ? (int64_t)toy_event_count(M, ts ^ 0x9E3779B97F4A7C15ull, (int64_t)s) : 0;
}

// the columns a toy takes in the event store: its events rounded up to whole tiles, at least one; room [T + 1] (last 0) goes
// through an exclusive prefix sum -> set_first [T + 1]
__global__ void k_sourcewise_sim_room(SourcewiseSimArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > a.T) return;
    if (t == a.T) { a.room[t] = 0; return; }
    int64_t tot = 0;
    for (int s = 0; s < a.sim.S; ++s) tot += a.n[t * a.sim.S + s];
    const int64_t tiles = (tot + kTile - 1) / kTile;
    a.room[t] = (tiles < 1 ? 1 : tiles) * kTile;
}

// first_{t,s} = set_first_t + sum_{s' < s} N_{t,s'}: [T][S + 1], the last entry the end of the toy's events
__global__ void k_sourcewise_sim_first(SourcewiseSimArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T) return;
    const int S = a.sim.S;
    int64_t at = a.set_first[t];
    for (int s = 0; s < S; ++s) { a.first[t * (S + 1) + s] = at; at += a.n[t * S + s]; }
    a.first[t * (S + 1) + S] = at;
}

__global__ __launch_bounds__(kThreads) void k_sourcewise_sim_events(SourcewiseSimArgs a) {
    const int64_t e = a.col0 + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.col0 + a.ncols) return;
    const int S = a.sim.S;
    int64_t lo = a.t0, hi = a.t0 + a.nt;             // the last t of the sub-batch with set_first[t] <= e (every toy has room)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.set_first[mid] <= e) lo = mid; else hi = mid;
    }
    const int64_t t = lo;
    const int64_t* __restrict__ f = a.first + t * (S + 1);
    if (e >= f[S]) {                                 // padding
        for (int ax = 0; ax < a.sim.k; ++ax) a.coords[(int64_t)ax * a.cols + e] = 0.0;
        a.source[e] = -1;
        return;
    }
    int s = 0;
    while (s + 1 < S && e >= f[s + 1]) ++s;
    const double* __restrict__ cdf = a.cdf + ((int64_t)a.truth[t] - a.h0) * S * a.B;
    sim_one_event(cdf, a.B, a.sim, a.edges, toy_seed(a.seed, (uint64_t)(a.toy0 + t)), s, e - f[s], a.cols, e, a.coords, a.source);
}

}  // namespace
