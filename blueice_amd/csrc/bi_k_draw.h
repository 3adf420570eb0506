// bi_k_draw.h -- the device functions every event-level generator draws through, in one place so that the translation units
// that hold generator kernels (bi_k_misc.h in the main one, bi_k_sourcewise_sim.h in tu_sourcewise_sim.hip) share one
// definition of a stream: the Poisson samplers, the number of events of a toy (toy_event_count), the seed of toy D of an
// ensemble (toy_seed) and one event of one source (sim_one_event).  No kernel is defined here.
#pragma once

#include "bi_philox.h"

namespace {

// lam < 10: inversion by sequential search with one 53-bit uniform; p0 = exp(-lam) comes from a per-bin table (it is
// the same for every toy)
__device__ __forceinline__ double poisson_small(double lam, double p0, double u) {
    double p = p0, F = p, n = 0.0;
    while (u > F && n < 1000.0) {
        n += 1.0;
        p *= lam / n;
        F += p;
    }
    return n;
}

// lam >= 10: PTRS, Hoermann (1993): transformed rejection with squeeze, as in numpy's random_poisson_ptrs
__device__ double poisson_ptrs(double lam, uint64_t seed, int64_t t, int64_t b) {
    uint32_t r[4];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const double slam = sqrt(lam), loglam = log(lam);
    const double bb = 0.931 + 2.53 * slam, aa = -0.059 + 0.02483 * bb;
    const double invalpha = 1.1239 + 1.1328 / (bb - 3.4), vr = 0.9277 - 3.6224 / (bb - 2.0);
    for (uint32_t attempt = 0; attempt < 4096u; ++attempt) {
        philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)t, ((uint32_t)(t >> 32) & 0xFFFFu) | ((attempt + 1u) << 16), k0, k1, r);
        const double U = u53(r[0], r[1]) - 0.5, V = u53(r[2], r[3]);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * aa / us + bb) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(aa / (us * us) + bb) <= -lam + k * loglam - lgamma(k + 1.0)) return k;
    }
    return floor(lam);  // unreachable in practice (acceptance > 0.9 per attempt)
}

constexpr uint32_t kEvTag = 0x45564E54u;        // separates the event counters from the per-bin ones

__device__ __forceinline__ int toy_event_count(double M, uint64_t seed, int64_t t) {
    if (M >= 10.0) return (int)poisson_ptrs(M, seed, t, ((int64_t)1 << 40) + 7);          // a "bin" no model has
    uint32_t r[4];
    philox4x32_10(0xFFFFFFFFu, kEvTag, (uint32_t)t, (uint32_t)(t >> 32) & 0xFFFFu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return (int)poisson_small(M, exp(-M), u53(r[0], r[1]));
}

constexpr uint32_t kSimTag = 0x53494D45u;
constexpr double kSimMaxRate = 1073741824.0;   // 2^30 expected events per source: toy_event_count returns an int, bi_simulate_events refuses more

// event j of source s of the toy keyed by `seed`, stored at column e of coords [k][N]
__device__ __forceinline__ void sim_one_event(const double* __restrict__ cdf /*[S][B]*/, int64_t B, const SimArgs& a,
                                              const double* __restrict__ edges, uint64_t seed, int s, int64_t j, int64_t N, int64_t e,
                                              double* __restrict__ coords /*[k][N]*/, int32_t* __restrict__ source /*[N]*/) {
    const double* __restrict__ F = cdf + (int64_t)s * B;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t r[4];
    philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), (uint32_t)s, kSimTag, k0, k1, r);
    const double target = u53(r[0], r[1]) * F[B - 1];
    int64_t lo = 0, hi = B;                                              // first bin whose cumulative sum exceeds the target
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (F[mid] <= target) lo = mid + 1; else hi = mid;
    }
    int64_t rem = min(lo, B - 1);
    for (int ax = 0; ax < a.k; ++ax) {
        // the position inside the bin: one uniform per axis, counter (event, source, axis)
        philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), (uint32_t)s | ((uint32_t)ax << 24), kSimTag + 1u, k0, k1, r);
        const double u = u53(r[0], r[1]);
        const int64_t i = rem / a.stride[ax];
        rem -= i * a.stride[ax];
        const double* __restrict__ ed = edges + a.edge_off[ax];
        // (uniform inside the bin, as Histdd.get_random draws it, source.py:248-264; a 'linear' pdf clips to the outer bin
        //  centres only when it is EVALUATED, source.py:231-239: k_score_locate does that, the stored events stay as drawn)
        coords[(int64_t)ax * N + e] = ed[i] + u * (ed[i + 1] - ed[i]);
    }
    source[e] = s;
}

// Toy D of the seed's ensemble is bi_simulate_events' toy with the seed toy_seed(seed, D) (include/blueice_hip.h): D ->
// seed + (D + 1) c is one-to-one modulo 2^64 (c odd), the rest is the bijective finaliser of splitmix64.
__host__ __device__ inline uint64_t toy_seed(uint64_t seed, uint64_t D) {
    uint64_t x = seed + (D + 1ull) * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

}  // namespace
