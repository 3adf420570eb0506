// bi_k_sampler.h -- the two kernels between the likelihood evaluations of the ensemble sampler (bi_sample_stretch, bi_sampler.h):
// Goodman & Weare's affine-invariant stretch move (Comm. App. Math. Comp. Sci. 5, 2010) with the fixed split into two halves
// that emcee's StretchMove uses.  Translation unit tu_sampler.hip.  One thread per moving walker; both kernels derive the move
// from the same Philox block, so nothing but the proposal's log likelihood travels between them.  The random stream and the
// order of every floating-point operation are part of the interface (include/blueice_hip.h): a NumPy restatement reproduces
// the proposals bit for bit.
#pragma once

#include "bi_philox.h"

namespace {

constexpr uint32_t kStretchTag = 0x53545200u;      // "STR\0": separates the sampler's counters from the toy generators'

struct StretchMove {
    int64_t e;      // ensemble
    int k, j;       // moving walker, its partner in the other half
    double z, u_a;
};

// the move of thread i of a half-step; false: no such walker
__device__ __forceinline__ bool stretch_move(const StretchArgs& a, int64_t i, StretchMove& m) {
    const int half = a.W / 2;
    if (i >= a.E * half) return false;
    m.e = i / half;
    m.k = a.h * half + (int)(i % half);
    uint32_t r[4];
    philox4x32_10((uint32_t)m.k, (uint32_t)(a.first_ensemble + m.e), (uint32_t)a.t, kStretchTag | (uint32_t)a.h, a.k0, a.k1, r);
    const double u_z = u53(r[0], r[1]);
    m.j = (1 - a.h) * half + (int)(((uint64_t)r[2] * (uint64_t)half) >> 32);
    m.u_a = __dmul_rn(__dadd_rn((double)r[3], 0.5), 1.0 / 4294967296.0);
    const double g = __dadd_rn(__dmul_rn(__dsub_rn(a.a, 1.0), u_z), 1.0);
    m.z = __ddiv_rn(__dmul_rn(g, g), a.a);
    return true;
}

// coordinate v of the proposal: every operation rounded on its own
__device__ __forceinline__ double stretch_coord(const StretchArgs& a, const StretchMove& m, int v) {
    const double xk = a.x[(m.e * a.W + m.k) * a.F + v], xj = a.x[(m.e * a.W + m.j) * a.F + v];
    return __dadd_rn(xj, __dmul_rn(m.z, __dsub_rn(xk, xj)));
}

// The Gaussian constraint terms of ensemble e at a point whose coordinate v is coord(v), in the order include/blueice_hip.h
// states: p = prior_const[e]; per variable with a finite sigma t = (x - mean) / sigma, p = p - 0.5 (t t); every operation
// rounded on its own.  (F loads of mean and sigma per thread, from two arrays of F doubles that every thread reads alike.)
template <class Coord>
__device__ __forceinline__ double gauss_terms(const StretchArgs& a, int64_t e, Coord coord) {
    double p = a.prior_const ? a.prior_const[e] : 0.0;
    if (a.prior_sigma)
        for (int v = 0; v < a.F; ++v) {
            const double sg = a.prior_sigma[v];
            if (sg - sg == 0.0) {                                    // finite
                const double t = __ddiv_rn(__dsub_rn(coord(v), a.prior_mean[v]), sg);
                p = __dsub_rn(p, __dmul_rn(0.5, __dmul_rn(t, t)));
            }
        }
    return p;
}

// the start: every walker's log likelihood (ll_prop, row e W + k) becomes its log density.  Only launched with terms.
__global__ __launch_bounds__(kThreads) void k_stretch_start_density(const StretchArgs a) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.E * a.W) return;
    const double p = gauss_terms(a, w / a.W, [&](int v) { return a.x[w * a.F + v]; });
    a.ll[w] = __dadd_rn(a.ll_prop[w], p);
}

// h = 0 / 1: the proposals of the moving half; h = -1: every walker's own position (the log likelihoods of the start).
// Row i of z_dev / rs_dev / ds_dev is what bi_plan_points_resident reads as point i.
__global__ __launch_bounds__(kThreads) void k_stretch_propose(const StretchArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    StretchMove m;
    if (a.h < 0) {
        if (i >= a.E * a.W) return;
        m.e = i / a.W;
        m.k = (int)(i % a.W);
    } else if (!stretch_move(a, i, m))
        return;
    varmap_write_point(a, i, m.e, [&](int v) { return a.h < 0 ? a.x[(m.e * a.W + m.k) * a.F + v] : stretch_coord(a, m, v); });
}

// accept or reject the proposals of a half-step, and append the moved walkers' state to row t of the chain (the other half's
// rows of step t are written by the other half-step: a walker moves once per step)
__global__ __launch_bounds__(kThreads) void k_stretch_accept(const StretchArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    StretchMove m;
    if (!stretch_move(a, i, m)) return;
    const int64_t w = m.e * a.W + m.k;
    double ll_y = a.ll_prop[i];
    const double ll_x = a.ll[w];
    // with constraint terms the density of the proposal is ll + p, p from the proposal's own coordinates
    if (a.prior_sigma || a.prior_const) ll_y = __dadd_rn(ll_y, gauss_terms(a, m.e, [&](int v) { return stretch_coord(a, m, v); }));
    bool ok = a.st_prop[i] == 0 && ll_y - ll_y == 0.0;              // status word clean, log density finite
    for (int v = 0; v < a.F && ok; ++v) {
        const double y = stretch_coord(a, m, v);
        ok = y >= a.lo[v] && y <= a.hi[v];
    }
    if (ok) {
        const double q = __dsub_rn(__dadd_rn(__dmul_rn((double)(a.F - 1), log(m.z)), ll_y), ll_x);
        ok = log(m.u_a) < q;
    }
    double llw = ll_x;
    if (ok) {
        // (the partner sits in the other half, which no thread of this launch writes)
        for (int v = 0; v < a.F; ++v) {
            const double y = stretch_coord(a, m, v);
            a.chain[w * a.F + v] = y;
            a.x[w * a.F + v] = y;
        }
        a.ll[w] = llw = ll_y;
        a.n_accepted[w] += 1;
    } else {
        for (int v = 0; v < a.F; ++v) a.chain[w * a.F + v] = a.x[w * a.F + v];
    }
    a.chain_ll[w] = llw;
}

}  // namespace
