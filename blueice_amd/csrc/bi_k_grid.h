// bi_k_grid.h -- the kernels of the gridded likelihood (bi_grid_reduce, bi_grid.h).  Translation unit tu_grid.hip.
//   k_grid_points   writes one chunk of a tensor-product grid into the layouts the resident planner reads, with the points'
//                   additive terms p (priors at the nodes) and q (log quadrature weights of the reduced variables)
//   k_grid_reduce   folds the chunk's result vector into the per-cell state in HBM: an online log-sum-exp of u = (ll + p) + q
//                   and the maximum of t = ll + p with the smallest index that attains it
//   k_grid_init / k_grid_finish   the state's start, and log_marginal / profile / argmax from it at the end
// A cell's points inside a chunk are reduced by ONE block (or one wave of it) in a fixed order -- lanes stride over the
// segment, the wave folds with shuffles, the block's waves through LDS, and one lane folds the result into the state the
// earlier chunks left -- and the chunks follow each other on the stream: no atomics, and the result of a call is bitwise
// reproducible for a given chunk size.
#pragma once

namespace {

// the partial result of a set of points of one cell
struct GridAcc {
    double m, s;        // max of u over the points with u > -inf, sum of exp(u - m); (-inf, 0): none
    double best;        // max of t; -inf: none
    int64_t arg;        // the smallest r attaining it; -1: none
    int64_t n_excl;
    int nan_flag;
};

__device__ __forceinline__ GridAcc grid_acc_empty() { return GridAcc{-__builtin_inf(), 0.0, -__builtin_inf(), -1, 0, 0}; }

// a + b (b's points may lie before or behind a's: ties go to the smaller index)
__device__ __forceinline__ GridAcc grid_acc_merge(const GridAcc& a, const GridAcc& b) {
    GridAcc r = a;
    if (b.m > a.m) {                               // (a.m = -inf: a.s = 0 and exp(-inf) = 0)
        r.s = a.s * exp(a.m - b.m) + b.s;
        r.m = b.m;
    } else if (b.m > -__builtin_inf()) {
        r.s = a.s + b.s * exp(b.m - a.m);
    }
    if (b.best > a.best || (b.best == a.best && b.arg >= 0 && b.arg < a.arg)) {
        r.best = b.best;
        r.arg = b.arg;
    }
    r.n_excl = a.n_excl + b.n_excl;
    r.nan_flag = a.nan_flag | b.nan_flag;
    return r;
}

__device__ __forceinline__ int64_t shfl_down_i64(int64_t v, int off) {
    return __double_as_longlong(__shfl_down(__longlong_as_double(v), off, 64));
}

__device__ __forceinline__ GridAcc grid_acc_wave(GridAcc v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        GridAcc o;
        o.m = __shfl_down(v.m, off, 64);
        o.s = __shfl_down(v.s, off, 64);
        o.best = __shfl_down(v.best, off, 64);
        o.arg = shfl_down_i64(v.arg, off);
        o.n_excl = shfl_down_i64(v.n_excl, off);
        o.nan_flag = __shfl_down(v.nan_flag, off, 64);
        v = grid_acc_merge(v, o);
    }
    return v;                                      // lane 0 holds the wave's result
}

__global__ __launch_bounds__(kThreads) void k_grid_points(const GridArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t g = a.g0 + i;
    double p = 0.0, q = 0.0;
    varmap_write_point(a, i, g / a.GK, [&](int j) {
        const int64_t at = a.node_off[j] + (g / a.stride[j]) % a.n_nodes[j];
        if (a.term) p = __dadd_rn(p, a.term[at]);
        if (a.logw && j >= a.n_keep) q = __dadd_rn(q, a.logw[at]);
        return a.nodes[at];
    });
    if (a.p) a.p[i] = p;
    if (a.q) a.q[i] = q;
}

__global__ __launch_bounds__(kThreads) void k_grid_init(const GridArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.cells) return;
    a.m[c] = -__builtin_inf();
    a.s[c] = 0.0;
    a.best[c] = -__builtin_inf();
    a.arg[c] = -1;
    a.n_excl[c] = 0;
    a.nan_flag[c] = 0;
}

// cpb = 1: block b works on cell cell0 + b with its four waves; cpb = 4: wave w of block b on cell cell0 + 4 b + w
__global__ __launch_bounds__(kThreads) void k_grid_reduce(const GridArgs a) {
    __shared__ GridAcc s_acc[kThreads / 64];
    const int wave = (int)threadIdx.x >> 6;
    const int lanes = a.cpb == 1 ? kThreads : 64;                       // lanes that share a cell
    const int lane = a.cpb == 1 ? (int)threadIdx.x : ((int)threadIdx.x & 63);
    const int64_t local = (int64_t)blockIdx.x * a.cpb + (a.cpb == 1 ? 0 : wave);
    GridAcc v = grid_acc_empty();
    int64_t cell = -1;
    if (local < a.n_cells) {
        cell = a.cell0 + local;
        // the cell's points inside the chunk, as indices into the chunk's vectors
        const int64_t first = cell * a.R, end = first + a.R;
        const int64_t lo = first > a.g0 ? first - a.g0 : 0, hi = end < a.g0 + a.n ? end - a.g0 : a.n;
        const int64_t r0 = a.g0 - cell * a.R;                            // r = i + r0
        for (int64_t i = lo + lane; i < hi; i += lanes) {
            const double ll = a.ll[i];
            const double p = a.p ? a.p[i] : 0.0;
            if ((a.st && a.st[i] != 0) || ll == -__builtin_inf() || p == -__builtin_inf()) {
                v.n_excl += 1;
                continue;
            }
            const double t = a.p ? __dadd_rn(ll, p) : ll;
            if (t != t) {
                v.nan_flag = 1;
                continue;
            }
            if (t > v.best) {                                            // (r ascends within a lane: the first one stays)
                v.best = t;
                v.arg = i + r0;
            }
            const double u = a.q ? __dadd_rn(t, a.q[i]) : t;
            if (u > v.m) {
                v.s = v.s * exp(v.m - u) + 1.0;
                v.m = u;
            } else if (u > -__builtin_inf()) {
                v.s += exp(u - v.m);
            }
        }
    }
    v = grid_acc_wave(v);
    if ((threadIdx.x & 63) == 0) s_acc[wave] = v;
    __syncthreads();
    if (cell < 0) return;
    if (a.cpb == 1) {
        if (threadIdx.x != 0) return;
        for (int w = 1; w < kThreads / 64; ++w) v = grid_acc_merge(v, s_acc[w]);
    } else {
        if ((threadIdx.x & 63) != 0) return;
        v = s_acc[wave];
    }
    // into the state the earlier chunks left (their points come before this chunk's)
    GridAcc old{a.m[cell], a.s[cell], a.best[cell], a.arg[cell], a.n_excl[cell], a.nan_flag[cell]};
    v = grid_acc_merge(old, v);
    a.m[cell] = v.m;
    a.s[cell] = v.s;
    a.best[cell] = v.best;
    a.arg[cell] = v.arg;
    a.n_excl[cell] = v.n_excl;
    a.nan_flag[cell] = v.nan_flag;
}

__global__ __launch_bounds__(kThreads) void k_grid_finish(const GridArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.cells) return;
    if (a.nan_flag[c]) {
        a.out_lm[c] = a.out_prof[c] = __builtin_nan("");
        a.out_arg[c] = -1;
        return;
    }
    a.out_lm[c] = a.s[c] > 0.0 ? a.m[c] + log(a.s[c]) : -__builtin_inf();
    a.out_prof[c] = a.best[c];
    a.out_arg[c] = a.arg[c];
}

}  // namespace
