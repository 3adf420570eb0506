// bi_k_item.h -- the device skeleton of the per-point work-item kernels (device code only; included by the kernel headers that
// use it): blockIdx.y = item, blockIdx.x strides over the item's 512-bin tiles, every thread keeps its sums in registers, the
// block posts one partial per result slot and k_finish adds the blocks.  What a kernel adds is its prologue pointers and its
// per-bin mathematics.  The host half of the same paths is bi_items.h.
//     ItemTiles            the XCD-aware tile walk of one work item
//     ListTiles            ... with the item's own number of blocks as its stride (k_sourcewise_nonempty, k_sourcewise_events)
//     item_columns         the G coefficient columns of one bin (HessArgs kernels, one bin in flight per thread)
//     item_reduce_store    the block reduction in its fixed order and the store of the block's partials
//     item_chain           the single-column expectation sum_k a_k row_k[b]
#pragma once

namespace {

// XCD-aware tile order: with 8 chunks block b -- dispatched to XCD b % 8 -- streams the b % 8-th contiguous region of
// every row instead of every 8th tile (measured +6 % on the 113-stream BB pass, +1 % on C2); short rows keep the
// plain order, where the padded chunk count would cost some blocks a second tile.  The trip count is the same for a whole
// block.
//     for (ItemTiles w(a, n_tiles); w.more(); w.step()) { const int tile = w.tile(); if (tile < 0) continue; ... }
struct ItemTiles {
    int n_tiles, chunks, per_chunk, lt;
    template <class Args>      // LaunchArgs or HessArgs: a.chunks is what the host asks for
    __device__ __forceinline__ ItemTiles(const Args& a, int n_tiles)
        : n_tiles(n_tiles), chunks((a.chunks > 1 && n_tiles >= 64 * a.chunks) ? a.chunks : 1),
          per_chunk((n_tiles + chunks - 1) / chunks), lt(blockIdx.x) {}
    __device__ __forceinline__ bool more() const { return lt < per_chunk * chunks; }
    __device__ __forceinline__ void step() { lt += gridDim.x; }
    __device__ __forceinline__ int tile() const {       // -1: this step is past the end of a ragged last chunk
        const int t = chunks > 1 ? (lt % chunks) * per_chunk + lt / chunks : lt;
        return t < n_tiles ? t : -1;
    }
};

// ItemTiles with the item's own stride: block x of nbx takes the steps x, x + nbx, ...
struct ListTiles : ItemTiles {
    int nbx;
    template <class Args>
    __device__ __forceinline__ ListTiles(const Args& a, int n_tiles, int nbx_) : ItemTiles(a, n_tiles), nbx(nbx_) {}
    __device__ __forceinline__ void step() { lt += nbx; }
};

// acc[g] = sum_k coef[k][g] row_k[bin], k ascending from 0.0 with one fma per row: column 0 is item_chain's mu_b bit for bit
// (Args: HessArgs, or k_morph_coarse_jac's CoarseArgs -- a.ps and a.NS are what is read)
template <int G, bool NT, class Args>
__device__ __forceinline__ void item_columns(const Args& a, const int64_t* __restrict__ rowoff, const double* __restrict__ coef,
                                             int64_t bin, double (&acc)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.0;
#pragma unroll 4
    for (int k = 0; k < a.NS; ++k) {
        const double* p = a.ps + rowoff[k] + bin;
        const double v = NT ? __builtin_nontemporal_load(p) : *p;
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = fma(coef[k * G + g], v, acc[g]);
    }
}

// The block reduction: the lanes' shuffle tree (wave_sum), then waves 0, 1, 2, 3 in order -- this fixed order is what makes
// a repeated call bitwise identical.  The block's slots go to partial[(item * gridDim.x + blockIdx.x) * NSL + j] with
// pflags = 0, for k_finish.
template <int N, int NSL>
__device__ __forceinline__ void item_wave_sums(const double (&v)[N], double (&s_sum)[kThreads / 64][NSL], int first) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double s = wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6][first + j] = s;
    }
}

template <int NSL>
__device__ __forceinline__ void item_store(const double (&s_sum)[kThreads / 64][NSL], int item, double* __restrict__ partial,
                                           unsigned* __restrict__ pflags) {
    static_assert(NSL <= kThreads, "one thread per result slot");
    __syncthreads();
    if (threadIdx.x < NSL) {
        double s = s_sum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) s += s_sum[w][threadIdx.x];
        const int64_t o = ((int64_t)item * gridDim.x + blockIdx.x) * NSL + threadIdx.x;
        partial[o] = s;
        pflags[o] = 0u;
    }
}

// G sums
template <int G>
__device__ __forceinline__ void item_reduce_store(const double (&sum)[G], int item, double* __restrict__ partial,
                                                  unsigned* __restrict__ pflags) {
    __shared__ double s_sum[kThreads / 64][G];
    item_wave_sums(sum, s_sum, 0);
    item_store(s_sum, item, partial, pflags);
}

// G sums, then NP Gram pairs
template <int G, int NP>
__device__ __forceinline__ void item_reduce_store(const double (&sum)[G], const double (&gram)[NP], int item,
                                                  double* __restrict__ partial, unsigned* __restrict__ pflags) {
    __shared__ double s_sum[kThreads / 64][G + NP];
    item_wave_sums(sum, s_sum, 0);
    item_wave_sums(gram, s_sum, G);
    item_store(s_sum, item, partial, pflags);
}

// mu = sum_k a_k ps[rowoff[k] + at], k = k0, k0 + step, ... < NS from 0.0 with one fma per row (every row: k0 = 0, step = 1;
// the rows of source s alone: k0 = s, step = S).  The one definition of the expectation's bits: k_morph_expect, k_real_expect
// and k_morph_coarse call it, so an Asimov dataset, the expectation and its coarse view agree bit for bit (UNROLL: the row
// loads in flight, which does not touch the order).
template <int UNROLL>
__device__ __forceinline__ double item_chain(const double* __restrict__ coef, const int64_t* __restrict__ rowoff,
                                             const double* __restrict__ ps, int64_t at, int k0, int NS, int step) {
    double mu = 0.0;
#pragma unroll UNROLL
    for (int k = k0; k < NS; k += step) mu = fma(coef[k], ps[rowoff[k] + at], mu);
    return mu;
}

}  // namespace
