// bi_k_sets.h -- k_morph_sets: the extended unbinned likelihood of work items that each have their OWN event set
// (translation unit tu_morph.hip, behind bi_k_morph.h).
#pragma once

#include "bi_k_item.h"

namespace {

// An unbinned context can hold T event sets side by side on the event axis (include/blueice_hip.h, bi_score_event_sets):
// set t is columns [first_t, first_t + N_t) of every row.  A fit ensemble is P problems, each at its own parameter point
// and with its own set, so the items of a launch share no pass over the rows: blockIdx.y = item, its row offsets already
// start at its set's first column (even: the double2 loads stay aligned) and item_cnt[item] is N_t.  The grid is sized by
// the longest segment; block x of an item walks tiles x, x + gridDim.x, ... of that item's segment alone, and a block that
// lands past its item's end posts a zero and leaves without a load.  The per-tile work is morph_tiles itself with B = N_t
// -- MODE 2 (G = 1: the value) or MODE 3 (value + G - 1 gradient columns), so the nan-skipping sum over sources, the
// outlier clamp and the checked / fast logarithm are the single-set kernels' own, instruction for instruction; the row
// loop keeps eight 16-byte loads in flight per lane, which is what a toy of 10^3 .. 10^4 events (latency, not bandwidth)
// needs.  Partials go to partial[item][block][g] for k_finish, as k_morph_reduce writes them (item_reduce_store, bi_k_item.h).
template <int G, int MODE>
__global__ __launch_bounds__(kThreads) void k_morph_sets(LaunchArgs a) {
    const int item = blockIdx.y;
    const int64_t n_ev = a.item_cnt[item];
    const int n_tiles = (int)((n_ev + kTile - 1) / kTile);
    const int64_t o = ((int64_t)item * gridDim.x + blockIdx.x) * G;
    if ((int)blockIdx.x >= n_tiles) {
        if (threadIdx.x < G) { a.partial[o + threadIdx.x] = 0.0; a.pflags[o + threadIdx.x] = 0u; }
        return;
    }
    const int NS = a.n0;
    LaunchArgs b = a;
    b.B = n_ev;            // the mask of the segment's last tile
    b.chunks = 1;

    double sum[G];
    unsigned flg[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { sum[g] = 0.0; flg[g] = 0u; }
    morph_tiles<G, false, false, MODE>(b, a.rowoff + (int64_t)item * NS, a.coef + (int64_t)item * NS * G, nullptr, a.ps, nullptr, n_tiles,
                                       (int)blockIdx.x, (int)gridDim.x, sum, flg);

    item_reduce_store(sum, item, a.partial, a.pflags);
}

}  // namespace
