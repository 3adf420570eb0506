// bi_k_toys.h -- the toy-MC EVALUATION kernels (device code only; translation unit tu_toys.hip): one parameter point, or the
// points of a group of passes, against many datasets.  The host half is bi_toys.h.
//     k_csr_tile_offsets, k_tm_counts, k_tm_scatter      the tile-major copy of the non-empty-bin lists
//     k_morph_logmu, k_morph_logmu_desc, k_morph_logmu_multi   log mu of one point / of the points of a group of passes
//     k_dataset_dot, k_dataset_dot_csr                   the row kernels (dense counts, dataset-major lists)
//     k_dataset_dot_tiled, k_dataset_dot_multi           the tile-major lists against log mu tiles staged in LDS
//     k_dataset_finish, k_dataset_finish_tiled, k_dataset_finish_multi, k_fill_rows
// The finish kernels share mu_partial_sum and publish_when_last.  The constants and argument structs the host half needs as well
// (kDotTile, kDotTileMulti, kDotPad, kDotGroup, kPartBlock, PointDesc, MuTotals) are in bi_dev_common.h.
#pragma once

namespace {

// toy-MC, CSR form: for dataset t: sum_j xlogy(n_j, mu[idx_j]); one block per dataset
__global__ __launch_bounds__(kThreads) void k_dataset_dot_csr(const int32_t* __restrict__ nz_idx,
                                                              const double* __restrict__ nz_n,
                                                              const int64_t* __restrict__ nz_off,
                                                              const double* __restrict__ logmu, int64_t t0,
                                                              double* __restrict__ partial) {
    const int64_t t = t0 + blockIdx.x;
    const int64_t lo = nz_off[t], hi = nz_off[t + 1];
    double s = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) {
        const double n = nz_n[j];
        double term = n * logmu[nz_idx[j]];
        if (n != n) term = __builtin_nan("");
        else if (n < 0.0 || n != floor(n)) term = -__builtin_inf();
        s += term;
    }
    __shared__ double sh[kThreads / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sh[0];
        for (int w = 1; w < kThreads / 64; ++w) r += sh[w];
        partial[blockIdx.x] = r;
    }
}

// ---- toy-MC, CSR form, bin tiles staged through LDS --------------------------------------------------------------
// The row kernel above gathers log mu[idx] from an 8 MB table with one 8-byte element per cache line: at C2 (10^4
// datasets x ~9 400 non-empty bins) that gather, not HBM, sets its 0.54 ms.  Here a block owns a TILE of kDotTile bins:
// it stages that part of log mu in LDS once and walks the entries of many datasets that fall into the tile -- a
// dataset's non-empty-bin list is sorted by bin, so they are one contiguous run, found through a per-dataset table
// of tile offsets (k_csr_tile_offsets, built once per data upload).  One wave per (dataset, tile); its sum goes to
// partial[dataset][tile], which k_dataset_finish adds up in tile order: fixed order, reproducible.
__global__ __launch_bounds__(kThreads) void k_csr_tile_offsets(const int32_t* __restrict__ nz_idx, const int64_t* __restrict__ nz_off,
                                                               int n_tl, int32_t* __restrict__ tile_off /*[T][n_tl + 1]*/,
                                                               int tile_shift /* log2 of the bins per tile */) {
    const int64_t t = blockIdx.x;
    const int64_t lo = nz_off[t], hi = nz_off[t + 1];
    int32_t* __restrict__ dst = tile_off + t * (n_tl + 1);
    if (hi == lo) {
        for (int tl = threadIdx.x; tl <= n_tl; tl += kThreads) dst[tl] = 0;
        return;
    }
    for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) {
        const int cur = nz_idx[j] >> tile_shift;
        const int prev = j > lo ? nz_idx[j - 1] >> tile_shift : -1;
        for (int tl = prev + 1; tl <= cur; ++tl) dst[tl] = (int32_t)(j - lo);     // first entry at or beyond the start of tile tl
        if (j == hi - 1)
            for (int tl = cur + 1; tl <= n_tl; ++tl) dst[tl] = (int32_t)(hi - lo);
    }
}

// Tile-major copy of the non-empty-bin lists: all entries of bin tile 0 (dataset 0, 1, ...), then tile 1, ... -- the
// block that owns a tile reads ONE contiguous stream instead of a sub-kilobyte run per dataset scattered over the
// dataset-major lists (which held the first tiled version at 2.6 TB/s).  An entry is 4 bytes: the byte offset of the bin
// within the staged tile (bits 3..16: bin * 8) and the count (15 bits, from bit 17), so that the kernel gets the LDS
// address with one AND and the count with one shift; data whose counts do not fit (or are not positive integers) keep
// the row kernel.  Every (dataset, tile) run is padded to a multiple of FOUR entries with the padding entry (bins per
// tile << 3, build_tile_major) -- count 0, and the
// offset of an extra LDS slot behind the tile that holds 0.0, never log mu = -inf -- so that a lane's 16-byte load is
// wholly inside its run or wholly outside it (one test per load, not per entry) and every load is 16-byte aligned.
// Round 4, measured: with the entry loads taken out the kernel runs in 24 us instead of 86 -- the ENTRY STREAM is its time
// (376 MB at C2: 54 us of HBM at best), neither the LDS gathers nor the arithmetic.  So where every count is at most 7 -- toys
// of sparse expectations: all of them -- an entry is TWO bytes: bin * 8 (the LDS byte offset, bits 3..15) | count (bits
// 0..2), eight entries per 16-byte load, runs padded to multiples of eight with 0 (count 0: the term is dropped by a select,
// there is no room for the offset of the extra slot).  Data with a larger count anywhere keeps the 4-byte entries.
__global__ void k_tm_counts(const int32_t* __restrict__ tile_off, int64_t T, int n_tl, int64_t* __restrict__ cnt /*[n_tl * T + 1]*/,
                            int group /* entries per 16-byte load: 4 or 8 */) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > (int64_t)n_tl * T) return;
    if (i == (int64_t)n_tl * T) { cnt[i] = 0; return; }
    const int64_t tl = i / T, t = i % T;
    const int32_t* __restrict__ o = tile_off + t * (n_tl + 1) + tl;
    cnt[i] = (o[1] - o[0] + group - 1) & ~(group - 1);     // (the run's padded length: the list is pre-filled with padding entries)
}

template <typename ENTRY>
__global__ __launch_bounds__(kThreads) void k_tm_scatter(const int32_t* __restrict__ nz_idx, const double* __restrict__ nz_n,
                                                         const int64_t* __restrict__ nz_off, const int32_t* __restrict__ tile_off,
                                                         int64_t T, int n_tl, const int64_t* __restrict__ tm_off,
                                                         ENTRY* __restrict__ tm_entries, int* __restrict__ bad, int tile_shift) {
    const int64_t t = blockIdx.x;
    const int64_t lo = nz_off[t], hi = nz_off[t + 1];
    const int32_t* __restrict__ o = tile_off + t * (n_tl + 1);
    bool any_bad = false;
    for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) {
        const int idx = nz_idx[j];
        const double n = nz_n[j];
        const int tl = idx >> tile_shift;
        if constexpr (sizeof(ENTRY) == 2) {
            if (!(n >= 1.0 && n <= 7.0 && n == floor(n))) any_bad = true;
            tm_entries[tm_off[(int64_t)tl * T + t] + (j - lo - o[tl])] = (ENTRY)(((uint32_t)(idx - (tl << tile_shift)) << 3) | ((uint32_t)n & 7u));
        } else {
            if (!(n >= 1.0 && n < 32768.0 && n == floor(n))) any_bad = true;
            tm_entries[tm_off[(int64_t)tl * T + t] + (j - lo - o[tl])] = ((uint32_t)(idx - (tl << tile_shift)) << 3) | ((uint32_t)n << 17);
        }
    }
    if (any_bad) atomicOr(bad, 1);
}

// 1024 threads: 16 waves share one staged tile; every 16-lane row of a wave takes its own dataset, so a wave has four
// (dataset, tile) runs in flight and a block 64.  The runs are short (~80 entries at C2) and each starts with a chain of
// dependent loads (offsets -> entries -> LDS): with one run after the other per row the kernel sat at 134 us for 0.4 GB
// (3 TB/s), every wave waiting a full memory latency two or three times per run.  Now a row keeps the loads of THREE
// runs in flight (ring buffers in registers, the loop unrolled over the ring so that nothing is copied and nothing
// newer than what it needs is waited for): offsets four runs ahead, entries two runs ahead.  Every load is
// unconditional -- a run behind the row's last one is the last one again (requested, never stored), an entry load
// reads up to kDotPad entries past its run (the lists are padded by that much) and its 4-entry sum is dropped afterwards
// (runs are whole 16-byte groups: round 4) -- because a branch around a load makes the compiler wait for ALL outstanding
// loads.  Index arithmetic is 32-bit, relative to the
// block's first entry (the launch keeps a block below 2^31 entries).  Per lane the entries are added in ascending
// order with fma, four at a time (one 16-byte load), the groups' sums then in ascending order: a fixed order, independent of
// the launch geometry.
typedef uint32_t bi_uint4 __attribute__((ext_vector_type(4)));
constexpr int kDotThreads = 1024;
#ifndef BI_DOT_DEPTH
#define BI_DOT_DEPTH 2
#endif

// sum over the L lanes of a group inside a 16-lane DPP row (L = 16, or 8: groups start at lanes 0 and 8) on the cross-lane
// data path; every lane of the group ends up with the total.  L = 16: four rotate-and-add steps; L = 8: the mirror image
// within the half row (lane i <-> 7 - i), then the two exchanges within quads -- three steps, in a fixed order.
template <int L>
__device__ __forceinline__ double row_group_sum(double v) {
#define BI_DPP_ADD(CTRL)                                                                                           \
    do {                                                                                                           \
        const unsigned long long u = __double_as_longlong(v);                                                      \
        const unsigned lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, true);                \
        const unsigned hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, true);        \
        v += __longlong_as_double(((unsigned long long)hi << 32) | lo);                                            \
    } while (0)
    if constexpr (L == 16) {
        BI_DPP_ADD(0x120 + 8);        // row_ror:8
        BI_DPP_ADD(0x120 + 4);
        BI_DPP_ADD(0x120 + 2);
        BI_DPP_ADD(0x120 + 1);
    } else if constexpr (L == 8) {
        BI_DPP_ADD(0x141);            // row_half_mirror
        BI_DPP_ADD(0xB1);             // quad_perm:[1,0,3,2]
        BI_DPP_ADD(0x4E);             // quad_perm:[2,3,0,1]
    } else if constexpr (L == 4) {
        BI_DPP_ADD(0xB1);             // quad_perm:[1,0,3,2]
        BI_DPP_ADD(0x4E);             // quad_perm:[2,3,0,1]
    } else {
        static_assert(L == 2, "groups of 2, 4, 8 or 16 lanes");
        BI_DPP_ADD(0xB1);             // quad_perm:[1,0,3,2]
    }
#undef BI_DPP_ADD
    return v;
}

// L lanes per (dataset, tile) run, AHEAD 16-byte loads per lane requested up front: 4 L AHEAD entry slots per run.
// <16, 2>: 128 slots, 64 runs in flight per block (round 3).  <8, 3>: 96 slots -- a run at C2 is ~76 entries, so 79 % of the
// slots carry an entry instead of 59 % --, 128 runs in flight per block, three rotate-and-add steps instead of four (round 4).
// W: bytes per entry (4, or 2: counts up to 7) -- 16 / W entries per 16-byte load, (16 / W) L AHEAD slots per run.
template <int L, int AHEAD, int W = 4>
__global__ __launch_bounds__(kDotThreads) void k_dataset_dot_tiled(const void* __restrict__ tm_entries_v,
                                                                   const int64_t* __restrict__ tm_off, int64_t T, int n_tl,
                                                                   const double* __restrict__ logmu, int64_t B, int64_t t0,
                                                                   int64_t n, double* __restrict__ partial /*[n_tl][n]*/) {
    typedef typename std::conditional<W == 2, uint16_t, uint32_t>::type entry_t;
    constexpr int EPL = 16 / W;                                        // entries per lane and load
    static_assert(EPL * L * AHEAD + 16 <= kDotPad, "the lists' padding must cover the read-ahead");
    const entry_t* __restrict__ tm_entries = static_cast<const entry_t*>(tm_entries_v);
    __shared__ double s_mu[kDotTile + 1];                              // (+ the slot of the padding entries: 0.0)
    const int tl = blockIdx.x;
    const int64_t bin0 = (int64_t)tl * kDotTile;
    const int row = threadIdx.x / L, gl = threadIdx.x % L;             // kDotThreads / L rows of L lanes
    const int per = (int)((n + gridDim.y - 1) / gridDim.y);
    const int c0u = (int)blockIdx.y * per, c1 = min((int)n, c0u + per);
    const int c0 = min(c0u, (int)n - 1);                               // (clamped: a block without datasets still loads validly)
    const int64_t* __restrict__ off = tm_off + (int64_t)tl * T + t0;
    const int64_t base = off[c0];                                  // block-uniform: the entries of this block start here
    const entry_t* __restrict__ ent = tm_entries + base;
    const uint32_t* __restrict__ off32 = reinterpret_cast<const uint32_t*>(off);   // low words: all a block-relative index needs
    const uint32_t base32 = (uint32_t)base;
    constexpr int kStep = kDotThreads / L, kAhead = AHEAD, kDepth = BI_DOT_DEPTH, kRing = 2 * (kDepth + 1);   // entries kDepth runs ahead, offsets 2 kDepth; the ring a multiple of the entry buffers
    const int q_last = max(c0, c1 - 1);
    // (a step only ISSUES loads into the rings; whatever touches a loaded value -- the subtraction of the base, the mask
    //  of the entries past the run's end -- happens in the step that consumes it, two or four steps later: the compiler
    //  waits where a value is first used, and it does not move that use out of the step it was written in)
    auto load_offsets = [&](int q, uint32_t& ra, uint32_t& rb) {
        const int qc = min(q, q_last);
        ra = off32[2 * qc];
        rb = off32[2 * qc + 2];
    };
    // (a lane takes EPL consecutive entries per load: a group's load covers 16 L contiguous bytes of its run)
    auto load_entries = [&](uint32_t ra, bi_uint4 (&e)[kAhead]) {
        const entry_t* __restrict__ p = ent + (int)(ra - base32) + EPL * gl;
#pragma unroll
        for (int k = 0; k < kAhead; ++k) __builtin_memcpy(&e[k], p + EPL * L * k, 16);   // (16-byte load, 16-byte aligned: runs are whole groups)
    };
    bi_uint4 E[kDepth + 1][kAhead];
    uint32_t RA[kRing], RB[kRing];
    const int q0 = c0 + row;
    // the pipeline's first requests go out before the tile is staged: their latency passes under the staging
#pragma unroll
    for (int u = 0; u < 2 * kDepth; ++u) load_offsets(q0 + u * kStep, RA[u], RB[u]);
    {   // (all loads first, addresses clamped instead of predicated: eight loads in flight per thread, not one at a time)
        double v[kDotTile / kDotThreads];
#pragma unroll
        for (int k = 0; k < kDotTile / kDotThreads; ++k) v[k] = logmu[min(bin0 + threadIdx.x + k * kDotThreads, B - 1)];
#pragma unroll
        for (int k = 0; k < kDotTile / kDotThreads; ++k)
            s_mu[threadIdx.x + k * kDotThreads] = bin0 + threadIdx.x + k * kDotThreads < B ? v[k] : 0.0;
        if (threadIdx.x == 0) s_mu[kDotTile] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < kDepth; ++u) load_entries(RA[u], E[u]);
    __syncthreads();
    if (c0u >= c1) return;
    const int n_iter = (c1 - c0 + kStep - 1) / kStep;             // block-uniform: rows past their last run idle along
    for (int it = 0; it < n_iter; it += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; ++u) {
            if (it + u < n_iter) {                               // (scalar condition)
                const int q = q0 + (it + u) * kStep;
                load_offsets(q + 2 * kDepth * kStep, RA[(u + 2 * kDepth) % kRing], RB[(u + 2 * kDepth) % kRing]);
                load_entries(RA[(u + kDepth) % kRing], E[(u + kDepth) % (kDepth + 1)]);
                __builtin_amdgcn_sched_barrier(0);               // the requests go out BEFORE this step's arithmetic, not after it
                const bi_uint4 (&e)[kAhead] = E[u % (kDepth + 1)];
                const int a = (int)(RA[u % kRing] - base32), b = (int)(RB[u % kRing] - base32);
                const int len = b - a - EPL * gl;                // (padded) entries of the run from this lane's first on
                double s = 0.0;
                if constexpr (W == 4) {
                    double lm[4 * kAhead];
#define BI_TM_LOG(x) (*reinterpret_cast<const double*>(reinterpret_cast<const char*>(s_mu) + ((x) & 0x1FFF8u)))
#pragma unroll
                    for (int k = 0; k < 4 * kAhead; ++k) lm[k] = BI_TM_LOG(e[k >> 2][k & 3]);      // LDS reads in flight together
#pragma unroll
                    for (int g = 0; g < kAhead; ++g) {
                        double sg = (double)(e[g][0] >> 17) * lm[4 * g];
#pragma unroll
                        for (int k = 1; k < 4; ++k) sg = __builtin_fma((double)(e[g][k] >> 17), lm[4 * g + k], sg);
                        s += 4 * L * g < len ? sg : 0.0;         // (a load behind the run's end read other runs' entries: dropped whole)
                    }
                    for (int j = a + gl + 4 * L * kAhead; j < b; j += L) {                  // (runs beyond 4 L AHEAD entries)
                        const uint32_t x = ent[j];
                        s = __builtin_fma((double)(x >> 17), BI_TM_LOG(x), s);
                    }
#undef BI_TM_LOG
                } else {
                    // two entries per word: LDS byte offset = entry & 0xFFF8, count = entry & 7 (0 = padding: its term is dropped,
                    // whatever log mu of bin 0 is)
                    double lm[8 * kAhead];
#define BI_TM_LOG16(x) (*reinterpret_cast<const double*>(reinterpret_cast<const char*>(s_mu) + ((x) & 0xFFF8u)))
#pragma unroll
                    for (int k = 0; k < 4 * kAhead; ++k) {
                        const uint32_t x = e[k >> 2][k & 3];
                        lm[2 * k] = BI_TM_LOG16(x);
                        lm[2 * k + 1] = BI_TM_LOG16(x >> 16);
                    }
#pragma unroll
                    for (int g = 0; g < kAhead; ++g) {
                        double sg = 0.0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t x = e[g][k];
                            const uint32_t n0 = x & 7u, n1 = (x >> 16) & 7u;
                            sg = __builtin_fma((double)n0, n0 ? lm[8 * g + 2 * k] : 0.0, sg);
                            sg = __builtin_fma((double)n1, n1 ? lm[8 * g + 2 * k + 1] : 0.0, sg);
                        }
                        s += 8 * L * g < len ? sg : 0.0;         // (a load behind the run's end read other runs' entries: dropped whole)
                    }
                    for (int j = a + gl + 8 * L * kAhead; j < b; j += L) {                  // (runs beyond 8 L AHEAD entries)
                        const uint32_t x = ent[j];
                        const uint32_t n0 = x & 7u;
                        s = __builtin_fma((double)n0, n0 ? BI_TM_LOG16(x) : 0.0, s);
                    }
#undef BI_TM_LOG16
                }
                s = row_group_sum<L>(s);
                if (gl == 0 && q < c1) partial[(int64_t)tl * n + q] = s;
            }
        }
    }
}

// ---- toy-MC form: one parameter point, many datasets --------------------------------------
// pass 1: mu_b -> logmu[b] (log mu, or -inf for mu == 0, or nan for invalid mu), partial sum mu
__device__ __forceinline__ void morph_logmu_body(const LaunchArgs& a, const int64_t* __restrict__ rowoff, const double* __restrict__ coef,
                                                 double* __restrict__ logmu, int store_mu) {
    double sum = 0.0;
    unsigned bad = 0u;
    log_table_load();
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t bin0 = (int64_t)tile * kTile + threadIdx.x * kBinsPerThread;
        double m0 = 0.0, m1 = 0.0;
#pragma unroll 8
        for (int k = 0; k < a.n0; ++k) {
            const double2 v = *reinterpret_cast<const double2*>(a.ps + rowoff[k] + bin0);
            const double c = coef[k];
            m0 = fma(c, v.x, m0);
            m1 = fma(c, v.y, m1);
        }
        double2 l;
        if (store_mu) {  // toy generation wants the expectation itself
            l.x = m0;
            l.y = m1;
        } else {
            l.x = (m0 >= 0.0) ? bin_log(m0) : __builtin_nan("");
            l.y = (m1 >= 0.0) ? bin_log(m1) : __builtin_nan("");
        }
        if (!(m0 >= 0.0) || !(m1 >= 0.0)) bad = 1u;
        *reinterpret_cast<double2*>(logmu + bin0) = l;
        sum += m0 + m1;
    }
    __shared__ double sh[kThreads / 64];
    __shared__ unsigned shf[kThreads / 64];
    sum = wave_sum(sum);
    bad = wave_or(bad);
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = sum; shf[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
        unsigned f = shf[0];
        for (int w = 1; w < kThreads / 64; ++w) { t += sh[w]; f |= shf[w]; }
        a.partial[blockIdx.x] = t;
        a.pflags[blockIdx.x] = f;
    }
}

__global__ __launch_bounds__(kThreads) void k_morph_logmu(LaunchArgs a, double* __restrict__ logmu, int store_mu) {
    morph_logmu_body(a, a.rowoff, a.coef, logmu, store_mu);
}

// The point's descriptors in the kernel arguments (PointDesc: up to kMaxSingleStreams streams): a toy-MC call is ONE point, and
// a host-to-device copy of its 512 bytes ahead of the launch costs more than the launch (10 ... 15 us on this runtime).
__global__ __launch_bounds__(kThreads) void k_morph_logmu_desc(LaunchArgs a, PointDesc d, double* __restrict__ logmu, int store_mu) {
    morph_logmu_body(a, d.rowoff, d.coef, logmu, store_mu);
}

// pass 2: for dataset t: sum_b xlogy(n_tb, mu_b).  blockIdx.y = group of kDotGroup datasets, x strides tiles: the
// log mu tile is loaded once per group (it stays in L2 / Infinity Cache: 8 MB), the counts rows stream through once
// with the nontemporal hint; XCD-aware tile order as in morph_tiles.
__device__ __forceinline__ double xlogy_term(double n, double l) {
    double t = (n > 0.0) ? n * l : 0.0;
    if (n != n) t = __builtin_nan("");
    else if (n < 0.0 || n != floor(n)) t = -__builtin_inf();
    return t;
}

__global__ __launch_bounds__(kThreads) void k_dataset_dot(const double* __restrict__ counts,
                                                          const double* __restrict__ logmu, int64_t Bp, int n_tiles,
                                                          int64_t t0, int64_t n_sets, double* __restrict__ partial) {
    const int64_t d0 = (int64_t)blockIdx.y * kDotGroup;
    const double* __restrict__ c[kDotGroup];
#pragma unroll
    for (int g = 0; g < kDotGroup; ++g) c[g] = counts + (t0 + min(d0 + g, n_sets - 1)) * Bp;   // tail group: repeats the last row
    double s[kDotGroup];
#pragma unroll
    for (int g = 0; g < kDotGroup; ++g) s[g] = 0.0;
    const int chunks = n_tiles >= 64 * 8 ? 8 : 1;
    const int per_chunk = (n_tiles + chunks - 1) / chunks;
    for (int lt = blockIdx.x; lt < per_chunk * chunks; lt += gridDim.x) {
        const int tile = chunks > 1 ? (lt % chunks) * per_chunk + lt / chunks : lt;
        if (tile >= n_tiles) continue;
        const int64_t bin0 = (int64_t)tile * kTile + threadIdx.x * kBinsPerThread;
        double2 n[kDotGroup];
#pragma unroll
        for (int g = 0; g < kDotGroup; ++g) n[g] = stream_load<true>(c[g] + bin0);
        const double2 l = *reinterpret_cast<const double2*>(logmu + bin0);
#pragma unroll
        for (int g = 0; g < kDotGroup; ++g) s[g] += xlogy_term(n[g].x, l.x) + xlogy_term(n[g].y, l.y);
    }
    __shared__ double sh[kThreads / 64][kDotGroup];
#pragma unroll
    for (int g = 0; g < kDotGroup; ++g) {
        const double w = wave_sum(s[g]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][g] = w;
    }
    __syncthreads();
    if (threadIdx.x < kDotGroup && d0 + threadIdx.x < n_sets) {
        double t = sh[0][threadIdx.x];
        for (int w = 1; w < kThreads / 64; ++w) t += sh[w][threadIdx.x];
        partial[(d0 + threadIdx.x) * gridDim.x + blockIdx.x] = t;
    }
}

// this thread's share of the mu partials of pass 1 and of their flags, b = threadIdx.x, + kThreads, ... (four loads in flight
// per thread: every block of a finish kernel repeats this sum before it can start on its datasets); the caller adds the
// threads up (wave_sum / wave_or, then the waves in order)
__device__ __forceinline__ void mu_partial_sum(const double* __restrict__ mu_partial, const unsigned* __restrict__ mu_flags, int nmu,
                                               double& m, unsigned& f) {
    double m4[4] = {0.0, 0.0, 0.0, 0.0};
    int b = threadIdx.x;
    for (; b + 3 * kThreads < nmu; b += 4 * kThreads) {
        double v[4];
        unsigned g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = mu_partial[b + k * kThreads]; g[k] = mu_flags[b + k * kThreads]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { m4[k] += v[k]; f |= g[k]; }
    }
    for (; b < nmu; b += kThreads) { m4[0] += mu_partial[b]; f |= mu_flags[b]; }
    m = (m4[0] + m4[1]) + (m4[2] + m4[3]);
}

// Called by the first wave of every block of a finish kernel once the block's results are written: the block is counted, and
// the one of the n_blocks that is counted last publishes `seq` in pinned host memory with a system-scope release (the host
// polls the word instead of synchronising the stream: wait_word, bi_wait.h) and leaves the counter at zero for the next call.
__device__ __forceinline__ void publish_when_last(unsigned* __restrict__ blocks_done, unsigned n_blocks, unsigned long long* done,
                                                  unsigned long long seq) {
    __threadfence_system();                            // this wave's results have left before the block is counted
    if (threadIdx.x == 0) {
        const unsigned before = __hip_atomic_fetch_add(blocks_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before == n_blocks - 1) {
            __hip_atomic_store(blocks_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (ready for the next call)
            __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// out[t] = sum_blocks partial[t][:] - summu - lgsum[t0 + t]   (nan if any mu invalid).  256 threads per block: the
// block first sums the mu partials of pass 1 together (fixed tree), then every thread finishes one dataset.
// (partial[t * t_stride + b * b_stride]: dataset-major from the row kernels, block-major from the tiled one, whose 123
// partials per dataset would otherwise be read with a stride of 123 doubles between neighbouring threads)
__global__ __launch_bounds__(kThreads) void k_dataset_finish(const double* __restrict__ partial, int nbx, int64_t t_stride, int64_t b_stride,
                                                             const double* __restrict__ mu_partial,
                                                             const unsigned* __restrict__ mu_flags, int nmu,
                                                             const double* __restrict__ lgsum, int64_t t0, int64_t n,
                                                             double* __restrict__ out) {
    __shared__ double sh[kThreads / 64];
    __shared__ unsigned shf[kThreads / 64];
    double m = 0.0;
    unsigned f = 0u;
    mu_partial_sum(mu_partial, mu_flags, nmu, m, f);
    m = wave_sum(m);
    f = wave_or(f);
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = m; shf[threadIdx.x >> 6] = f; }
    __syncthreads();
    m = sh[0];
    f = shf[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) { m += sh[w]; f |= shf[w]; }
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    // eight running sums: the loads of a thread do not wait for one another (123 block-major partials per dataset from
    // the tiled kernel are 123 trips to L2 otherwise); fixed order all the same
    const double* __restrict__ p = partial + t * t_stride;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int b = 0;
    for (; b + 7 < nbx; b += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(int64_t)(b + k) * b_stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += v[k];
    }
    for (; b < nbx; ++b) acc[0] += p[(int64_t)b * b_stride];
    const double s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    double r = (s - m) - lgsum[t0 + t];
    if (f) r = __builtin_nan("");
    out[t] = r;
}

// The finish of the tiled toy-MC pass, partial[tile][dataset] (block-major): 64 datasets per block, the tiles of a
// dataset split over the block's four waves (k_dataset_finish has one thread walk all ~123 tiles of its dataset, 16 trips
// to L2 one after the other on 40 blocks: 10 ... 15 us for 10^4 datasets; here 157 blocks and four trips).  Fixed order:
// a wave's range in steps of eight with eight running sums, then the four waves' sums ((0 + 1) + (2 + 3)).
// done != NULL: out is pinned host memory; the block that finishes last publishes `seq` there (publish_when_last) once every
// block's results are on their way.
__global__ __launch_bounds__(kThreads) void k_dataset_finish_tiled(const double* __restrict__ partial, int nbx,
                                                                   const double* __restrict__ mu_partial,
                                                                   const unsigned* __restrict__ mu_flags, int nmu,
                                                                   const double* __restrict__ lgsum, int64_t t0, int64_t n,
                                                                   double* __restrict__ out, unsigned* __restrict__ blocks_done,
                                                                   unsigned long long* done, unsigned long long seq) {
    static_assert(kThreads == 256, "four waves per block");
    __shared__ double sh[kThreads / 64];
    __shared__ unsigned shf[kThreads / 64];
    __shared__ double part[kThreads / 64][64];
    double m = 0.0;
    unsigned f = 0u;
    mu_partial_sum(mu_partial, mu_flags, nmu, m, f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const int per = (nbx + 3) / 4;
    const int b0 = wave * per, b1 = min(nbx, b0 + per);
    double s = 0.0;
    if (t < n) {
        const double* __restrict__ p = partial + t;
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int b = b0;
        for (; b + 7 < b1; b += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[(int64_t)(b + k) * n];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += v[k];
        }
        for (; b < b1; ++b) acc[0] += p[(int64_t)b * n];
        s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    part[wave][lane] = s;
    m = wave_sum(m);
    f = wave_or(f);
    if (lane == 0) { sh[wave] = m; shf[wave] = f; }
    __syncthreads();
    if (wave == 0 && t < n) {
        double mm = sh[0];
        unsigned ff = shf[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) { mm += sh[w]; ff |= shf[w]; }
        const double tot = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        double r = (tot - mm) - lgsum[t0 + t];
        if (ff) r = __builtin_nan("");
        out[t] = r;
    }
    if (!done) return;
    if (wave == 0) publish_when_last(blocks_done, gridDim.x, done, seq);
}

// ---- the toy-MC form over SEVERAL parameter points (bi_eval_datasets_points; the host half in bi_toys.h says what it replaces) ----
// (1) log mu of the points of a group of passes
// The table of a group is GC = (passes per group) x PP rows of Bp doubles, row = pass-in-group * PP + column-in-pass.
// blockIdx.y = work item = the points of ONE group that lie in ONE grid cell (1 .. GC of them: the rows of the cell's anchors are
// read once for all of them, across the passes of the group); blockIdx.x strides over the 512-bin tiles in the XCD-aware order
// of morph_tiles.  coef [items][NS][GC]: column g of the matrix is row g of the group's table, zero for the rows that belong to
// another item (another cell); meta [items][4] = {first row, number of rows, 0, 0}.  Same accumulation order over the streams as
// k_morph_logmu (fma, k ascending): the same log mu bits.
// partial / pflags [items][gridDim.x][GC]: sum_b mu_b and the "some mu is negative or nan" flag per row.
template <int GC, bool NT>
__global__ __launch_bounds__(kThreads) void k_morph_logmu_multi(LaunchArgs a, const int32_t* __restrict__ meta, double* __restrict__ lm) {
    const int item = blockIdx.y;
    const int NS = a.n0;
    const int64_t* __restrict__ rowoff = a.rowoff + (int64_t)item * NS;
    const double* __restrict__ coef = a.coef + (int64_t)item * NS * GC;
    const int col0 = meta[4 * item], ncol = meta[4 * item + 1];
    double* __restrict__ out = lm;                                    // row g of the group's table: out + g * Bp
    double sum[GC];
    unsigned bad[GC];
#pragma unroll
    for (int g = 0; g < GC; ++g) { sum[g] = 0.0; bad[g] = 0u; }
    log_table_load();
    const int n_tiles = a.n_tiles;
    const int chunks = (a.chunks > 1 && n_tiles >= 64 * a.chunks) ? a.chunks : 1;      // (ItemTiles, bi_k_item.h, written out)
    const int per_chunk = (n_tiles + chunks - 1) / chunks;
    if (ncol == 1) {
        // (block-uniform) a point alone in its cell: one column -- the other GC - 1 accumulators would be most of the
        // kernel's fp64 work for nothing (random cells: 5.1 -> 6.x TB/s); the same operations in the same order
        double s1 = 0.0;
        unsigned b1 = 0u;
        for (int lt = blockIdx.x; lt < per_chunk * chunks; lt += gridDim.x) {
            const int tile = chunks > 1 ? (lt % chunks) * per_chunk + lt / chunks : lt;
            if (tile >= n_tiles) continue;
            const int64_t bin0 = (int64_t)tile * kTile + threadIdx.x * kBinsPerThread;
            double m0 = 0.0, m1 = 0.0;
#pragma unroll 8
            for (int k = 0; k < NS; ++k) {
                const double2 v = stream_load<NT>(a.ps + rowoff[k] + bin0);
                const double c = coef[k * GC + col0];
                m0 = fma(c, v.x, m0);
                m1 = fma(c, v.y, m1);
            }
            double2 w;
            w.x = (m0 >= 0.0) ? bin_log(m0) : __builtin_nan("");
            w.y = (m1 >= 0.0) ? bin_log(m1) : __builtin_nan("");
            *reinterpret_cast<double2*>(out + (int64_t)col0 * a.Bp + bin0) = w;
            if (!(m0 >= 0.0) || !(m1 >= 0.0)) b1 = 1u;
            s1 += m0 + m1;
        }
#pragma unroll
        for (int g = 0; g < GC; ++g)
            if (g == col0) { sum[g] = s1; bad[g] = b1; }
    } else
    for (int lt = blockIdx.x; lt < per_chunk * chunks; lt += gridDim.x) {
        const int tile = chunks > 1 ? (lt % chunks) * per_chunk + lt / chunks : lt;
        if (tile >= n_tiles) continue;
        const int64_t bin0 = (int64_t)tile * kTile + threadIdx.x * kBinsPerThread;
        double acc[GC][2];
#pragma unroll
        for (int g = 0; g < GC; ++g) { acc[g][0] = 0.0; acc[g][1] = 0.0; }
#pragma unroll 8
        for (int k = 0; k < NS; ++k) {
            const double2 v = stream_load<NT>(a.ps + rowoff[k] + bin0);
#pragma unroll
            for (int g = 0; g < GC; ++g) {
                const double c = coef[k * GC + g];
                acc[g][0] = fma(c, v.x, acc[g][0]);
                acc[g][1] = fma(c, v.y, acc[g][1]);
            }
        }
        double l[2][GC];
#pragma unroll
        for (int g = 0; g < GC; ++g) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double m = acc[g][j];
                l[j][g] = (m >= 0.0) ? bin_log(m) : __builtin_nan("");
                if (!(m >= 0.0)) bad[g] = 1u;
            }
            sum[g] += acc[g][0] + acc[g][1];
        }
#pragma unroll
        for (int g = 0; g < GC; ++g)
            if (g >= col0 && g < col0 + ncol) {                       // (block-uniform) the columns of this item
                double2 w;
                w.x = l[0][g];
                w.y = l[1][g];
                *reinterpret_cast<double2*>(out + (int64_t)g * a.Bp + bin0) = w;
            }
    }
    __shared__ double sh[kThreads / 64][GC];
    __shared__ unsigned shf[kThreads / 64][GC];
#pragma unroll
    for (int g = 0; g < GC; ++g) {
        const double s = wave_sum(sum[g]);
        const unsigned f = wave_or(bad[g]);
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][g] = s; shf[threadIdx.x >> 6][g] = f; }
    }
    __syncthreads();
    if (threadIdx.x < GC) {
        const int g = threadIdx.x;
        double s = sh[0][g];
        unsigned f = shf[0][g];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) { s += sh[w][g]; f |= shf[w][g]; }
        const int64_t o = ((int64_t)item * gridDim.x + blockIdx.x) * GC + g;
        a.partial[o] = s;
        a.pflags[o] = f;
    }
}

// (2) the datasets' entry lists against the log mu tiles of PP points
// k_dataset_dot_tiled's pipeline (rings of offsets and entries in registers, every load unconditional, runs of whole 16-byte
// groups: see there) with PP accumulators per lane, written out a second time: under a shared walk the register counts of three
// variants of the two kernels moved.  blockIdx.x = bin tile of TB bins, blockIdx.y = slice of the datasets,
// blockIdx.z = pass.  LDS: PP / 2 planes of (TB + 1) 16-byte cells (dynamic: more than 64 KB needs the function attribute); the
// extra cell behind a plane holds 0.0 for the padding entries.
// partial [passes][dataset blocks of kPartBlock][n_tl][kPartBlock][PP].
// The block of tile 0 / slice 0 of every pass first adds up sum mu (and the "some mu negative or nan" flags) of the pass's PP points
// from the block partials of their log mu work items -- a fixed order: thread-strided, wave, the 16 waves in turn -- into
// MuTotals::tot / flag [pass in group][PP]: the finish kernel reads PP numbers instead of every one of its blocks adding them up.
template <int L, int AHEAD, int W, int PP, int TB>
__global__ __launch_bounds__(kDotThreads) void k_dataset_dot_multi(const void* __restrict__ tm_entries_v, const int64_t* __restrict__ tm_off,
                                                                   int64_t T, int n_tl, const double* __restrict__ lm, int64_t B,
                                                                   int64_t Bp, int64_t t0, int64_t n, double* __restrict__ partial, MuTotals mt) {
    typedef typename std::conditional<W == 2, uint16_t, uint32_t>::type entry_t;
    constexpr int EPL = 16 / W;                                        // entries per lane and load
    static_assert(EPL * L * AHEAD + 16 <= kDotPad, "the lists' padding must cover the read-ahead");
    static_assert(PP == 2 || PP == 4, "two or four points per pass");
    // LDS layout: planes of 16-byte cells, one cell per bin -- plane 0 holds (point 0, point 1) of every bin, plane 1 (point 2,
    // point 3) -- so that a wave's 16-byte reads of RANDOM bins spread over all eight 16-byte bank groups (bin & 7).  Round 5's
    // first layout kept a bin's four values adjacent (32 bytes): each of the two ds_read_b128 of an entry then only ever touched
    // every other bank group, and the kernel -- bound by LDS bank conflicts, 7.9 conflict cycles per LDS instruction on top of
    // its 8 -- ran 120 us per pass of four points.
    constexpr int kPlane = (TB + 1) * 16;                              // bytes per plane (+ the zero cell of the padding entries)
    const entry_t* __restrict__ tm_entries = static_cast<const entry_t*>(tm_entries_v);
    extern __shared__ double s_mu[];
    if (blockIdx.x == 0 && blockIdx.y == 0) {                          // (block-uniform)
        __shared__ double sh_m[kDotThreads / 64][PP];
        __shared__ unsigned sh_f[kDotThreads / 64][PP];
        const int pz = blockIdx.z;
#pragma unroll
        for (int g = 0; g < PP; ++g) {
            const int gc = pz * PP + g;
            const int item = mt.colmap[2 * gc];
            double m = 0.0;
            unsigned f = 0u;
            if (item >= 0) {
                const double* __restrict__ mp = mt.partial + (int64_t)item * mt.nmu * mt.GC + gc;
                const unsigned* __restrict__ mf = mt.flags + (int64_t)item * mt.nmu * mt.GC + gc;
                for (int b = threadIdx.x; b < mt.nmu; b += kDotThreads) { m += mp[(int64_t)b * mt.GC]; f |= mf[(int64_t)b * mt.GC]; }
            }
            const double mw = wave_sum(m);
            const unsigned fw = wave_or(f);
            if ((threadIdx.x & 63) == 0) { sh_m[threadIdx.x >> 6][g] = mw; sh_f[threadIdx.x >> 6][g] = fw; }
        }
        __syncthreads();
        if (threadIdx.x < PP) {
            double mm = 0.0;
            unsigned ff = 0u;
#pragma unroll
            for (int w = 0; w < kDotThreads / 64; ++w) { mm += sh_m[w][threadIdx.x]; ff |= sh_f[w][threadIdx.x]; }
            mt.tot[pz * PP + threadIdx.x] = mm;
            mt.flag[pz * PP + threadIdx.x] = ff;
        }
    }
    const int tl = blockIdx.x;
    const int pass = blockIdx.z;
    const int64_t bin0 = (int64_t)tl * TB;
    const int row = threadIdx.x / L, gl = threadIdx.x % L;
    const int per = (int)((n + gridDim.y - 1) / gridDim.y);
    const int c0u = (int)blockIdx.y * per, c1 = min((int)n, c0u + per);
    const int c0 = min(c0u, (int)n - 1);
    const int64_t* __restrict__ off = tm_off + (int64_t)tl * T + t0;
    const int64_t base = off[c0];
    const entry_t* __restrict__ ent = tm_entries + base;
    const uint32_t* __restrict__ off32 = reinterpret_cast<const uint32_t*>(off);
    const uint32_t base32 = (uint32_t)base;
    constexpr int kStep = kDotThreads / L, kAhead = AHEAD, kDepth = BI_DOT_DEPTH, kRing = 2 * (kDepth + 1);
    const int q_last = max(c0, c1 - 1);
    auto load_offsets = [&](int q, uint32_t& ra, uint32_t& rb) {
        const int qc = min(q, q_last);
        ra = off32[2 * qc];
        rb = off32[2 * qc + 2];
    };
    auto load_entries = [&](uint32_t ra, bi_uint4 (&e)[kAhead]) {
        const entry_t* __restrict__ p = ent + (int)(ra - base32) + EPL * gl;
#pragma unroll
        for (int k = 0; k < kAhead; ++k) __builtin_memcpy(&e[k], p + EPL * L * k, 16);
    };
    bi_uint4 E[kDepth + 1][kAhead];
    uint32_t RA[kRing], RB[kRing];
    const int q0 = c0 + row;
#pragma unroll
    for (int u = 0; u < 2 * kDepth; ++u) load_offsets(q0 + u * kStep, RA[u], RB[u]);
    {   // stage the tile: TB bins of each of the pass's PP rows, interleaved in LDS so that a bin's PP values are adjacent (all
        // loads first, addresses clamped instead of predicated; bins beyond the table read as 0.0: never addressed by an entry)
        const double* __restrict__ src = lm + (int64_t)pass * PP * Bp + bin0;
        const int avail = (int)(min(bin0 + TB, Bp) - bin0);           // (the table is Bp bins long, Bp a multiple of 512)
        constexpr int kPer = TB / 2 / kDotThreads;                    // 16-byte pieces per thread and row
        double2 v[PP][kPer];
#pragma unroll
        for (int g = 0; g < PP; ++g)
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int i2 = (threadIdx.x + k * kDotThreads) * 2;
                v[g][k] = *reinterpret_cast<const double2*>(src + (int64_t)g * Bp + min(i2, avail - 2));
            }
#pragma unroll
        for (int g = 0; g < PP; ++g)
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int i2 = (threadIdx.x + k * kDotThreads) * 2;
                const bool in = i2 < avail;
                double* __restrict__ cell = s_mu + (g >> 1) * (kPlane / 8) + (g & 1);
                cell[i2 * 2] = in ? v[g][k].x : 0.0;
                cell[(i2 + 1) * 2] = in ? v[g][k].y : 0.0;
            }
        if (threadIdx.x < PP) s_mu[(threadIdx.x >> 1) * (kPlane / 8) + TB * 2 + (threadIdx.x & 1)] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < kDepth; ++u) load_entries(RA[u], E[u]);
    __syncthreads();
    if (c0u >= c1) return;
    // partial sums in blocks of kPartBlock datasets, [pass][dataset block][tile][dataset in block][PP]: the finish of a dataset
    // block reads ONE contiguous range (all tiles of its datasets), the dot kernel writes whole 1 KB pieces of it
    const int64_t n_pad = (n + kPartBlock - 1) / kPartBlock * kPartBlock;
    double* __restrict__ pout = partial + (int64_t)pass * n_tl * n_pad * PP + (int64_t)tl * kPartBlock * PP;
    const int n_iter = (c1 - c0 + kStep - 1) / kStep;
    for (int it = 0; it < n_iter; it += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; ++u) {
            if (it + u < n_iter) {
                const int q = q0 + (it + u) * kStep;
                load_offsets(q + 2 * kDepth * kStep, RA[(u + 2 * kDepth) % kRing], RB[(u + 2 * kDepth) % kRing]);
                load_entries(RA[(u + kDepth) % kRing], E[(u + kDepth) % (kDepth + 1)]);
                __builtin_amdgcn_sched_barrier(0);
                const bi_uint4 (&e)[kAhead] = E[u % (kDepth + 1)];
                const int a = (int)(RA[u % kRing] - base32), b = (int)(RB[u % kRing] - base32);
                const int len = b - a - EPL * gl;
                double s[PP];
#pragma unroll
                for (int p = 0; p < PP; ++p) s[p] = 0.0;
                // one entry: its PP log mu values (adjacent in LDS) times its count, into the PP sums.  Padding entries carry count 0
                // and the offset of the extra slot behind the tile, which holds 0.0 (both entry widths: tiles of 4096 bins leave
                // a two-byte entry the bit for it): 0 x 0.0, no select -- and every padding lane of a wave reads the SAME LDS
                // address, a broadcast that costs the banks one access
                auto add_entry = [&](uint32_t byte_off, uint32_t cnt, double (&sg)[PP]) {
                    const char* __restrict__ q8 = reinterpret_cast<const char*>(s_mu) + (byte_off << 1);    // bin * 16
                    const double nn = (double)cnt;
#pragma unroll
                    for (int p = 0; p < PP; p += 2) {
                        const double2 lv = *reinterpret_cast<const double2*>(q8 + (p >> 1) * kPlane);
                        sg[p] = __builtin_fma(nn, lv.x, sg[p]);
                        sg[p + 1] = __builtin_fma(nn, lv.y, sg[p + 1]);
                    }
                };
#pragma unroll
                for (int g = 0; g < kAhead; ++g) {
                    // a load behind the run's end read other runs' entries: the whole group is skipped -- its LDS reads would be
                    // as random as live ones (the kernel is bound by LDS bank conflicts: 64 lanes x 32 random bytes per entry)
                    if (EPL * L * g < len) {
                        double sg[PP];
#pragma unroll
                        for (int p = 0; p < PP; ++p) sg[p] = 0.0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t x = e[g][k];
                            if constexpr (W == 4) {
                                add_entry(x & 0x1FFF8u, x >> 17, sg);
                            } else {
                                add_entry(x & 0xFFF8u, x & 7u, sg);
                                add_entry((x >> 16) & 0xFFF8u, (x >> 16) & 7u, sg);
                            }
                        }
#pragma unroll
                        for (int p = 0; p < PP; ++p) s[p] += sg[p];
                    }
                }
                for (int j = a + gl + EPL * L * kAhead; j < b; j += L) {                  // (runs beyond EPL L AHEAD entries)
                    const uint32_t x = ent[j];
                    if constexpr (W == 4) add_entry(x & 0x1FFF8u, x >> 17, s);
                    else add_entry(x & 0xFFF8u, x & 7u, s);
                }
#pragma unroll
                for (int p = 0; p < PP; ++p) s[p] = row_group_sum<L>(s[p]);
                if (gl == 0 && q < c1) {
#pragma unroll
                    for (int p = 0; p < PP; p += 2) {
                        double2 w;
                        w.x = s[p];
                        w.y = s[p + 1];
                        *reinterpret_cast<double2*>(pout + ((int64_t)(q / kPartBlock) * n_tl * kPartBlock + q % kPartBlock) * PP + p) = w;
                    }
                }
            }
        }
    }
}

// (3) finish: out[point][dataset]
// mu_tot / mu_flag [passes of the group][PP]: sum mu of every column's point and its flag, added up by the dot kernel's first block
// of the pass (MuTotals); colmap [passes][PP][2] = {work item of the log mu kernel, output row} of every column (-1: no point).
// k_dataset_finish_multi: blockIdx.y = pass, blockIdx.x = block of kPartBlock = 32 datasets.  A block is 32 datasets x 8 SLICES
// of the tiles: a thread adds the partial sums of ITS dataset over its slice of the tiles for all PP columns of the pass (the PP
// values of a (tile, dataset) are adjacent: 16-byte loads; the block's input is ONE contiguous range, [tile][32 datasets][PP]),
// the slices are added in order by the first 32 threads -- a fixed order.
// done != NULL: out is pinned host memory; the block that finishes last publishes `seq` there (publish_when_last).
template <int PP>
__global__ __launch_bounds__(kThreads) void k_dataset_finish_multi(const double* __restrict__ partial, int n_tl, const int32_t* __restrict__ colmap,
                                                                   const double* __restrict__ mu_tot, const unsigned* __restrict__ mu_flag,
                                                                   const double* __restrict__ lgsum, int64_t t0, int64_t n,
                                                                   double* __restrict__ out, int64_t out_stride,
                                                                   unsigned* __restrict__ blocks_done, unsigned long long* done,
                                                                   unsigned long long seq) {
    constexpr int kDs = kPartBlock, kSl = kThreads / kDs;
    __shared__ double part[kSl][PP][kDs];
    const int pass = blockIdx.y;
    const int32_t* __restrict__ cm = colmap + (int64_t)pass * PP * 2;
    const int dsl = threadIdx.x % kDs, sl = threadIdx.x / kDs;
    const int64_t t = (int64_t)blockIdx.x * kDs + dsl;
    const int per = (n_tl + kSl - 1) / kSl;
    const int b0 = min(n_tl, sl * per), b1 = min(n_tl, b0 + per);
    double s[PP];
#pragma unroll
    for (int g = 0; g < PP; ++g) s[g] = 0.0;
    if (t < n) {
        const int64_t n_pad = (n + kPartBlock - 1) / kPartBlock * kPartBlock;
        const double* __restrict__ p = partial + (int64_t)pass * n_tl * n_pad * PP + ((int64_t)blockIdx.x * n_tl * kDs + dsl) * PP;
        const int64_t stride = (int64_t)kDs * PP;
        // four tiles in flight per thread (PP / 2 16-byte loads each), four running sums (measured: 16 datasets x 16 slices with
        // eight in flight is slower, 40 against 33 us per pass of 10^4 datasets -- with the results going to pinned host memory
        // the kernel's floor is their ~320 KB over PCIe)
        constexpr int U = 4;
        double acc[4][PP];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int g = 0; g < PP; ++g) acc[k][g] = 0.0;
        int b = b0;
        for (; b + U - 1 < b1; b += U) {
            double2 vv[U][PP / 2];
#pragma unroll
            for (int k = 0; k < U; ++k)
#pragma unroll
                for (int g = 0; g < PP; g += 2) vv[k][g / 2] = *reinterpret_cast<const double2*>(p + (int64_t)(b + k) * stride + g);
#pragma unroll
            for (int k = 0; k < U; ++k)
#pragma unroll
                for (int g = 0; g < PP; g += 2) { acc[k & 3][g] += vv[k][g / 2].x; acc[k & 3][g + 1] += vv[k][g / 2].y; }
        }
        for (; b < b1; ++b)
#pragma unroll
            for (int g = 0; g < PP; ++g) acc[0][g] += p[(int64_t)b * stride + g];
#pragma unroll
        for (int g = 0; g < PP; ++g) s[g] = (acc[0][g] + acc[1][g]) + (acc[2][g] + acc[3][g]);
    }
#pragma unroll
    for (int g = 0; g < PP; ++g) part[sl][g][dsl] = s[g];
    __syncthreads();
    if (sl == 0 && t < n) {
        const double lg = lgsum[t0 + t];
#pragma unroll
        for (int g = 0; g < PP; ++g) {
            const int orow = cm[2 * g + 1];
            if (orow < 0) continue;
            double tot = 0.0;
#pragma unroll
            for (int q = 0; q < kSl; q += 4)
                tot += (part[q][g][dsl] + part[q + 1][g][dsl]) + (part[q + 2][g][dsl] + part[q + 3][g][dsl]);
            double r = (tot - mu_tot[pass * PP + g]) - lg;
            if (mu_flag[pass * PP + g]) r = __builtin_nan("");
            out[(int64_t)orow * out_stride + t] = r;
        }
    }
    if (!done) return;
    __syncthreads();
    if (threadIdx.x < 64) publish_when_last(blocks_done, gridDim.x * gridDim.y, done, seq);
}

// rows of rejected points (outside the anchor box, unphysical rates): -inf, as the reference answers before it looks at any data
__global__ void k_fill_rows(double* __restrict__ out, int64_t out_stride, const int32_t* __restrict__ rows, int n_rows, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int r = 0; r < n_rows; ++r) out[(int64_t)rows[r] * out_stride + i] = v;
}

}  // namespace
