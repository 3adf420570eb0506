// bi_k_misc.h -- the small kernels of the main translation unit (blueice_hip.hip): uploads, reductions, finish kernels,
// the toy-MC form, toy generation, histogramming, event scoring.  The heavy template families live in bi_k_morph.h,
// bi_k_bbgrad.h, bi_k_scan.h, bi_scan_sorted.h and bi_grad_mfma.h, one translation unit each.
#pragma once

#include "bi_philox.h"
#include "bi_k_draw.h"

namespace {

// self-test hook: out[i] = bin_log(x[i])
__global__ void k_selftest_log(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
    log_table_load();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = bin_log(x[i]);
}

// measurement probe: a plain sum over n2 16-byte elements -- the read-only streaming ceiling the morph kernel is
// compared with (bi_measure_read_bandwidth)
template <bool NT>
__global__ __launch_bounds__(kThreads) void k_read_sum(const double* __restrict__ p, int64_t n2, double* __restrict__ sink) {
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (; i + 7 * stride < n2; i += 8 * stride) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = stream_load<NT>(p + 2 * (i + u * stride));
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u].x + v[u].y;
    }
    for (; i < n2; i += stride) s += p[2 * i] + p[2 * i + 1];
    if (s == 0.123456789) sink[0] = s;      // keeps the loads alive, practically never stores
}

// measurement probe with the morph kernel's access pattern and nothing else: blockIdx.y = item, every item streams
// `rows` template rows of its own (row r of item i starts at element ((first + i * rows + r) % total_rows) * Bp), the
// tiles of a row are walked in the XCD-aware order of morph_tiles, 16 bytes per lane per row, `rows` loads in flight
// per lane in batches of 8 -- the ceiling `k_morph_reduce` can be held against (bi_measure_stream_bandwidth)
// PIECES: 16-byte pieces per lane per row (1 = the morph kernel's own 512-bin tiles; 2 = 1024-bin tiles, i.e. twice the
// contiguous run per row per block -- to see whether a wider tile would raise the ceiling: it does not, by more than 1 %)
template <bool NT, int PIECES>
__global__ __launch_bounds__(kThreads) void k_read_rows(const double* __restrict__ ps, int64_t Bp, int64_t total_rows,
                                                        int64_t first, int rows, int n_tiles, int chunks_in,
                                                        double* __restrict__ sink) {
    const int64_t row0 = first + (int64_t)blockIdx.y * rows;
    const int chunks = (chunks_in > 1 && n_tiles >= 64 * chunks_in) ? chunks_in : 1;      // (ItemTiles, bi_k_item.h, written out)
    const int per_chunk = (n_tiles + chunks - 1) / chunks;
    double s = 0.0;
    for (int lt = blockIdx.x; lt < per_chunk * chunks; lt += gridDim.x) {
        const int tile = chunks > 1 ? (lt % chunks) * per_chunk + lt / chunks : lt;
        if (tile >= n_tiles) continue;
        const int64_t bin0 = (int64_t)tile * kTile * PIECES + threadIdx.x * kBinsPerThread;
#pragma unroll 8
        for (int r = 0; r < rows; ++r) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) {
                const double2 v = stream_load<NT>(ps + ((row0 + r) % total_rows) * Bp + bin0 + q * kTile);
                s += v.x + v.y;
            }
        }
    }
    if (s == 0.123456789) sink[0] = s;      // keeps the loads alive, practically never stores
}

__global__ void k_mail_init(unsigned long long* slots, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slots[i] = kMailEmpty;
}

// second launch of the single-point path when the grid is too large for in-launch finishing to pay
// (an agent-scope release per block costs more than a kernel boundary once there are hundreds of blocks)
__global__ __launch_bounds__(kThreads) void k_finish_single(const double* __restrict__ partial,
                                                            const unsigned* __restrict__ pflags, int nbx, double slot_lg,
                                                            double* __restrict__ out, int32_t* __restrict__ status,
                                                            unsigned long long* done, unsigned long long seq) {
    __shared__ double sh[kThreads / 64];
    __shared__ unsigned shf[kThreads / 64];
    double s = 0.0;
    unsigned f = 0u;
#pragma unroll 8
    for (int b = threadIdx.x; b < nbx; b += kThreads) { s += partial[b]; f |= pflags[b]; }
    s = wave_sum(s);
    f = wave_or(f);
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; shf[threadIdx.x >> 6] = f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
        unsigned ff = shf[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) { t += sh[w]; ff |= shf[w]; }
        *out = t - slot_lg;
        *status = (int32_t)ff;
        __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Sum the per-block partials of every (item, g) in a fixed order, subtract the dataset's
// sum lgamma(n+1), scatter to the caller's point order.  `lanes` (64 or 256) threads per slot.
__global__ __launch_bounds__(kThreads) void k_finish(const double* __restrict__ partial,
                                                     const unsigned* __restrict__ pflags, int nbx, int G, int lanes,
                                                     int64_t n_slots, const int64_t* __restrict__ perm,
                                                     const double* __restrict__ slot_lg, double* __restrict__ out,
                                                     int32_t* __restrict__ status) {
    __shared__ double sh[kThreads / 64];
    __shared__ unsigned shf[kThreads / 64];
    const int per_block = kThreads / lanes;
    const int64_t slot = (int64_t)blockIdx.x * per_block + threadIdx.x / lanes;
    const int l = threadIdx.x % lanes;
    const bool live = slot < n_slots;
    const int64_t item = live ? slot / G : 0;
    const int g = live ? (int)(slot % G) : 0;
    const int64_t p = live ? perm[slot] : -1;
    const double lg = live ? slot_lg[slot] : 0.0;
    double s = 0.0;
    unsigned f = 0u;
    if (p >= 0) {
#pragma unroll 8
        for (int b = l; b < nbx; b += lanes) {
            const int64_t o = (item * nbx + b) * G + g;
            s += partial[o];
            f |= pflags[o];
        }
    }
    s = wave_sum(s);
    f = wave_or(f);
    if (lanes == 64) {
        if ((threadIdx.x & 63) == 0 && p >= 0) {
            out[p] = s - lg;
            if (status) status[p] |= (int32_t)f;
        }
        return;
    }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; shf[threadIdx.x >> 6] = f; }
    __syncthreads();
    if (threadIdx.x == 0 && p >= 0) {
        double t = sh[0];
        unsigned ff = shf[0];
        for (int w = 1; w < kThreads / 64; ++w) { t += sh[w]; ff |= shf[w]; }
        out[p] = t - lg;
        if (status) status[p] |= (int32_t)ff;
    }
}

// OR of the per-point status words of a plan -> one word (bi_plan_status)
__global__ __launch_bounds__(kThreads) void k_status_or(const int32_t* __restrict__ status, int64_t n, int32_t* __restrict__ out) {
    unsigned f = 0u;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) f |= (unsigned)status[i];
    f = wave_or(f);
    if ((threadIdx.x & 63) == 0 && f) atomicOr((unsigned*)out, f);
}

// a resident plan's status words are OR-ed into by every run: the "gave up" bit of one run must not outlive its report
__global__ __launch_bounds__(kThreads) void k_status_clear(int32_t* __restrict__ status, int64_t n, int32_t mask) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        if (status[i] & mask) status[i] &= ~mask;
}

__global__ void k_fill_value(double* __restrict__ out, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

__global__ void k_fill_const(double* __restrict__ out, const int64_t* __restrict__ idx, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[idx[i]] = v;
}

// sum_b lgamma(n_b + 1) over the valid counts of one dataset chunk -> partial[t][blk]
__global__ __launch_bounds__(kThreads) void k_counts_lgamma(const double* __restrict__ counts, int64_t B, int64_t Bp,
                                                            double* __restrict__ partial, int nblk) {
    const int t = blockIdx.y;
    const double* __restrict__ c = counts + (int64_t)t * Bp;
    double s = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x; b < B; b += (int64_t)nblk * kThreads) {
        const double n = c[b];
        if (n > 1.0 && n == floor(n)) s += lgamma(n + 1.0);
    }
    __shared__ double sh[kThreads / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sh[0];
        for (int w = 1; w < kThreads / 64; ++w) r += sh[w];
        partial[(int64_t)t * nblk + blockIdx.x] = r;
    }
}

// The narrow copy of the counts (build_narrow_counts): one byte per bin beside the doubles, same [dataset][padded bin] layout,
// eight bins per thread.  A value has a narrow form when converting it to a byte and back gives the SAME BITS (0 ... 255, whole;
// -0.0, nan, +-inf, negative, fractional and larger values have none); a dataset with one value that has none is flagged in
// bad[t] and keeps the double path (its narrow row is never read).  Padding bins are written as 0.
constexpr int kNarrowPerThread = 8;
__global__ __launch_bounds__(kThreads) void k_counts_narrow(const double* __restrict__ counts, int64_t B, int64_t Bp,
                                                            uint8_t* __restrict__ narrow, unsigned* __restrict__ bad) {
    const int t = blockIdx.y;
    const int64_t b0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kNarrowPerThread;
    bool lossy = false;
    if (b0 < Bp) {                                               // (Bp is a multiple of 512: a thread's eight bins are all inside or all outside)
        const double* __restrict__ src = counts + (int64_t)t * Bp + b0;
        unsigned long long packed = 0ull;
#pragma unroll
        for (int j = 0; j < kNarrowPerThread; ++j) {
            const double v = b0 + j < B ? src[j] : 0.0;
            const bool in_range = v >= 0.0 && v <= 255.0;       // (false for nan)
            const unsigned q = in_range ? (unsigned)(int)v : 0u;
            lossy |= __double_as_longlong((double)q) != __double_as_longlong(v);
            packed |= (unsigned long long)q << (8 * j);
        }
        *reinterpret_cast<unsigned long long*>(narrow + (int64_t)t * Bp + b0) = packed;
    }
    if (__ballot(lossy) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad + t, 1u);
}

// The packed shadow of the template rows (build_packed_rows; the format is described at kPkChunk in bi_dev_common.h): one
// block per chunk = 512-bin tile of a row, a thread takes the two bins a lane of morph_tiles owns.  A chunk has a packed
// form when each of its values is +0.0 or a positive normal double and the biased exponents of the non-zero ones lie within
// kPkSpan consecutive values; -0.0, negative values, subnormals, inf and nan have none.  One chunk without a packed form
// raises *bad, and the model keeps streaming ps (the shadow is then never read).
__global__ __launch_bounds__(kThreads) void k_pack_rows(const double* __restrict__ ps, int64_t chunk0, uint8_t* __restrict__ pk,
                                                        uint16_t* __restrict__ pk_base, unsigned* __restrict__ bad) {
    const int64_t q = chunk0 + blockIdx.x;
    const double2 v = *reinterpret_cast<const double2*>(ps + q * kTile + threadIdx.x * kBinsPerThread);
    const unsigned long long u[2] = {(unsigned long long)__double_as_longlong(v.x), (unsigned long long)__double_as_longlong(v.y)};
    unsigned emin = 0xFFFFu, emax = 0u;
    bool lossy = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (u[j] == 0ull) continue;
        const unsigned e = (unsigned)(u[j] >> 52);           // the sign bit rides on top: a negative value reads as e >= 2048
        lossy |= e < 1u || e > 2046u;
        emin = min(emin, e);
        emax = max(emax, e);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        emin = min(emin, (unsigned)__shfl_xor((int)emin, off, 64));
        emax = max(emax, (unsigned)__shfl_xor((int)emax, off, 64));
    }
    __shared__ unsigned s_min[kThreads / 64], s_max[kThreads / 64];
    if ((threadIdx.x & 63) == 0) { s_min[threadIdx.x >> 6] = emin; s_max[threadIdx.x >> 6] = emax; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { emin = min(emin, s_min[w]); emax = max(emax, s_max[w]); }
    const unsigned base = emax == 0u ? 0u : emin;             // (a chunk of zeros: no exponent to store)
    lossy |= emax > emin && emax - emin > (unsigned)(kPkSpan - 1);
    unsigned long long lo = 0ull;
    unsigned mid = 0u, top = 0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (u[j] == 0ull) continue;
        const unsigned code = ((unsigned)(u[j] >> 52) - base + 1u) & 15u;
        lo |= (u[j] & 0xFFFFFFFFull) << (32 * j);
        mid |= (unsigned)((u[j] >> 32) & 0xFFFFull) << (16 * j);
        top |= ((unsigned)((u[j] >> 48) & 0xFull) | (code << 4)) << (8 * j);
    }
    uint8_t* __restrict__ p = pk + q * kPkChunk;
    reinterpret_cast<unsigned long long*>(p)[threadIdx.x] = lo;
    reinterpret_cast<unsigned*>(p + kPkMidOff)[threadIdx.x] = mid;
    reinterpret_cast<uint16_t*>(p + kPkTopOff)[threadIdx.x] = (uint16_t)top;
    if (threadIdx.x == 0) pk_base[q] = (uint16_t)base;
    if (__ballot(lossy) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

// the shadow expanded back to doubles, out[chunk][512] (bi_unpack_rows: tests)
__global__ __launch_bounds__(kThreads) void k_unpack_rows(const uint8_t* __restrict__ pk, const uint32_t* __restrict__ pk_base,
                                                          int64_t chunk0, double* __restrict__ out) {
    const int64_t q = chunk0 + blockIdx.x;
    *reinterpret_cast<double2*>(out + q * kTile + threadIdx.x * kBinsPerThread) = pk_decode(pk_load<false>(pk, q), pk_exp_add(pk_base_word(pk_base, q), q));
}

__global__ void k_rows_sum(const double* __restrict__ partial, int nblk, double* __restrict__ out, int64_t T) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partial[t * nblk + b];
    out[t] = s;
}

// Compatibility morph: out[r][b] = sum_c V[row(c, r)][b] * w_c in the reference's corner order
// with separate multiply and add (scipy _evaluate_linear: `value = value + term`), i.e.
// bit-identical to the CPU path.  rows of `src` have stride Bp, rows of `out` stride B.
__global__ __launch_bounds__(kThreads) void k_morph_store(const double* __restrict__ src,
                                                          const int64_t* __restrict__ rowoff,  // [R][nc]
                                                          const double* __restrict__ w,        // [nc]
                                                          int nc, int64_t B, double* __restrict__ out,
                                                          const int32_t* __restrict__ place = nullptr) {
    const int r = blockIdx.y;
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    double v = 0.0;
    for (int c = 0; c < nc; ++c) {
        const double term = __dmul_rn(src[rowoff[(int64_t)r * nc + c] + b], w[c]);
        v = __dadd_rn(v, term);
    }
    // place: column b of the tensor is the caller's column place[b] (unbinned data whose events were ordered by cell)
    out[(int64_t)r * B + (place ? (int64_t)place[b] : b)] = v;
}

// sum over bins of one padded row -> out[row]  (used for the Beeston-Barlow N table)
__global__ __launch_bounds__(kThreads) void k_row_total(const double* __restrict__ rows, int64_t B, int64_t Bp,
                                                        double* __restrict__ out) {
    const double* __restrict__ r = rows + (int64_t)blockIdx.x * Bp;
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kThreads) s += r[b];
    __shared__ double sh[kThreads / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
        for (int w = 1; w < kThreads / 64; ++w) t += sh[w];
        out[blockIdx.x] = t;
    }
}

// The Beeston-Barlow normalisation N(z) = n_model_events[i].sum() (likelihood.py:645) in NUMPY'S summation order, so
// that single-point calls hand bb_roots the very bits the reference computes (the knife edge at
// U_b == 0).  np.sum over a contiguous array adds, in order, the pairwise sums of 8192-element chunks (its reduction
// buffer); a chunk's pairwise sum (numpy loops_utils.h.src, pairwise_sum) splits in halves down to blocks of 128, and a
// block is summed with 8 strided accumulators r_j = a[j] + a[8 + j] + ..., combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)).
// One block per chunk: interpolate a(z) for the chunk in the reference's order (value = value + V*w), reproduce that
// tree.  The (shorter) last chunk is written out as values and summed on the host by the same rule (pairwise_sum_host).
constexpr int kSumChunk = 8192;

// blockIdx.x = point (fastest in dispatch order: the points of one cell read a chunk's rows back to back, out of L2),
// blockIdx.y = chunk.  rowoff / w: [points][nc]; chunk_sum: [points][n_full]; tail: [points][B % 8192].
__global__ __launch_bounds__(kThreads) void k_bb_chunk_sums(const double* __restrict__ nm, const int64_t* __restrict__ rowoff_all,
                                                            const double* __restrict__ w_all, int nc, int64_t B,
                                                            double* __restrict__ chunk_sum_all, double* __restrict__ tail_all) {
    __shared__ double a[kSumChunk / 2];
    __shared__ double r[256];
    __shared__ double leaf[64];
    const int64_t q = blockIdx.x;
    const int64_t* __restrict__ rowoff = rowoff_all + q * nc;
    const double* __restrict__ w = w_all + q * nc;
    double* __restrict__ chunk_sum = chunk_sum_all + q * (B / kSumChunk);
    double* __restrict__ tail = tail_all + q * (B % kSumChunk);
    const int64_t b0 = (int64_t)blockIdx.y * kSumChunk;
    const int n = (int)(B - b0 < (int64_t)kSumChunk ? B - b0 : (int64_t)kSumChunk);
    if (n < kSumChunk) {                              // the last, partial chunk: values out, the host sums them
        for (int i = threadIdx.x; i < n; i += kThreads) {
            double v = 0.0;
            for (int c = 0; c < nc; ++c) v = __dadd_rn(v, __dmul_rn(nm[rowoff[c] + b0 + i], w[c]));
            tail[i] = v;
        }
        return;
    }
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        for (int i = threadIdx.x; i < kSumChunk / 2; i += kThreads) {
            double v = 0.0;
            for (int c = 0; c < nc; ++c) v = __dadd_rn(v, __dmul_rn(nm[rowoff[c] + b0 + half * (kSumChunk / 2) + i], w[c]));
            a[i] = v;
        }
        __syncthreads();
        {   // 32 blocks of 128 x 8 accumulators = 256 (block, j) pairs, one per thread
            const int blk = threadIdx.x >> 3, j = threadIdx.x & 7;
            double t = a[blk * 128 + j];
#pragma unroll
            for (int i = 1; i < 16; ++i) t = __dadd_rn(t, a[blk * 128 + 8 * i + j]);
            r[threadIdx.x] = t;
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const double* q = r + threadIdx.x * 8;
            leaf[half * 32 + threadIdx.x] = __dadd_rn(__dadd_rn(__dadd_rn(q[0], q[1]), __dadd_rn(q[2], q[3])),
                                                      __dadd_rn(__dadd_rn(q[4], q[5]), __dadd_rn(q[6], q[7])));
        }
    }
    __syncthreads();
    for (int stride = 1; stride < 64; stride <<= 1) {   // the halving recursion over 64 blocks = adjacent pairs, level by level
        if (threadIdx.x < 64 && (threadIdx.x % (2 * stride)) == 0) leaf[threadIdx.x] = __dadd_rn(leaf[threadIdx.x], leaf[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) chunk_sum[blockIdx.y] = leaf[0];
}

// full_output with Beeston-Barlow (likelihood.py:634-658) on already-morphed templates:
// aw[b] = A_b * w_b and per-block partial sums of it.
__global__ __launch_bounds__(kThreads) void k_bb_full(const double* __restrict__ ps_m, const double* __restrict__ a_row,
                                                      const double* __restrict__ counts_row,
                                                      const double* __restrict__ mus, int S, int src, double p_cal,
                                                      double Ntot, int64_t B, double* __restrict__ aw,
                                                      double* __restrict__ partial) {
    double s = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kThreads) {
        double U = 0.0;
        for (int k = 0; k < S; ++k) {
            const double e = __dmul_rn(ps_m[(int64_t)k * B + b], k == src ? 0.0 : mus[k]);
            U = k == 0 ? e : __dadd_rn(U, e);
        }
        const double ab = a_row[b];
        const double w = ps_m[(int64_t)src * B + b] / ab * Ntot;
        double r1, r2;
        bb_roots(ab, w * p_cal, U, counts_row[b], r1, r2);
        const double A = (U == 0.0) ? (counts_row[b] + ab) / (1.0 + p_cal) : r2;
        const double v = A * w;
        aw[b] = v;
        s += v;
    }
    __shared__ double sh[kThreads / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
        for (int w = 1; w < kThreads / 64; ++w) t += sh[w];
        partial[blockIdx.x] = t;
    }
}

__global__ void k_bb_normalise(const double* __restrict__ aw, const double* __restrict__ tot, int64_t B,
                               double* __restrict__ row) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) row[b] = aw[b] / tot[0];
}

// per padded row: sum over bins, minimum, and a "has non-finite" flag -> out[row*3 + {0,1,2}]
__global__ __launch_bounds__(kThreads) void k_row_stats(const double* __restrict__ rows, int64_t B, int64_t Bp,
                                                        double* __restrict__ out) {
    const double* __restrict__ r = rows + (int64_t)blockIdx.x * Bp;
    double s = 0.0, mn = __builtin_inf(), bad = 0.0;
    {   // (four loads in flight per thread: with one, the 37 MB tensor of a 9400-event unbinned toy took 147 us)
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        int64_t b = threadIdx.x;
        for (; b + 3 * kThreads < B; b += 4 * kThreads) {
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = r[b + k * kThreads];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s4[k] += v[k];
                mn = fmin(mn, v[k]);
                if (!(fabs(v[k]) < __builtin_inf())) bad = 1.0;
            }
        }
        for (; b < B; b += kThreads) {
            const double v = r[b];
            s4[0] += v;
            mn = fmin(mn, v);
            if (!(fabs(v) < __builtin_inf())) bad = 1.0;
        }
        s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    }
    __shared__ double sh[3][kThreads / 64];
    s = wave_sum(s);
    bad = wave_sum(bad);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = fmin(mn, __shfl_down(mn, off, 64));
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = mn; sh[2][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0][0], m = sh[1][0], f = sh[2][0];
        for (int w = 1; w < kThreads / 64; ++w) { t += sh[0][w]; m = fmin(m, sh[1][w]); f += sh[2][w]; }
        out[(int64_t)blockIdx.x * 3 + 0] = t;
        out[(int64_t)blockIdx.x * 3 + 1] = m;
        out[(int64_t)blockIdx.x * 3 + 2] = f;
    }
}

// ---- non-empty-bin lists (CSR) of the datasets, built in bin order (deterministic) -----------
constexpr int kNzPerThread = 8;
constexpr int kNzChunk = kThreads * kNzPerThread;  // 2048 bins per block

__device__ __forceinline__ bool is_nz(double n) { return n != 0.0; }  // true for nan as well

__global__ __launch_bounds__(kThreads) void k_nz_count(const double* __restrict__ counts, int64_t B, int64_t Bp,
                                                       int32_t* __restrict__ cnt, int nchunks) {
    const double* __restrict__ c = counts + (int64_t)blockIdx.y * Bp;
    const int64_t b0 = (int64_t)blockIdx.x * kNzChunk + threadIdx.x * kNzPerThread;
    int k = 0;
#pragma unroll
    for (int j = 0; j < kNzPerThread; ++j)
        if (b0 + j < B && is_nz(c[b0 + j])) ++k;
    __shared__ int sh[kThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k += __shfl_down(k, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(int64_t)blockIdx.y * nchunks + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(kThreads) void k_nz_scatter(const double* __restrict__ counts, int64_t B, int64_t Bp,
                                                         const int64_t* __restrict__ chunk_off, int nchunks,
                                                         int32_t* __restrict__ nz_idx, double* __restrict__ nz_n) {
    const double* __restrict__ c = counts + (int64_t)blockIdx.y * Bp;
    const int64_t b0 = (int64_t)blockIdx.x * kNzChunk + threadIdx.x * kNzPerThread;
    double v[kNzPerThread];
    int k = 0;
#pragma unroll
    for (int j = 0; j < kNzPerThread; ++j) {
        v[j] = (b0 + j < B) ? c[b0 + j] : 0.0;
        if (is_nz(v[j])) ++k;
    }
    // exclusive prefix of k over the block, in thread order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = k;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    __shared__ int sh[kThreads / 64];
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += sh[w];
    int64_t pos = chunk_off[(int64_t)blockIdx.y * nchunks + blockIdx.x] + base + incl - k;
#pragma unroll
    for (int j = 0; j < kNzPerThread; ++j)
        if (is_nz(v[j])) {
            nz_idx[pos] = (int32_t)(b0 + j);
            nz_n[pos] = v[j];
            ++pos;
        }
}

// compacted templates of one dataset: out[row][j] = rows[row][idx[j]] (0 beyond nnz)
__global__ __launch_bounds__(kThreads) void k_gather_rows(const double* __restrict__ rows, int64_t Bp,
                                                          const int32_t* __restrict__ idx, int64_t nnz, int64_t np,
                                                          double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= np) return;
    const int64_t row = blockIdx.y;
    out[row * np + j] = j < nnz ? rows[row * Bp + idx[j]] : 0.0;
}

__global__ void k_pad_copy(const double* __restrict__ src, int64_t n, int64_t np, double* __restrict__ dst) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < np) dst[j] = j < n ? src[j] : 0.0;
}

// ---- toy-MC generation on the device ---------------------------------------------------------
// n_{t,b} ~ Poisson(mu_b): the binned equivalent of Model.simulate (blueice/model.py:69-91: Poisson number of
// events per source, each drawn from the source's pdf) followed by set_data's binning (likelihood.py:603-609).
// Counter-based Philox4x32-10 keyed by the seed, counter = (bin, dataset, attempt): every (dataset, bin) draw
// is independent of launch geometry and can be regenerated, which is what lets the two-pass CSR build
// (count, then scatter) see the same numbers twice.
// (poisson_small for lam < 10 and poisson_ptrs from there on: bi_k_draw.h)

// The draws of bins b (even) and b + 1 of toy t: one Philox block gives both their uniforms.
__device__ __forceinline__ void poisson_draw_pair(const double* __restrict__ mu, const double* __restrict__ p0, int64_t B,
                                                  uint64_t seed, int64_t t, int64_t b, double& n0, double& n1) {
    n0 = n1 = 0.0;
    if (b >= B) return;
    const double2 lam = *reinterpret_cast<const double2*>(mu + b);      // rows are padded to an even length
    const double2 e = *reinterpret_cast<const double2*>(p0 + b);
    const bool has1 = b + 1 < B;
    const bool small0 = lam.x > 0.0 && lam.x < 10.0, small1 = has1 && lam.y > 0.0 && lam.y < 10.0;
    if (small0 || small1) {
        uint32_t r[4];
        const int64_t pair = b >> 1;
        philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), (uint32_t)t, (uint32_t)(t >> 32) & 0xFFFFu, (uint32_t)seed,
                      (uint32_t)(seed >> 32), r);
        if (small0) n0 = poisson_small(lam.x, e.x, u53(r[0], r[1]));
        if (small1) n1 = poisson_small(lam.y, e.y, u53(r[2], r[3]));
    }
    if (lam.x >= 10.0) n0 = poisson_ptrs(lam.x, seed, t, b);            // mu = 0 or invalid -> no events
    if (has1 && lam.y >= 10.0) n1 = poisson_ptrs(lam.y, seed, t, b + 1);
}

// p0[b] = exp(-mu[b]): once per bin, shared by all toys
__global__ void k_exp_neg(const double* __restrict__ mu, int64_t n, double* __restrict__ p0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p0[i] = exp(-mu[i]);
}

// A toy of a generator call: its number in the call (toy_offset + t is its number in the seed's ensemble) and the truth point
// it is drawn at.  The kernels below run over one method group of a call (the toys whose truth is drawn bin by bin, or event by
// event), blockIdx / thread i of a launch taking ref[i]; the entry is uniform over a block, so the loads stay scalar.  mu, p0
// (rows of stride Bp) and cdf (rows of stride B), M and npow2 are tables over the truths of the call.
struct ToyRef {
    int32_t t;
    int32_t h;
};

__global__ __launch_bounds__(kThreads) void k_toy_count(const double* __restrict__ mu, const double* __restrict__ p0, int64_t Bp,
                                                        int64_t B, uint64_t seed, int64_t toy0, const ToyRef* __restrict__ ref,
                                                        int32_t* __restrict__ cnt, int nchunks) {
    const ToyRef r = ref[blockIdx.y];
    const int64_t t = toy0 + r.t;
    mu += (int64_t)r.h * Bp;
    p0 += (int64_t)r.h * Bp;
    const int64_t b0 = (int64_t)blockIdx.x * kNzChunk + threadIdx.x * kNzPerThread;
    int k = 0;
#pragma unroll 1
    for (int j = 0; j < kNzPerThread; j += 2) {
        double n0, n1;
        poisson_draw_pair(mu, p0, B, seed, t, b0 + j, n0, n1);
        k += (n0 != 0.0) + (n1 != 0.0);
    }
    __shared__ int sh[kThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k += __shfl_down(k, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(int64_t)blockIdx.y * nchunks + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(kThreads) void k_toy_scatter(const double* __restrict__ mu, const double* __restrict__ p0, int64_t Bp,
                                                          int64_t B, uint64_t seed, int64_t toy0, const ToyRef* __restrict__ ref,
                                                          const int64_t* __restrict__ chunk_off, int nchunks,
                                                          int32_t* __restrict__ nz_idx, double* __restrict__ nz_n,
                                                          double* __restrict__ lg_partial) {
    const ToyRef r = ref[blockIdx.y];
    const int64_t t = toy0 + r.t;
    mu += (int64_t)r.h * Bp;
    p0 += (int64_t)r.h * Bp;
    const int64_t b0 = (int64_t)blockIdx.x * kNzChunk + threadIdx.x * kNzPerThread;
    double v[kNzPerThread];
    int k = 0;
    double lg = 0.0;
#pragma unroll
    for (int j = 0; j < kNzPerThread; j += 2) {
        poisson_draw_pair(mu, p0, B, seed, t, b0 + j, v[j], v[j + 1]);
#pragma unroll
        for (int q = j; q < j + 2; ++q)
            if (v[q] != 0.0) { ++k; if (v[q] > 1.0) lg += lgamma(v[q] + 1.0); }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = k;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int q = __shfl_up(incl, off, 64);
        if (lane >= off) incl += q;
    }
    __shared__ int sh[kThreads / 64];
    __shared__ double shl[kThreads / 64];
    lg = wave_sum(lg);
    if (lane == 63) sh[wave] = incl;
    if (lane == 0) shl[wave] = lg;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += sh[w];
    int64_t pos = chunk_off[(int64_t)blockIdx.y * nchunks + blockIdx.x] + base + incl - k;
#pragma unroll
    for (int j = 0; j < kNzPerThread; ++j)
        if (v[j] != 0.0) {
            nz_idx[pos] = (int32_t)(b0 + j);
            nz_n[pos] = v[j];
            ++pos;
        }
    if (threadIdx.x == 0) lg_partial[(int64_t)blockIdx.y * nchunks + blockIdx.x] = shl[0] + shl[1] + shl[2] + shl[3];
}

// lgsum of the toys of the bin-by-bin group: k_rows_sum's left-to-right sum over a toy's chunks, stored at the toy's number
__global__ void k_toy_lgsum(const double* __restrict__ lg_partial, int nchunks, const ToyRef* __restrict__ ref, int64_t n,
                            double* __restrict__ lgsum) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int q = 0; q < nchunks; ++q) s += lg_partial[i * nchunks + q];
    lgsum[ref[i].t] = s;
}

// ---- toy-MC generation, event by event (sparse expectations) ----------------------------------------------------
// Independent n_b ~ Poisson(mu_b) is the same law as N ~ Poisson(M = sum_b mu_b) events thrown onto the bins with
// probabilities mu_b / M.  Where M << B (10^4 expected events in 10^6 bins at C2) that is 100 times fewer random numbers
// than one draw per bin: one block per toy draws N, finds every event's bin by bisection in the cumulative sums of mu
// (8 MB, L2), sorts the bin numbers in LDS (bitonic, up to 32 768 keys = 128 KB of the CU's 160 KB) and run-length
// encodes them into the non-empty-bin list of the toy -- sorted by bin, as the per-bin generator leaves it.  Two passes
// with the same counters (Philox4x32-10 keyed by the seed; counter = (event, toy)): the first only counts the non-empty
// bins of every toy, the second writes them behind the offsets a scan made of the counts.
constexpr int kEvThreads = 512;
// (toy_event_count and its counter tag kEvTag: bi_k_draw.h)

// events per toy (an upper bound of its non-empty bins: the room it gets in the provisional lists)
// (overflow: one word per truth -- a toy beyond its truth's sort buffer sends that truth to the bin-by-bin group)
__global__ void k_toy_event_counts(const double* __restrict__ Mtab, const int* __restrict__ npow2tab, uint64_t seed, int64_t toy0,
                                   const ToyRef* __restrict__ ref, int64_t T, int64_t* __restrict__ n_ev, int* __restrict__ overflow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > T) return;
    if (i == T) { n_ev[i] = 0; return; }
    const ToyRef r = ref[i];
    const int npow2 = npow2tab[r.h];
    const int n = toy_event_count(Mtab[r.h], seed, toy0 + r.t);
    if (n > npow2) atomicOr(overflow + r.h, 1);
    n_ev[i] = min(n, npow2);
}

// (nnz_out runs over the group like room_off; lgsum over the toys of the call)
__global__ __launch_bounds__(kEvThreads) void k_toy_events(const double* __restrict__ cdf, int64_t B, const double* __restrict__ Mtab,
                                                           const int* __restrict__ npow2tab, uint64_t seed, int64_t toy0,
                                                           const ToyRef* __restrict__ ref, const int64_t* __restrict__ room_off,
                                                           int32_t* __restrict__ idx_out, double* __restrict__ n_out,
                                                           int64_t* __restrict__ nnz_out, double* __restrict__ lgsum) {
    const ToyRef tr = ref[blockIdx.x];
    const double M = Mtab[tr.h];
    const int npow2 = npow2tab[tr.h];
    cdf += (int64_t)tr.h * B;
    // LDS (sized for the truth of the call that needs most, laid out by this toy's own npow2):
    // radix sort (npow2 <= 16384): two key buffers of npow2 and 16 x 512 counters; bitonic sort: one key buffer;
    // then kEvThreads ints and doubles of scratch
    extern __shared__ uint32_t s_keys[];
    const bool radix = npow2 <= 16384;
    const int n_alloc = npow2;
    int key_bits = 1;
    while (key_bits < 32 && ((int64_t)1 << key_bits) < B) ++key_bits;
    int* s_scan = reinterpret_cast<int*>(s_keys + (radix ? 2 * n_alloc + 16 * kEvThreads / 2 : n_alloc));
    double* s_lg = reinterpret_cast<double*>(s_scan + kEvThreads);
    __shared__ int s_N;
    const int64_t t = toy0 + tr.t;
    const int tid = threadIdx.x;
    if (tid == 0) s_N = min(toy_event_count(M, seed, t), npow2);
    __syncthreads();
    const int N = s_N;
    int n2 = 1024;                                             // the power of two this toy needs (the sort is the cost)
    while (n2 < N) n2 <<= 1;
    for (int e = tid; e < n2; e += kEvThreads) {
        uint32_t key = 0xFFFFFFFFu;
        if (e < N) {
            uint32_t r[4];
            philox4x32_10((uint32_t)e, kEvTag, (uint32_t)t, (uint32_t)(t >> 32) & 0xFFFFu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
            const double target = u53(r[0], r[1]) * M;
            int64_t lo = 0, hi = B;                                         // first bin whose cumulative sum exceeds the target
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (cdf[mid] <= target) lo = mid + 1; else hi = mid;
            }
            key = (uint32_t)min(lo, B - 1);
        }
        s_keys[e] = key;
    }
    __syncthreads();
    if (radix) {
        // LSD radix sort, 4 bits per pass, in LDS: keys ping-pong between two buffers; every thread owns a contiguous chunk
        // and a column of 16 counters, so counting and scattering need no atomics and the sort is stable.  ~100 LDS
        // accesses per thread and pass against the bitonic network's 105 stages over all keys (10^4 toys of C2: 21 -> 5 ms).
        uint32_t* src = s_keys;
        uint32_t* dst = s_keys + n_alloc;
        uint16_t* cnt = reinterpret_cast<uint16_t*>(s_keys + 2 * n_alloc);        // [16][kEvThreads]
        const int chunk = n2 / kEvThreads, c0 = tid * chunk;
        for (int shift = 0; shift < key_bits; shift += 4) {
#pragma unroll
            for (int d = 0; d < 16; ++d) cnt[d * kEvThreads + tid] = 0;
            for (int i = 0; i < chunk; ++i) ++cnt[((src[c0 + i] >> shift) & 15u) * kEvThreads + tid];
            __syncthreads();
            // exclusive scan of the 16 x 512 counters in (digit, thread) order: thread t takes elements 16 t .. 16 t + 15
            unsigned local[16], sum = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) { local[q] = sum; sum += cnt[tid * 16 + q]; }
            unsigned incl = sum;
            const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(incl, off, 64);
                if (lane >= off) incl += v;
            }
            if (lane == 63) s_scan[wave] = (int)incl;
            __syncthreads();
            unsigned base = incl - sum;
            for (int w = 0; w < wave; ++w) base += (unsigned)s_scan[w];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16; ++q) cnt[tid * 16 + q] = (uint16_t)(base + local[q]);
            __syncthreads();
            for (int i = 0; i < chunk; ++i) {
                const uint32_t key = src[c0 + i];
                uint16_t& slot = cnt[((key >> shift) & 15u) * kEvThreads + tid];
                dst[slot] = key;
                ++slot;
            }
            __syncthreads();
            uint32_t* t2 = src; src = dst; dst = t2;
        }
        if (src != s_keys) {                                   // an odd number of passes: bring the result home
            for (int i = tid; i < n2; i += kEvThreads) s_keys[i] = src[i];
            __syncthreads();
        }
    } else {
        for (int k = 2; k <= n2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n2; i += kEvThreads) {
                    const int x = i ^ j;
                    if (x > i) {
                        const uint32_t a = s_keys[i], b = s_keys[x];
                        if ((a > b) == ((i & k) == 0)) { s_keys[i] = b; s_keys[x] = a; }
                    }
                }
                __syncthreads();
            }
    }
    // run-length encoding: every thread owns a contiguous segment of the sorted keys
    const int seg = n2 / kEvThreads;
    const int a0 = tid * seg, a1 = a0 + seg;
    int heads = 0;
    for (int i = a0; i < a1 && i < N; ++i) heads += (i == 0 || s_keys[i] != s_keys[i - 1]);
    s_scan[tid] = heads;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < tid; ++q) base += s_scan[q];                        // (512 additions per thread: nothing beside the sort)
    int64_t pos = room_off[blockIdx.x] + base;
    double lg = 0.0;
    for (int i = a0; i < a1 && i < N; ++i) {
        if (i != 0 && s_keys[i] == s_keys[i - 1]) continue;
        int j = i + 1;
        while (j < N && s_keys[j] == s_keys[i]) ++j;
        const double n = (double)(j - i);
        idx_out[pos] = (int32_t)s_keys[i];
        n_out[pos] = n;
        ++pos;
        if (n > 1.0) lg += lgamma(n + 1.0);
    }
    s_lg[tid] = lg;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int q = 0; q < kEvThreads; ++q) tot += s_lg[q];
        lgsum[tr.t] = tot;
        int nn = 0;
        for (int q = 0; q < kEvThreads; ++q) nn += s_scan[q];
        nnz_out[blockIdx.x] = nn;
    }
}

// the provisional lists (room for one entry per EVENT) packed into the final ones (one entry per non-empty bin)
__global__ __launch_bounds__(kThreads) void k_toy_pack(const ToyRef* __restrict__ ref, const int64_t* __restrict__ room_off,
                                                       const int64_t* __restrict__ nz_off,
                                                       const int32_t* __restrict__ idx_in, const double* __restrict__ n_in,
                                                       int32_t* __restrict__ nz_idx, double* __restrict__ nz_n) {
    const int64_t t = ref[blockIdx.x].t;
    const int64_t src = room_off[blockIdx.x], dst = nz_off[t], n = nz_off[t + 1] - dst;
    for (int64_t j = threadIdx.x; j < n; j += kThreads) { nz_idx[dst + j] = idx_in[src + j]; nz_n[dst + j] = n_in[src + j]; }
}

// set_data on the device: bin events into the analysis space with numpy.histogramdd semantics (what
// Histdd.add does in blueice/likelihood.py:608-609): per axis the bin is searchsorted(edges, x, 'right') - 1,
// the right-most edge is inclusive, events outside any axis range (or nan) are dropped.  Adding 1.0 with an fp64
// atomic is exact, so the result does not depend on the order of arrival.
struct HistArgs {
    int k;
    int n_edges[kMaxDim];
    int edge_off[kMaxDim];
};

__global__ __launch_bounds__(kThreads) void k_histogram(const double* __restrict__ coords /*[k][N]*/, int64_t N, HistArgs h,
                                                        const double* __restrict__ edges, double* __restrict__ counts) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= N) return;
    int64_t bin = 0;
    for (int a = 0; a < h.k; ++a) {
        const double x = coords[(int64_t)a * N + e];
        const double* __restrict__ g = edges + h.edge_off[a];
        const int n = h.n_edges[a];
        if (!(x >= g[0] && x <= g[n - 1])) return;      // out of range or nan
        int lo = 0, hi = n;                               // first index with g[idx] > x  (side = 'right')
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (g[mid] <= x) lo = mid + 1; else hi = mid;
        }
        int b = lo - 1;
        if (b == n - 1) b = n - 2;                        // x == last edge: belongs to the last bin
        bin = bin * (n - 1) + b;
    }
    atomicAdd(&counts[bin], 1.0);
}

// ---- unbinned set_data: histogram pdfs evaluated at the events ------------------------------------------------
// HistogramPdfSource.pdf (blueice/source.py:218-243) for every (anchor, source) row at once.  One thread = one event:
// the per-axis cell and weights are found once, then the thread walks the template rows (blockIdx.y strides over them).
//   method 0: density of the bin holding the event -- numpy.searchsorted(edges, x) - 1, clipped (nan sorts last);
//   method 1: scipy RegularGridInterpolator over the bin centres, its arithmetic: i = largest index with g[i] <= x
//             (at most n - 2), t = (x - g[i]) / (g[i+1] - g[i]); corners in itertools.product order (axis 0 slowest),
//             weight = ((1 * w_0) * w_1) ..., value = value + V * weight from 0 -- no contraction (the build sets
//             -ffp-contract=off), so the bits are scipy's.
struct ScoreArgs {
    int k, method;
    int clip;                    // 'linear': clip the coordinates to [first centre, last centre] HERE, as HistogramPdfSource.pdf does
                                 // (blueice/source.py:231-239) -- events simulated on the device keep their true coordinates
    int n_grid[kMaxDim];
    int grid_off[kMaxDim];
    int64_t stride[kMaxDim];     // bins (C order) per step along the axis
};

// Two passes (round 4).  Round 3's single kernel -- one thread per event looping over all anchors x sources rows -- let its
// blocks drift apart over the rows, so the 10^9-byte-scale gathers of 10^6 events came from a working set of gigabytes:
// every 8-byte value cost a whole memory transaction (10.6 ms for the 4 GB tensor of the C2 shape = 0.05 of the HBM peak).
// Now (1) k_score_locate finds every event's cell and interpolation weights ONCE, and (2) k_score_rows has the ROW as the
// slow grid dimension: blocks are dispatched row by row, so at any time the gathers of the whole chip fall into one or two
// 8 MB histograms that stay in L2 / Infinity Cache, and each histogram is read from HBM once (6.1 ms).  And (3) between the
// two the events are ORDERED BY CELL (radix sort of the cell indices, stable): the events of a block then fall into a few
// consecutive cache lines of the histogram, every line is fetched once per block instead of once per event, and the
// kernel becomes the stream it should be -- 4 GB in, 4 GB out.  The tensor's columns are then in sorted order; `perm`
// (sorted position -> the caller's event) stays with the context and bi_interpolate / bi_eval_full hand per-event values
// back in the caller's order, so the order is visible only to sums over events (1e-10, not bitwise, against a host-scored
// tensor).  Same arithmetic per value in the same order as before: bit-identical values.
__global__ __launch_bounds__(kThreads) void k_score_locate(const double* __restrict__ coords /*[k][N]*/, int64_t N, ScoreArgs a,
                                                           const double* __restrict__ grid, int64_t* __restrict__ base_out,
                                                           double* __restrict__ t_out /*[k][N], method 1 only*/) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= N) return;
    int64_t base = 0;
    for (int ax = 0; ax < a.k; ++ax) {
        double x = coords[(int64_t)ax * N + e];
        const double* __restrict__ g = grid + a.grid_off[ax];
        const int n = a.n_grid[ax];
        if (a.clip && a.method == 1) x = fmin(fmax(x, g[0]), g[n - 1]);
        int lo = 0, hi = n;
        if (a.method == 0) {                       // first index with g[idx] >= x  (side = 'left')
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (g[mid] < x) lo = mid + 1; else hi = mid;
            }
            if (x != x) lo = n;
        } else {                                   // first index with g[idx] > x
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (g[mid] <= x) lo = mid + 1; else hi = mid;
            }
        }
        const int i = min(max(lo - 1, 0), n - 2);
        if (a.method == 1) t_out[(int64_t)ax * N + e] = (x - g[i]) / (g[i + 1] - g[i]);
        base += i * a.stride[ax];
    }
    base_out[e] = base;
}

// events per thread of k_score_rows (their gathers are in flight together; one event where 2^K corners are many already)
constexpr int score_events_per_thread(int K) { return K <= 3 ? 4 : 1; }

// K: analysis dimensions of the 'linear' method (0 = 'piecewise': one value per event and row)
// RGI2D (K = 2 only; bi_sourcewise_score_events): value = value + (V * w_0) * w_1, the association of scipy's routine for
// two-dimensional fields, which RegularGridInterpolator takes for k = 2 -- the bits of HistogramPdfSource.pdf there too.  An
// instantiation of its own: k_score_rows<K> of bi_score_events and the simulators is the code it was.
template <int K, bool RGI2D = false>
__global__ __launch_bounds__(kThreads) void k_score_rows(const int64_t* __restrict__ base_in, const double* __restrict__ t_in, int64_t N,
                                                         ScoreArgs a, const double* __restrict__ rows, int64_t row_stride, int n_rows,
                                                         double* __restrict__ out, int64_t out_stride,
                                                         const int32_t* __restrict__ perm /*NULL: base_in in event order*/) {
    constexpr int kScoreEvents = score_events_per_thread(K);
    const int64_t e0 = (int64_t)blockIdx.x * (kThreads * kScoreEvents) + threadIdx.x;
    int64_t base[kScoreEvents];
    double t[kScoreEvents][K > 0 ? K : 1];
#pragma unroll
    for (int j = 0; j < kScoreEvents; ++j) {
        const int64_t e = min(e0 + (int64_t)j * kThreads, N - 1);
        base[j] = base_in[e];                        // (sorted keys when perm is given)
        const int64_t ev = perm ? (int64_t)perm[e] : e;
#pragma unroll
        for (int ax = 0; ax < K; ++ax) t[j][ax] = t_in[(int64_t)ax * N + ev];
    }
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const double* __restrict__ row = rows + (int64_t)r * row_stride;
        double value[kScoreEvents];
        if constexpr (K == 0) {
#pragma unroll
            for (int j = 0; j < kScoreEvents; ++j) value[j] = row[base[j]];
        } else {
#pragma unroll
            for (int j = 0; j < kScoreEvents; ++j) {
                const double* __restrict__ src = row + base[j];
                double v = 0.0;
                auto add_corner = [&](int corner) {
                    if constexpr (RGI2D) {
                        static_assert(K == 2, "scipy's own routine is the two-dimensional one");
                        const bool up0 = (corner >> 1) & 1, up1 = corner & 1;
                        const int64_t off = (up0 ? a.stride[0] : 0) + (up1 ? a.stride[1] : 0);
                        v = v + (src[off] * (up0 ? t[j][0] : 1.0 - t[j][0])) * (up1 ? t[j][1] : 1.0 - t[j][1]);
                        return;
                    }
                    double weight = 1.0;
                    int64_t off = 0;
#pragma unroll
                    for (int ax = 0; ax < K; ++ax) {
                        const bool up = (corner >> (K - 1 - ax)) & 1;
                        weight = weight * (up ? t[j][ax] : 1.0 - t[j][ax]);
                        if (up) off += a.stride[ax];
                    }
                    v = v + src[off] * weight;
                };
                if constexpr (K <= 3) {
#pragma unroll
                    for (int corner = 0; corner < (1 << K); ++corner) add_corner(corner);
                } else {
#pragma unroll 1
                    for (int corner = 0; corner < (1 << K); ++corner) add_corner(corner);
                }
                value[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < kScoreEvents; ++j) {
            const int64_t e = e0 + (int64_t)j * kThreads;
            if (e < N) out[(int64_t)r * out_stride + e] = value[j];
        }
    }
}

// ---- event-level toy Monte Carlo for histogram-pdf sources (bi_simulate_events) ---------------------------------
// Model.simulate (blueice/model.py:69-91): per source N_s ~ Poisson(mu_s) events, each drawn from the source's pdf --
// for a histogram pdf (HistogramPdfSource.simulate, source.py:248-264 -> Histdd.get_random) a bin with probability
// proportional to density x volume, then a uniform position inside the bin.  Here: pmf rows of the morphed densities and
// their running sums are prepared per source (k_sim_pmf + a scan), then one thread per event finds its source from the
// per-source counts, its bin by bisection in that source's cumulative sums and its position in the bin -- Philox4x32-10
// counters (event within its source, source) keyed by the seed, so a toy does not depend on the launch geometry.
// (SimArgs: bi_dev_common.h; kSimTag, kSimMaxRate and sim_one_event, the draw of one event: bi_k_draw.h)

// dens [S][B] (morphed densities) -> pmf [S][B] = density x bin volume (negative / nan densities count as 0)
__global__ __launch_bounds__(kThreads) void k_sim_pmf(const double* __restrict__ dens, SimArgs a, const double* __restrict__ edges,
                                                      int64_t B, double* __restrict__ pmf) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    double vol = 1.0;
    int64_t rem = b;
    for (int ax = 0; ax < a.k; ++ax) {
        const int64_t i = rem / a.stride[ax];
        rem -= i * a.stride[ax];
        const double* __restrict__ e = edges + a.edge_off[ax];
        vol *= e[i + 1] - e[i];
    }
    const double v = dens[(int64_t)blockIdx.y * B + b] * vol;
    pmf[(int64_t)blockIdx.y * B + b] = v > 0.0 ? v : 0.0;
}

// events per source: N_s ~ Poisson(rate_s), counter (source, stream)
__global__ void k_sim_counts(const double* __restrict__ rates, int S, uint64_t seed, int64_t* __restrict__ n_out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double M = rates[s];
    n_out[s] = (M > 0.0 && M < kSimMaxRate) ? (int64_t)toy_event_count(M, seed ^ 0x9E3779B97F4A7C15ull, (int64_t)s) : 0;
}

__global__ __launch_bounds__(kThreads) void k_sim_events(const double* __restrict__ cdf /*[S][B]*/, int64_t B, SimArgs a,
                                                         const double* __restrict__ edges, const int64_t* __restrict__ first /*[S+1]*/,
                                                         uint64_t seed, int64_t N, double* __restrict__ coords /*[k][N]*/,
                                                         int32_t* __restrict__ source /*[N]*/) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= N) return;
    int s = 0;
    while (s + 1 < a.S && e >= first[s + 1]) ++s;
    sim_one_event(cdf, B, a, edges, seed, s, e - first[s], N, e, coords, source);          // event j = e - first_s of source s
}

// ---- an ensemble of T event-level toys (bi_simulate_event_toys) ------------------------------------------------
// Toy D of the seed's ensemble is bi_simulate_events' toy with the seed toy_seed(seed, D) (bi_k_draw.h).

// one launch for the T x S counts: N_{t,s} ~ Poisson(rate_s) of toy toy0 + t (k_sim_counts with that toy's seed)
__global__ void k_sim_toy_counts(const double* __restrict__ rates, int S, int64_t T, uint64_t seed, int64_t toy0, int64_t* __restrict__ n_out /*[T][S]*/) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * S) return;
    const int64_t t = i / S;
    const int s = (int)(i - t * S);
    const double M = rates[s];
    const uint64_t ts = toy_seed(seed, (uint64_t)(toy0 + t));
    n_out[i] = (M > 0.0 && M < kSimMaxRate) ? (int64_t)toy_event_count(M, ts ^ 0x9E3779B97F4A7C15ull, (int64_t)s) : 0;
}

// the columns a toy takes: its events rounded up to even, so that the next set starts 16-byte aligned; room [T + 1] (last 0)
// goes through an exclusive prefix sum -> set_first [T + 1]
__global__ void k_sim_toy_room(const int64_t* __restrict__ n /*[T][S]*/, int S, int64_t T, int64_t* __restrict__ room /*[T+1]*/) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > T) return;
    int64_t tot = 0;
    if (t < T) for (int s = 0; s < S; ++s) tot += n[t * S + s];
    room[t] = (tot + 1) & ~(int64_t)1;
}

// first_{t,s} = set_first_t + sum_{s' < s} N_{t,s'}: [T][S + 1], the last entry the end of the toy's events
__global__ void k_sim_toy_first(const int64_t* __restrict__ n /*[T][S]*/, const int64_t* __restrict__ set_first /*[T+1]*/, int S, int64_t T,
                                int64_t* __restrict__ first /*[T][S+1]*/) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    int64_t at = set_first[t];
    for (int s = 0; s < S; ++s) { first[t * (S + 1) + s] = at; at += n[t * S + s]; }
    first[t * (S + 1) + S] = at;
}

// one launch for the bin search and the positions of all (t, s, j): column e of the padded layout belongs to the toy whose
// [set_first_t, set_first_{t+1}) holds it (bisection), then to a source as in k_sim_events.  A padding column (at most one
// behind a toy) gets the coordinate 0 and source -1.
__global__ __launch_bounds__(kThreads) void k_sim_toy_events(const double* __restrict__ cdf /*[S][B]*/, int64_t B, SimArgs a,
                                                             const double* __restrict__ edges, const int64_t* __restrict__ set_first /*[T+1]*/,
                                                             const int64_t* __restrict__ first /*[T][S+1]*/, int64_t T, uint64_t seed,
                                                             int64_t toy0, int64_t N /*columns*/, double* __restrict__ coords /*[k][N]*/,
                                                             int32_t* __restrict__ source /*[N]*/) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= N) return;
    int64_t lo = 0, hi = T;                          // the last t with set_first[t] <= e (empty toys share their start with the next)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (set_first[mid] <= e) lo = mid; else hi = mid;
    }
    const int64_t t = lo;
    const int64_t* __restrict__ f = first + t * (a.S + 1);
    if (e >= f[a.S]) {                               // padding
        for (int ax = 0; ax < a.k; ++ax) coords[(int64_t)ax * N + e] = 0.0;
        source[e] = -1;
        return;
    }
    int s = 0;
    while (s + 1 < a.S && e >= f[s + 1]) ++s;
    sim_one_event(cdf, B, a, edges, toy_seed(seed, (uint64_t)(toy0 + t)), s, e - f[s], N, e, coords, source);
}

// value -> the given columns of every row (the padding columns between event sets)
__global__ void k_fill_columns(double* __restrict__ rows, int64_t row_stride, int64_t n_rows, const int64_t* __restrict__ cols, int64_t n_cols, double value) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * n_cols) return;
    rows[(i / n_cols) * row_stride + cols[i % n_cols]] = value;
}

// small device -> pinned-host copies as a kernel (bi_memcpy_to_host): a copy-engine transfer of 80 KB costs 15 ... 110 us on
// this runtime, a launch writing through the host mapping about 10
__global__ void k_copy_words(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t n_words) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// densify one dataset from its non-empty-bin list
__global__ void k_csr_to_dense(const int32_t* __restrict__ idx, const double* __restrict__ n, int64_t nnz,
                               double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nnz) out[idx[j]] = n[j];
}

// The finish of a scan plan: partial is [items][nslots][16] (point fastest), one wave per item.  Lane l takes point
// l & 15 and the slots l >> 4, l >> 4 + 4, ...: every load instruction of the wave covers 64 consecutive doubles (k_finish
// walks the same array with one 8-byte element per 128-byte line and took 1.3 ms for the 640 MB of a 10^6-point scan;
// this takes 0.1).  Fixed order: slots in steps of four per lane, then the four lane groups -- bitwise reproducible.
__global__ __launch_bounds__(kThreads) void k_finish_scan(const double* __restrict__ partial, int nslots, int64_t n_items,
                                                          const int64_t* __restrict__ perm, const double* __restrict__ slot_lg,
                                                          double* __restrict__ out) {
    const int64_t item = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63, g = lane & 15;
    const double* __restrict__ src = partial + item * nslots * 16 + g;
    double s = 0.0;
#pragma unroll 4
    for (int b = lane >> 4; b < nslots; b += 4) s += src[(int64_t)b * 16];
    s = rows4_sum(s);
    if (lane < 16) {
        const int64_t p = perm[item * 16 + g];
        if (p >= 0) out[p] = s - slot_lg[item * 16 + g];
    }
}

// out[perm[slot]] = nan where the validity pass flagged the slot
__global__ __launch_bounds__(kThreads) void k_apply_bad(const unsigned* __restrict__ bad, const int64_t* __restrict__ perm,
                                                        int64_t n_slots, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_slots || !bad[i]) return;
    const int64_t p = perm[i];
    if (p >= 0) out[p] = __builtin_nan("");
}

}  // namespace
