// bi_k_sourcewise_scan.h -- the scan planner of source-wise points: from the per-point descriptors of k_sourcewise_plan<SC, NE = true>
// to the 16-point work items of k_scan_mfma.  Translation unit tu_sourcewise_scan.hip; host half bi_sourcewise_scan.h.
//
//   k_sourcewise_scan_key     one thread per (point, source slot): the 64-bit sort key of the point and its index
//   k_sourcewise_scan_cut     groups of equal keys cut every `cut` points (a multiple of 16), so that few cells with very long
//                             item lists still give the chip enough groups
//   k_sourcewise_scan_groups  one thread per sorted position: the group tables and the four counts the host reads
//   k_sourcewise_scan_fill    one thread per sorted position: ScanArgs' descriptors
//
// The key.  All points of one tuple of cells (one cell per source, over the axes that source owns) read the same NR rows; the
// first-corner row of a source names its cell.  With r_s that row counted from the source's first row and n_s the source's rows,
//     key = (sum_s r_s prod_{q > s} n_q) T + dataset        < (prod_s n_s) T = bad_key, the key of every rejected point.
// The row is read back from the planner's rowoff (rowoff = ne_off[t] + row ne_np[t]) instead of being searched for again: what
// the key names is what the planner wrote.  The SC lanes of a point are neighbours, so their S reads fall into one or two lines,
// and the radix sum is log2(SC) lane exchanges.
//
// These are gather / scatter kernels: their cost is the address pattern.  The fill kernel therefore reads a block's coefficients
// with the lanes walking (point, row) pairs -- the NR w_c of a point lie 8 W bytes apart, a wave's load covers 64 W doubles of
// at most a few points instead of one line per lane -- multiplies by the source's rate on the way into LDS ([row][thread] with a
// row pitch of one double more than the block: the lanes that walk a point's rows on the way in are spread over the banks -- with
// a pitch of the block itself all NR rows of a point met in one bank --, the lanes that walk the threads of a row on the way out
// are anyway), and writes from there with the lanes walking the slots of an item: the 16 slots of a row are one 128-byte line, a
// wave writes four whole lines per store.  Padding slots of a group's last item repeat its last point (perm -1):
// with coefficients of zero their expectations would be zero and k_scan_mfma's product form would leave its fast path for the
// whole item (k_plan_fill, bi_planning_device.h, does the same).
//
// No floating-point atomics (one integer maximum per group), no scratch: every index into the argument block's arrays is a
// compile-time constant of an unrolled loop (profiles/sourcewise_scan_kernel_resources.txt).
#pragma once

namespace {

constexpr int kSwScanFillThreads = 128;     // LDS of the fill kernel: NR (<= 32) doubles and one index per thread ...
constexpr int kSwScanFillPitch = kSwScanFillThreads + 1;   // ... the rows one double apart from a multiple of the banks

__global__ __launch_bounds__(kThreads) void k_sourcewise_scan_key(const SourcewiseScanArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t i = gid / a.SC;
    const int s = (int)(gid % a.SC);
    if (i >= a.n) return;                  // (whole groups: kThreads is a multiple of SC)
    const bool live = a.status[i] == 0;
    const int64_t ds = a.ds[i];
    const int64_t t = (ds < 0 || ds >= a.T) ? 0 : ds;      // (a rejected point: in-range reads, the key is bad_key anyway)
    int first = 0;
    int64_t row_first = 0, mult = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q == s) { first = a.first[q]; row_first = a.row_first[q]; mult = a.mult[q]; }
    int64_t part = 0;
    if (s < a.S) {
        const int64_t row = (a.rowoff_pt[i * a.NR + first] - a.ne_off[t]) / a.ne_np[t];
        part = (row - row_first) * mult;
    }
    for (int x = 1; x < a.SC; x <<= 1) part += __shfl_xor(part, x);
    if (s == 0) {
        a.keys[i] = live ? (uint64_t)(part * a.T + ds) : a.bad_key;
        a.idx[i] = i;
    }
}

__global__ __launch_bounds__(kThreads) void k_sourcewise_scan_cut(int64_t* __restrict__ gstart, int64_t n, int64_t cut) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t g = gstart[i];
    gstart[i] = g + (i - g) / cut * cut;
}

// grp_first / grp_items of every group in front of the rejected points, and the counts: scal[0] (valid points) was written by
// the kernel before this one; [1] items, [3] the most items of a group, [6] groups
__global__ __launch_bounds__(kThreads) void k_sourcewise_scan_groups(const SourcewiseScanArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nv = a.scal[0];
    if (i >= nv) return;
    const int64_t g0 = a.gstart[i], grp = a.gid_incl[i] - 1;
    if (g0 == i) a.grp_first[grp] = a.item_incl[i] - 1;
    if (i + 1 == nv || a.gstart[i + 1] == i + 1) {
        const int64_t items = a.item_incl[i] - (a.item_incl[g0] - 1);
        a.grp_items[grp] = (int32_t)items;
        atomicMax((unsigned long long*)(a.scal + 3), (unsigned long long)items);
    }
    if (i + 1 == nv) {
        a.scal[1] = a.item_incl[i];
        a.scal[6] = a.gid_incl[i];
    }
}

__global__ __launch_bounds__(kSwScanFillThreads) void k_sourcewise_scan_fill(const SourcewiseScanArgs a) {
    constexpr int BD = kSwScanFillThreads, PITCH = kSwScanFillPitch;
    extern __shared__ double s_fill[];
    double* __restrict__ s_c = s_fill;                                        // [NR][PITCH] w_c r_s
    int64_t* __restrict__ s_idx = reinterpret_cast<int64_t*>(s_c + (size_t)a.NR * PITCH);   // [BD]
    const int tx = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * BD;
    const int live = (int)min((int64_t)BD, a.n_valid - i0);
    if (tx < live) s_idx[tx] = a.idx_s[i0 + tx];
    __syncthreads();
    for (int e = tx; e < live * a.NR; e += BD) {
        const int q = e / a.NR, k = e - q * a.NR;
        const int64_t p = s_idx[q];
        int s = 0;                         // the source of row k: the last one whose first row is <= k
#pragma unroll
        for (int u = 1; u < 8; ++u) s += (u < a.S && k >= a.first[u]) ? 1 : 0;
        s_c[k * PITCH + q] = __dmul_rn(a.coef_pt[(p * a.NR + k) * a.W], a.rates_pt[p * a.SC + s]);
    }
    __syncthreads();
    if (tx >= live) return;
    const int64_t i = i0 + tx, p = s_idx[tx];
    const int g = (int)((i - a.gstart[i]) % 16);
    const int64_t item = a.item_incl[i] - 1;
    const bool last_of_group = i + 1 == a.n_valid || a.gstart[i + 1] == i + 1;
    const int g_end = last_of_group ? 16 : g + 1;
    for (int k = 0; k < a.NR; ++k) {
        const double v = s_c[k * PITCH + tx];
        for (int gg = g; gg < g_end; ++gg) a.coef[(item * a.NR + k) * 16 + gg] = v;
    }
    if (g == 0) {
        for (int k = 0; k < a.NR; ++k) a.rowoff[item * a.NR + k] = a.rowoff_pt[p * a.NR + k];
        a.item_cnt[item] = a.cnt_off_pt[p];
        a.item_tiles[item] = a.tiles_pt[p];
    }
    a.slot_lg[item * 16 + g] = a.slot_lg_pt[p];
    a.perm[item * 16 + g] = p;
    for (int gg = g + 1; gg < g_end; ++gg) {
        a.slot_lg[item * 16 + gg] = 0.0;
        a.perm[item * 16 + gg] = -1;
    }
}

}  // namespace
