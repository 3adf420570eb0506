// bi_dev_common.h -- device helpers and launch-argument structs shared by every translation unit of libblueice_hip
// (gfx950 only).  No __global__ function lives here: a kernel is defined in the header of the ONE translation unit that
// launches it (bi_k_*.h), so that the families compile in parallel and no kernel is emitted twice.  DESIGN.md section 4.
#pragma once

// ---- launch-argument structs (global scope: they cross translation units through the tu_launch_* functions) ----

constexpr long long kMailTicksPerMs = 100000;                          // wall_clock64 runs at 100 MHz

struct LaunchArgs {
    const double* ps;       // [rows][Bp]
    const double* nm;       // [A][Bp] (BB) or null
    const double* counts;   // [T][Bp]
    const int64_t* rowoff;  // [items][NS]  element offsets of the stream rows
    const double* coef;     // [items][NS][G]
    const double* aux;      // [items][G][2]  (p_cal, N) for BB
    const int64_t* item_cnt; // [items] element offset of the item's counts row (k_morph_sets: the events of the item's set)
    const int32_t* item_tiles; // [items] 512-bin tiles of the item's rows (NULL: n_tiles)
    double* partial;        // [items][nbx][G]
    unsigned* pflags;       // [items][nbx][G]
    int64_t B, Bp;
    double outlier;         // MODE 2: likelihood given to events with a non-positive density (0 = none)
    int n0, n1, n2;         // streams into U (or mu), into P_i, into a
    int n_tiles;
    int chunks;             // > 1: consecutive blocks work in `chunks` far-apart regions of the rows
    int n_keep;             // NT kernels: the first n_keep stream rows are loaded with the default (cacheable) policy
    // in-launch finish (k_morph_reduce): when fin_mail != NULL the item's last block collects the item's partials
    // from the mailbox slots and writes the results -- no k_finish launch behind the morph launch
    double* fin_mail;           // [items][nbx][G] mailbox slots, empty on entry and on exit
    unsigned* fin_flags;        // [items][G] status words (Beeston-Barlow), zero on entry and on exit
    const int64_t* fin_perm;    // [items][G]  result index of every slot (-1: unused slot)
    const double* fin_slot_lg;  // [items][G]  constant subtracted from the sum
    double* fin_out;            // results (device or pinned host memory)
    int32_t* fin_status;        // or NULL
    int nan_S;              // MODE 2 with non-finite pdf values: number of sources (streams are [corner][source]); the
                            // sum over sources then skips nan terms -- np.nansum, blueice/likelihood.py:686.  0 = off
    long long mail_timeout = 2000 * kMailTicksPerMs; // in-launch finish: ticks of the 100 MHz wall clock a collector waits (context: mail_timeout_ms;
                            // default 2 s, far beyond any delay a busy, shared GPU causes)
    int skip_post = -1, late_post = -1;   // fault injection (tests): this block never posts / posts after the collector gave up; -1 = off
    // (last, so that no other member moves in the kernel-argument block: the existing instantiations compile as before)
    const uint8_t* cnt8 = nullptr;   // [T][Bp] the counts as one byte per bin, or NULL: the launch reads the doubles (build_narrow_counts)
    const uint8_t* pk = nullptr;     // the packed shadow of ps (build_packed_rows), 7 bytes per value, or NULL: the launch reads ps
    const uint32_t* pk_base = nullptr; // ... and its exponent bases, one uint16_t per (row, tile), read two at a time
};

// ---- the packed shadow of the template rows ----
// One 3584-byte chunk per 512-bin tile of a row, chunks in the order of the tiles in ps (chunk q = elements [512 q, 512 q + 512)
// of ps): [512 x u32: mantissa bits 0..31][512 x u16: bits 32..47][512 x u8: bits 48..51 | code << 4].  code 0: the value is
// +0.0 (every stored bit 0); code 1..15: biased exponent base + code - 1, base = the smallest exponent of the chunk's non-zero
// values (pk_base[q], 11 bits in a uint16_t).
constexpr int kPkChunk = 3584;       // 7 * kTile
constexpr int kPkMidOff = 2048;      // 4 * kTile
constexpr int kPkTopOff = 3072;      // 6 * kTile
constexpr int kPkSpan = 15;          // exponents a chunk's non-zero values may take

constexpr int kMaxSingleStreams = 128;

struct SingleDesc {
    int64_t rowoff[kMaxSingleStreams];
    double coef[kMaxSingleStreams];
    double aux[2];        // Beeston-Barlow: p_cal, N
    double slot_lg;       // constant subtracted from the sum (sum lgamma, empty-bin term, or sum of rates)
    unsigned* flags;      // one status word (Beeston-Barlow bits), zero on entry and on exit
    double* out;          // pinned host
    int32_t* status;      // pinned host
    unsigned long long* done;   // pinned host: receives `seq` after out / status (the host polls it)
    unsigned long long seq;
};

typedef double bi_double4 __attribute__((ext_vector_type(4)));

struct ScanArgs {
    const double* ps;
    const double* counts;
    const int64_t* rowoff;      // [items][NS]   (rows of a group = rows of its first item)
    const double* coef;         // [items][NS][16]
    const int64_t* item_cnt;    // [items]
    const int32_t* item_tiles;  // [items] 512-bin tiles of the item's rows
    const int64_t* grp_first;   // [groups] first item of the group
    const int32_t* grp_items;   // [groups] items in the group
    double* partial;            // [items][nslots][16], zero on entry
    int NS;
    int nslots;                 // waves per group = gridDim.x * 4
    int n_groups;               // k_scan_sorted (one-dimensional grid, dealt to the XCDs in contiguous ranges of blocks)
    int xcd_mode;               // 0 launch order, 1 contiguous ranges (default), 2 group g -> XCD g mod 8
    int share_slow;             // k_scan_sorted: strips of mixed counts are worked by all waves of the cell together
};

struct ValidArgs {
    const double* ps;
    const int64_t* rowoff;      // [items][NS] element offsets of the FULL rows (rows of a group = rows of its first item)
    const double* coef;         // [items][NS][16]
    const int64_t* grp_first;   // [groups]
    const int32_t* grp_items;   // [groups]
    unsigned* bad;              // [items][16], zero on entry: set to 1 where a point has a bin with mu < 0 or nan
    int NS;
    int nslots;                 // waves per group = gridDim.x * 4
    int n_strips;               // strips of 16 CB bins per full row
};

// k_scan_bb (bi_k_scan_bb.h): Beeston-Barlow scans on the matrix cores
struct BbScanArgs {
    const double* ps;           // template rows
    const double* nm;           // Monte-Carlo count rows of the Beeston-Barlow source
    const double* counts;
    const int64_t* rowoff;      // [items][NS]   (rows of a group = rows of its first item)
    const double* coef;         // [items][NS][16]: n0 streams into U, nc into P, nc into a
    const double* aux;          // [items][16][2]  (p_cal, N) per point
    const int64_t* item_cnt;    // [items] element offset of the item's counts row
    const int64_t* grp_first;   // [groups] first item of the group
    const int32_t* grp_items;   // [groups] items in the group
    double* partial;            // [items][gridDim.x][16]
    unsigned* pflags;           // [items][gridDim.x][16]
    int64_t B;
    int n0, nc;
    int n_tiles;                // tiles of 16 bins covering [0, B)
};

// k_grad_mfma (bi_k_grad_mfma.h)
struct GradMfmaArgs {
    const double* ps;
    const double* counts;
    const int64_t* rowoff;      // [items][NS]   (rows of a group = rows of its first item)
    const double* coef;         // [items][NS][16]  value coefficients w_corner * r_source (unused slots repeat a point)
    const int64_t* item_cnt;    // [items]
    const int32_t* item_tiles;  // [items]
    const int64_t* grp_first;   // [groups]
    const int32_t* grp_items;   // [groups]
    double* part_ll;            // [items][n_slices][16]
    double* part_g;             // [items][n_slices][NSP][16]   NSP = 16 * NB
    int NS, n_slices;
};

// k_morph_hess (bi_k_hess.h)
struct HessArgs {
    const double* ps;          // [rows][Bp] (or the compacted rows of the non-empty bins)
    const double* counts;      // [T][Bp] (or the compacted counts); unused when UNB
    const int64_t* rowoff;     // [items][NS] element offsets of the rows
    const double* coef;        // [items][NS][G]
    const int64_t* item_cnt;   // [items] element offset of the item's counts row
    const int32_t* item_tiles; // [items] 512-bin tiles of the item's rows
    double* partial;           // [items][nbx][NSL]
    unsigned* pflags;          // [items][nbx][NSL] (zeroes: k_finish reads them)
    int64_t B;                 // bins (events) of a row; UNB: later entries are padding
    double outlier;            // UNB: likelihood of events whose density is not > 0 (0 = none)
    int NS;                    // rows per item
    int D;                     // first-order columns (<= DM)
    int chunks;                // > 1: consecutive blocks work in far-apart regions of long rows (as morph_tiles)
};

// k_morph_factored (bi_k_factored.h), k_factored_curv (bi_k_factored_curv.h): one point of a source-wise model per item.  The rows of an item are its sources' corner
// rows back to back, source s contributing 1 << e[s] of them (e[s] < 0: a padded source, no rows); EM is the kernel's
// template argument, the largest e[s] it is built for.
struct FactoredArgs {
    const double* ps;          // [rows][Bp] every source's anchor rows
    const double* counts;      // [T][Bp]
    const int64_t* rowoff;     // [items][NR] element offsets of the item's corner rows
    const double* coef;        // [items][NR][1 + EM] per row: w_c, then d w_c / d (own axis j), zero for j >= e[s]
    const double* rates;       // [items][SC] r_s = M_s(z) rs_s (zero for padded sources)
    const int64_t* item_cnt;   // [items] element offset of the item's counts row
    double* partial;           // [items][nbx][NSL]
    unsigned* pflags;          // [items][nbx][NSL] (zeroes: k_finish reads them)
    int n_tiles;               // 512-bin tiles of every row
    int NR;                    // rows per item
    int chunks;                // > 1: consecutive blocks work in far-apart regions of long rows (ItemTiles)
    int e[8];                  // own axes of every source
    // k_factored_curv (bi_k_factored_curv.h) alone: coef is [items][NR][1 + EM + EM (EM - 1) / 2] in its observed form, and its
    // Fisher form reads
    const double* chain;       // [items][SC][1 + EM] per source: M_s, then rs_s d M_s / d (own axis j)
    unsigned lead;             // bit s * 3 + j: slot (s, j) is the first slot of its axis (the one that counts for it)
    signed char ax[8][3];      // the axis of slot (s, j), -1 for none
    // k_morph_factored<.., GRAD = false, ..> alone: items planned on the device (k_sourcewise_plan).  NULL on every other path.
    const unsigned* live;      // [items] 0: a rejected point -- its blocks return at once: no row is read, no partial posted
};

// k_sourcewise_plan (bi_k_sourcewise_plan.h): the device copy of what fac_geometry and FacSource::at read (bi_factored.h) ...
struct SourcewiseGeom {
    const double* anchors;     // the d axes' anchors back to back
    const int32_t* anchor_off; // [d + 1] where an axis' anchors start
    const int32_t* n_own;      // [S] e_s
    const int32_t* own;        // [S][3] the owned axes, ascending
    const int64_t* own_stride; // [S][3] row stride of every owned axis
    const int64_t* row_first;  // [S] first row of source s
    const double* mus;         // [rows] the anchors' rates
    const double* lgsum;       // [T] sum_b lgamma(n_b + 1) of every dataset
    int64_t T, Bp;
    int d, S;
    // k_sourcewise_plan<SC, NE = true> alone (the non-empty-bin form, bi_sourcewise_nonempty.h)
    const double* rowsum;      // [rows] R_{s,c}: the anchor rows' totals over all bins
    const int64_t* ne_off;     // [T] where the dataset's compacted rows start
    const int64_t* ne_np;      // [T] its list length padded to whole tiles
    const int64_t* ne_cnt_off; // [T] where its compacted counts start
};
// ... and n staged points in VarMap's layouts -> their status words and FacBatch's value-order descriptors
struct SourcewisePlanArgs {
    SourcewiseGeom g;
    const double* z;           // [n][d]
    const double* rs;          // [n][S]
    const int64_t* ds;         // [n]
    int64_t n;
    int NR, W;                 // rows per item, coefficient columns per row (1 + EM)
    int e[8];                  // own axes of every source slot, -1: padded (FactoredArgs::e)
    int32_t* status;           // [n]
    unsigned* live;            // [n] status == 0
    int64_t* rowoff;           // [n][NR]
    double* coef;              // [n][NR][W]
    double* rates;             // [n][SC]
    int64_t* cnt_off;          // [n]
    double* slot_lg;           // [n]
    int64_t* perm;             // [n] k_finish's: i, or -1 for a rejected point (neither summed nor written)
    double* out;               // [n] where k_finish writes the results: the planner writes a rejected point's -inf
    int32_t* tiles;            // [n] (NE, EV) the 512-bin tiles of the item's dataset's list / of its event set
    // k_sourcewise_plan<SC, false, EV = true> alone (the event store, bi_sourcewise_events.h); g.T is the number of event sets there
    const int64_t* ev_first;   // [T] the set's first column
    const int64_t* ev_n;       // [T] its number of events
    int64_t ev_cols;           // columns of every row of the store
};

// k_sourcewise_nonempty (bi_k_sourcewise_nonempty.h): FactoredArgs' descriptors over the compacted copies of the non-empty bins.
// The rows of an item lie in ITS dataset's copy (rowoff holds the copy's offset), and so does the number of tiles: per item.
struct SourcewiseNonemptyArgs {
    const double* ps;          // the compacted rows of every dataset
    const double* counts;      // the compacted counts of every dataset
    const int64_t* rowoff;     // [items][NR] element offsets of the item's corner rows in ps
    const double* coef;        // [items][NR][1 + EM] as FactoredArgs::coef
    const double* rates;       // [items][SC]
    const int64_t* item_cnt;   // [items] element offset of the item's compacted counts
    const int32_t* item_tiles; // [items] tiles of the item's list (>= 1)
    double* partial;           // [items][gridDim.x][NSL]
    unsigned* pflags;          // [items][gridDim.x][NSL]
    int NR;                    // rows per item
    int chunks;                // ItemTiles' chunks
    int max_blocks;            // an item's tiles are walked by min(tiles, max_blocks) blocks, whatever gridDim.x is
    int e[8];                  // own axes of every source
    const unsigned* live;      // [items] planned items (GRAD = false): 0 = rejected; NULL on the host paths
};

// k_sourcewise_events (bi_k_sourcewise_events.h): FactoredArgs' descriptors over the event store of a source-wise model.  The rows
// of an item are the store's rows at ITS event set's columns (rowoff holds the set's first column), and the number of tiles and
// of events is the set's: per item.
struct SourcewiseEventsArgs {
    const double* ps;          // [rows][columns] the pdf values of every event at every anchor row
    const int64_t* rowoff;     // [items][NR] element offsets of the item's corner rows at its set's first column
    const double* coef;        // [items][NR][1 + EM] as FactoredArgs::coef
    const double* rates;       // [items][SC]
    const int64_t* item_n;     // [items] events of the item's set: later columns are padding, masked by index
    const int32_t* item_tiles; // [items] tiles of the item's set (>= 1)
    double* partial;           // [items][gridDim.x][NSL]
    unsigned* pflags;          // [items][gridDim.x][NSL]
    double outlier;            // likelihood of events whose density is not > 0 (0 = none)
    int NR;                    // rows per item
    int chunks;                // ItemTiles' chunks
    int max_blocks;            // an item's tiles are walked by min(tiles, max_blocks) blocks, whatever gridDim.x is
    int e[8];                  // own axes of every source
};

// The scan planner of source-wise points (bi_k_sourcewise_scan.h): from what k_sourcewise_plan<SC, NE = true> wrote per point to
// ScanArgs' descriptors per 16-point item.  One block of arguments for its four kernels; every pointer is device memory.
struct SourcewiseScanArgs {
    // per point, the planner's output (and the staged datasets)
    const int32_t* status;     // [n]
    const int64_t* rowoff_pt;  // [n][NR]
    const double* coef_pt;     // [n][NR][W], column 0 = w_c
    const double* rates_pt;    // [n][SC]
    const int64_t* cnt_off_pt; // [n]
    const int32_t* tiles_pt;   // [n]
    const double* slot_lg_pt;  // [n]
    const int64_t* ds;         // [n]
    const int64_t* ne_off;     // [T] where a dataset's compacted rows start
    const int64_t* ne_np;      // [T] their length
    int64_t n, T;
    int NR, W, SC, S;
    int first[8];              // first row of source s among a point's NR rows
    int64_t row_first[8];      // first row of source s in the model
    int64_t mult[8];           // mixed radix: the product of the row counts of the sources behind s
    uint64_t bad_key;          // (all cell tuples) * T: the key of rejected points, one above every other
    // k_sourcewise_scan_key
    uint64_t* keys;            // [n]
    int64_t* idx;              // [n]
    // sorted order: k_sourcewise_scan_cut, k_sourcewise_scan_groups, k_sourcewise_scan_fill
    const int64_t* idx_s;      // [n] the point at every sorted position
    int64_t* gstart;           // [n] first sorted position of the position's group
    const int64_t* item_incl;  // [n] its item + 1
    const int64_t* gid_incl;   // [n] its group + 1
    int64_t cut;               // points (a multiple of 16) after which a group of equal keys is cut into a group of its own
    int64_t* scal;             // [0] valid points (in), [1] items, [3] most items of a group, [6] groups (out)
    int64_t* grp_first;        // [groups]
    int32_t* grp_items;        // [groups]
    int64_t n_valid;           // k_sourcewise_scan_fill: the sorted positions in front of the rejected points
    int64_t* rowoff;           // [items][NR]
    double* coef;              // [items][NR][16]
    int64_t* item_cnt;         // [items]
    int32_t* item_tiles;       // [items]
    double* slot_lg;           // [items][16]
    int64_t* perm;             // [items][16] the point of the slot, -1: padding
};

// k_sourcewise_gather (bi_k_sourcewise_nonempty.h): the compacted copies of the datasets t0 + blockIdx.z
struct SourcewiseGatherArgs {
    const double* ps;          // [rows][Bp] the dense rows
    const int32_t* nz_idx;     // the datasets' lists back to back, ascending bins
    const double* nz_n;        // ... and their counts
    const int64_t* nz_off;     // [T + 1]
    const int64_t* ne_off;     // [T]
    const int64_t* ne_np;      // [T]
    const int64_t* ne_cnt_off; // [T]
    double* out_ps;
    double* out_cnt;
    int64_t Bp, rows, t0;
};

// k_sourcewise_expect (bi_k_sourcewise.h): the descriptors of FactoredArgs (rowoff, coef [items][NR][1 + EM], rates, e; no
// counts, partials or chain) and where the expectation goes
struct SourcewiseExpectArgs {
    FactoredArgs f;
    double* out;               // [items][R][Bp]: R = 1 (mu_b) or S (r_s tau_s,b); the pad bins behind B are written too (zeros)
    int64_t Bp;
    int R;
};

// the analysis space of the event simulators (k_sim_*, bi_k_misc.h; sim_one_event, bi_k_draw.h; bi_k_sourcewise_sim.h)
struct SimArgs {
    int k;                       // analysis dimensions
    int S;
    int n_edges[kMaxDim];
    int edge_off[kMaxDim];
    int64_t stride[kMaxDim];     // bins (C order) per step along the axis
};

// k_sourcewise_pmf (bi_k_sourcewise_sim.h): FactoredArgs' order-0 descriptors of a sub-batch of truths and where their pmf rows go
struct SourcewisePmfArgs {
    FactoredArgs f;
    SimArgs sim;
    const double* edges;       // the bin edges of every axis back to back
    double* out;               // [items][S][B] max(tau_s,b, 0) vol_b
    int64_t B;
};

// the other kernels of bi_sourcewise_simulate_event_toys (bi_k_sourcewise_sim.h): T toys, toy t at truth[t], its number in the
// seed's ensemble toy0 + t
struct SourcewiseSimArgs {
    SimArgs sim;
    const double* edges;
    const double* rates;       // [H][rate_stride] r_s of every truth
    const int32_t* truth;      // [T]
    int64_t* n;                // [T][S] events per (toy, source)
    int64_t* room;             // [T + 1] columns a toy takes (whole tiles, at least one); the last entry 0
    const int64_t* set_first;  // [T + 1] the exclusive prefix sums of room
    int64_t* first;            // [T][S + 1] first column of (toy, source); the last entry the end of the toy's events
    int64_t T, toy0;
    uint64_t seed;
    int rate_stride;
    // k_sourcewise_sim_events: the columns [col0, col0 + ncols) of the toys [t0, t0 + nt), whose truths start at h0
    const double* cdf;         // [truths of the sub-batch][S][B] running sums of the pmf rows
    int64_t B, col0, ncols, t0, nt, h0;
    int64_t cols;              // columns of the whole call: the row length of coords
    double* coords;            // [k][cols]
    int32_t* source;           // [cols]
};

// k_morph_expect (bi_k_gof.h)
struct ExpectArgs {
    const double* ps;          // [rows][Bp] the dense template tensor
    const int64_t* rowoff;     // [items][NS] element offsets of the rows, row k = (corner, source): k = corner * S + source
    const double* coef;        // [items][NS] a_k
    double* out;               // [items][R][B]
    int64_t B;
    int NS;
    int S;                     // sources: group r of a per-source call holds the rows k = r, r + S, ...
    int R;                     // groups per item: 1 (every row) or S
};

// k_morph_coarse / k_coarse_finish (bi_k_coarse.h)
struct CoarseArgs {
    const double* ps;          // [rows][Bp] the dense template tensor (or the dense counts [T][Bp])
    const int64_t* rowoff;     // [items][NS] element offsets of the rows, k = corner * S + source
    const double* coef;        // [items][NS] a_k (k_morph_coarse_jac<G>: [items][NS][G], and R = G)
    const int64_t* row_off;    // [CR + 1] the fine rows of coarse row q are row_list[row_off[q] .. row_off[q + 1])
    const int32_t* row_list;
    const int32_t* xb;         // [Cx + 1] fine columns [xb[j], xb[j + 1]) make coarse column j; xb[0] = x_lo
    double* partial;           // [items][R][CR][nsplit][Lx]
    double* out;               // [items][R][CR][Cx]
    int64_t L;                 // fine bins of the last axis: fine bin b = r L + x
    int64_t x_lo, Lx;          // the fine columns that belong to a cell
    int64_t CR, Cx;
    int64_t n_out;             // items R CR Cx
    int NS, S, R;              // R groups of rows per item: 1 (every row) or S (group r holds the rows k = r, r + S, ...)
    int nsplit;                // shares a coarse row's fine rows are dealt into
    int n_xt;                  // x-tiles of TX = 1 << tx_shift lanes
    int tx_shift;              // 6, 7 or 8; TY = 256 >> tx_shift fine rows of a share are in flight at a time
    int wide;                  // the finish kernel: 0 one thread per cell, 1 one block per cell (k_coarse_finish_wide)
};

// k_sourcewise_coarse (bi_k_sourcewise_coarse.h): the descriptors of FactoredArgs (rowoff, coef [items][NR][1 + EM], rates, e) and
// the binning, geometry and partial sums of CoarseArgs (g.ps, g.rowoff, g.coef, g.NS and g.S are not read; g.R = 1 or S)
struct SourcewiseCoarseArgs {
    FactoredArgs f;
    CoarseArgs g;
};

// k_sourcewise_coarse_jac (bi_k_sourcewise_coarse_jac.h): the same with FacBatch's descriptors of order 1 (coef's columns 1 .. EM
// are read too) and the map from k_morph_factored's result slots ([0] mu, [1 + s] tau_s, [1 + SC + s EM + j] ups_s,j) to the
// g.R = K = 1 + S + sum_s e_s groups that are written; -1: a padding slot (s >= S or j >= e_s), never written
constexpr int kCoarseJacSlots = 33;          // 1 + 8 (1 + 3)
struct SourcewiseCoarseJacArgs {
    FactoredArgs f;
    CoarseArgs g;
    signed char group[kCoarseJacSlots];
};

// k_coarse_list (bi_k_coarse.h): the non-empty-bin lists of n datasets into 64-bit integer tables [n][C]
struct CoarseListArgs {
    const int32_t* nz_idx;     // fine bin of every entry
    const double* nz_n;        // ... and its count (an integer by construction)
    const int64_t* nz_off;     // [T + 1]
    const int64_t* dataset;    // [n]
    const int32_t* row_map;    // [NR]
    const int32_t* x_map;      // [L]
    unsigned long long* table; // [n][C], zeroed
    int64_t L, Cx, C;
};

// k_real_expect (bi_k_real.h)
struct RealExpectArgs {
    const double* ps;          // [rows][Bp] the dense template tensor
    const int64_t* rowoff;     // [items][NS] element offsets of the rows, row k = (corner, source)
    const double* coef;        // [items][NS] a_k
    double* out;               // [items][Bp] rows of the real-valued store (the padding bins are zeroed by the caller)
    int64_t* bad;              // [items] 0, or 1 + a bin whose expectation is negative or nan
    int64_t B, Bp;
    int NS;
};

// ---- toy-MC evaluation (bi_k_toys.h; the host half is bi_toys.h, which sizes its lists and buffers by the same constants) ----
constexpr int kDotTile = 8192;               // bins per tile of the single-point lists: 64 KB of LDS
constexpr int kDotTileMulti = 4096;          // bins per tile of the multi-point lists: 4096 x 4 points x 8 B = 128 KB of LDS
constexpr int kDotPad = 64 * 2 + 16;         // entries behind the lists that the read-ahead may touch (read, masked, never used): the largest of the variants
constexpr int kDotGroup = 8;                 // datasets per block of the dense row kernel k_dataset_dot
constexpr int kPartBlock = 32;               // datasets per block of the multi-point per-(tile, dataset) partial sums

// k_morph_logmu_desc: the descriptors of one point in the kernel arguments
struct PointDesc {
    int64_t rowoff[kMaxSingleStreams];
    double coef[kMaxSingleStreams];
};

// k_dataset_dot_multi: sum mu of the points of a group of passes, added up by the first block of every pass
struct MuTotals {
    const int32_t* colmap;        // [passes of the group][PP][2] = {work item of the log mu kernel, output row} (-1: no point)
    const double* partial;        // [items][nmu][GC]
    const unsigned* flags;
    int nmu, GC;
    double* tot;
    unsigned* flag;
};

// k_csr_tile_offsets, k_tm_counts, k_tm_scatter: the tile-major copy of the non-empty-bin lists
struct TileListArgs {
    const int32_t* nz_idx;        // the dataset-major lists
    const double* nz_n;
    const int64_t* nz_off;        // [T + 1]
    int32_t* tile_off;            // [T][n_tl + 1] first entry of every tile within a dataset's list
    int64_t* cnt;                 // [n_tl T + 1] padded length of every (tile, dataset) run
    const int64_t* tm_off;        // [n_tl T + 1] their exclusive sum
    void* entries;                // the tile-major entries, `width` bytes each, pre-filled with padding entries
    int* bad;                     // set to 1 where a count does not fit the entry format
    int64_t T;
    int n_tl, tile_shift, width;
};

// k_dataset_dot_tiled / k_dataset_dot_multi
struct ToyDotArgs {
    const void* entries;          // tile-major lists and their offsets [n_tl][T]
    const int64_t* off;
    int64_t T;
    int n_tl;
    const double* lm;             // log mu [Bp], or [passes][PP][Bp]
    int64_t B, Bp, t0, n;
    double* partial;
};

// k_dataset_finish / k_dataset_finish_tiled / k_dataset_finish_multi
struct ToyFinishArgs {
    const double* partial;
    int nbx;                      // partial sums per dataset (tiles)
    int64_t t_stride, b_stride;   // k_dataset_finish: partial[t * t_stride + b * b_stride]
    const double* mu;             // the log mu pass's block partials [nmu]; multi: MuTotals::tot [passes][PP]
    const unsigned* mu_flags;
    int nmu;
    const int32_t* colmap;        // multi: [passes][PP][2]
    const double* lgsum;
    int64_t t0, n;
    double* out;
    int64_t out_stride;           // multi: out[row * out_stride + dataset]
    unsigned* blocks_done;        // the tiled and multi forms: see publish_when_last
    unsigned long long* done;
    unsigned long long seq;
};

// The free-variable map of the native loops (fit, sampler, grid): which variable is which model parameter, the other settings
// of every entry (problem, ensemble, dataset entry) and the staging rows, in the layouts bi_eval_grad and the resident planner
// read.  The device loops hold device pointers, the fit's objective host pointers.  Its host side is bi_varmap.h.
struct VarMap {
    int F, d, S;               // variables, shape parameters and sources of the model
    const int32_t* var_kind;   // [F] 0: shape parameter var_index, 1: rate multiplier of source var_index
    const int32_t* var_index;
    const double* z0;          // [E][d]  the entries' other shape settings
    const double* scale0;      // [E][S]  ... rate scales of the sources whose multiplier is no variable
    const double* unit;        // [E][S]  rate scale per unit multiplier
    const int64_t* dataset;    // [E] or NULL
    double* z_dev;             // [n][d]  the points
    double* rs_dev;            // [n][S]
    int64_t* ds_dev;           // [n]
};

// point i = entry e with variable j at coord(j); coord is called once per variable, in order.  The product is one rounded
// multiply on both sides (the host is compiled without contraction).
template <class Coord>
__host__ __device__ __forceinline__ void varmap_write_point(const VarMap& m, int64_t i, int64_t e, Coord coord) {
    for (int k = 0; k < m.d; ++k) m.z_dev[i * m.d + k] = m.z0[e * m.d + k];
    for (int s = 0; s < m.S; ++s) m.rs_dev[i * m.S + s] = m.scale0[e * m.S + s];
    for (int j = 0; j < m.F; ++j) {
        const double y = coord(j);
        const int k = m.var_index[j];
        if (m.var_kind[j] == 0) m.z_dev[i * m.d + k] = y;
#ifdef __HIP_DEVICE_COMPILE__
        else m.rs_dev[i * m.S + k] = __dmul_rn(y, m.unit[e * m.S + k]);
#else
        else m.rs_dev[i * m.S + k] = y * m.unit[e * m.S + k];
#endif
    }
    m.ds_dev[i] = m.dataset ? m.dataset[e] : 0;
}

// k_stretch_propose / k_stretch_accept (bi_k_sampler.h): one half-step of the ensemble sampler; every pointer is device memory
struct StretchArgs : VarMap {  // the variables (F), the ensembles' settings, the proposals' rows
    int64_t E;                 // ensembles
    int W;                     // walkers per ensemble
    int h;                     // the half that moves: walkers [h W/2, (h + 1) W/2); -1: stage every walker's own position (the start)
    int64_t t;                 // step
    int64_t first_ensemble;    // ensemble e of the call is ensemble first_ensemble + e of the seed's stream
    uint32_t k0, k1;           // seed, low and high word
    double a;                  // stretch scale
    const double* lo;          // [F]
    const double* hi;
    double* x;                 // [E][W][F] the walkers
    double* ll;                // [E][W]    their log likelihoods
    int64_t* n_accepted;       // [E][W]
    const double* ll_prop;     // [n]   the proposals' log likelihoods and status words (accept)
    const int32_t* st_prop;
    double* chain;             // [E][W][F] row of step t
    double* chain_ll;          // [E][W]
    // Gaussian constraint terms on the variables (bi_sample_stretch_gauss): `ll` above then holds the log density ll + p.
    // prior_sigma NULL: no term on any variable; prior_const NULL: 0; both NULL: the kernels do what they did without terms
    const double* prior_mean;  // [F]
    const double* prior_sigma; // [F]  +inf: no term on that variable
    const double* prior_const; // [E]
};

// k_grid_points / k_grid_reduce / k_grid_finish (bi_k_grid.h): one chunk of a tensor-product grid; every pointer is device memory
constexpr int kGridMaxVars = 16;

struct GridArgs : VarMap {     // the variables (F), the entries' settings, the chunk's rows
    int64_t g0, n;             // the chunk: grid points [g0, g0 + n)
    int64_t R, GK;             // points of a cell (product of the reduced node counts), points of a dataset entry (K R)
    int n_keep;                // kept variables (the first n_keep)
    int32_t n_nodes[kGridMaxVars];   // nodes of variable j
    int64_t node_off[kGridMaxVars];  // where they start in nodes / term / logw
    int64_t stride[kGridMaxVars];    // grid points per step of variable j: i_j = (g / stride_j) mod n_j
    const double* nodes;       // concatenated
    const double* term;        // concatenated or NULL
    const double* logw;        // concatenated or NULL
    double* p;                 // [n] or NULL (no term): the additive terms of the points
    double* q;                 // [n] or NULL (no logw)
    // the reduction
    const double* ll;          // [n]  the chunk's result vector
    const int32_t* st;         // [n]  its status words, or NULL (self-test)
    int64_t cell0, n_cells;    // the cells the chunk touches: [cell0, cell0 + n_cells)
    int cpb;                   // cells per block: 1 (four waves per cell) or 4 (one wave per cell)
    double* m;                 // [cells] per-cell state: running maximum of u
    double* s;                 // [cells] ... sum of exp(u - m)
    double* best;              // [cells] ... maximum of t
    int64_t* arg;              // [cells] ... smallest r that attains it, -1: none
    int64_t* n_excl;           // [cells] ... excluded points
    int32_t* nan_flag;         // [cells] ... a nan with status 0 was seen
    // k_grid_finish
    int64_t cells;
    double* out_lm;            // [cells]
    double* out_prof;          // [cells]
    int64_t* out_arg;          // [cells]
};

namespace {

// ------------------------------------------------------------------------------------------
// device code
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// exchange for a transposing reduction: returns a' * b' where a' = [a | b](lower halves / even rows), b' = the others
#define BI_SWAP_MUL(SWAP, a, b, out)                                                                               \
    do {                                                                                                           \
        const unsigned long long ua = __double_as_longlong(a), ub = __double_as_longlong(b);                       \
        const auto lo = SWAP((unsigned)ua, (unsigned)ub, false, false);                                            \
        const auto hi = SWAP((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false);                            \
        out = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]) *                                    \
              __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);                                     \
    } while (0)
// (used by k_scan_sorted and k_grad_mfma: four items' products over the four 16-lane rows of a wave, row q keeping item q --
//  BI_SWAP_MUL(permlane32_swap, p0, p2, x); BI_SWAP_MUL(permlane32_swap, p1, p3, y); BI_SWAP_MUL(permlane16_swap, x, y, P))

// a lane's double as a wave-uniform (scalar) value
__device__ __forceinline__ double lane_value(double v, int src_lane) {
    const unsigned long long u = __double_as_longlong(v);
    return __longlong_as_double(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(u >> 32), src_lane) << 32) |
                                (unsigned)__builtin_amdgcn_readlane((int)u, src_lane));
}

__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_down(v, off, 64);
    return v;
}

// Natural logarithm for the per-bin terms, table-driven (the scheme of Tang's table-driven log as used by modern
// libms, laid out for this hardware): x = 2^k z with z in [0.6875, 1.375); the 7 leading mantissa bits pick a
// subinterval with centre c from a 128-entry {1/c, log c hi, log c lo} table held in LDS (bi_log_table.h); then
//     log x = (k ln2_hi + log c_hi) + ( r + (r^2 P(r) + k ln2_lo + log c_lo) ),   r = z / c - 1   (one fma, |r| <= 2^-7)
// where the first bracket is EXACT in one fma (ln2_hi on a 2^-37 grid, log c_hi on a 2^-43 grid), P is log1p's Taylor
// polynomial through r^8, and the sum of the first bracket and r is carried with its rounding error.  16 fp64
// instructions, one conversion and 6 integer ones per call (round 1: 19 + 1 + 6: it also had to recover the rounding of an
// inexact k ln2 + log c), two LDS reads, no division and no transcendental-rate instruction; worst error 0.70 ulp, 98.6 %
// of results correctly rounded
// (tools/gen_log_table.py, tests/test_gpu_golden.py::test_device_log_accuracy).  On a chip where no vector instruction
// executes beside an fp64 MFMA, the logarithm's instruction count is what bounds scans over dense data.
// Every kernel that calls bin_log fills the LDS table first: log_table_load(), or the overlapped form in morph_tiles.
__shared__ double4 s_log_table[128];

__device__ __forceinline__ void log_table_load() {
    if (threadIdx.x < 128) s_log_table[threadIdx.x] = kLogTable[threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ bool pos_normal(double x) { return __builtin_amdgcn_class(x, 0x100); }
// Factors of the product forms of sum n log mu (k_scan_mfma): up to eight of them, each above 2^-127, multiply to at least
// 2^-1016 -- a normal number -- in any grouping; a comparison with it is false for nan, zero and negative numbers too.
constexpr double kProdFloor = 0x1p-127;

// the core: x must be a positive normal number (anything else gives a meaningless but harmless value);
// k_adjust is added to the binary exponent
__device__ __forceinline__ double log_core(double x, int k_adjust) {
    const unsigned long long ix = __double_as_longlong(x);
    const int hi = (int)(ix >> 32);
    const int t = hi - 0x3FE60000;                  // bits(x) - bits(0.6875), high word
    const int k0 = t >> 20;
    const int k = k0 + k_adjust;
    // high word of z = hi - (k0 << 20), as ONE 24-bit multiply-add (|k0| <= 2^10, 2^20 < 2^23; written as an instruction
    // because the compiler turns the product back into a mask and a subtraction)
    int zhi;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(zhi) : "v"(k0), "s"(-(1 << 20)), "v"(hi));
    const double z = __longlong_as_double(((unsigned long long)(unsigned)zhi << 32) | (ix & 0xFFFFFFFFull));
    const double4 e = s_log_table[(t >> 13) & 127];
    const double kd = (double)k;
    const double r = fma(z, e.x, -1.0);
    const double w = fma(kd, kLn2Hi, e.y);         // exact
    const double tail = fma(kd, kLn2Lo, e.z);
    double p = fma(r, -1.0 / 8.0, e.w);            // e.w = 1/7: arrives in a vector register with the table entry
    p = fma(r, p, -1.0 / 6.0);
    p = fma(r, p, 1.0 / 5.0);
    p = fma(r, p, -1.0 / 4.0);
    p = fma(r, p, 1.0 / 3.0);
    p = fma(r, p, -0.5);
    const double q = fma(r * r, p, tail);
    // w + r with its rounding error kept (|w| >= |r| wherever w != 0: k != 0, or a subinterval away from the two that touch
    // 1): where log c and r nearly cancel -- arguments a little off 1 -- the plain r + q would cost up to an ulp
    const double h = w + r;
    const double err = (w - h) + r;
    return h + (err + q);
}

// for arguments known to be positive normal numbers
__device__ __forceinline__ double bin_log_fast(double x) { return log_core(x, 0); }

// for any argument, still without a branch: denormals are scaled by 2^54 first; log 0 = -inf, log of a negative
// number or nan = nan, log inf = inf (numpy.log's values)
__device__ __forceinline__ double bin_log(double x) {
    const bool tiny = x < 2.2250738585072014e-308;
    double y = log_core(tiny ? x * 18014398509481984.0 : x, tiny ? -54 : 0);
    if (x == 0.0) y = -__builtin_inf();
    if (!(x >= 0.0)) y = __builtin_nan("");
    if (x == __builtin_inf()) y = x;
    return y;
}

template <bool NT>
__device__ __forceinline__ double2 stream_load(const double* p) {
    if constexpr (NT) {
        // streamed-once data: nontemporal hint (global_load_dwordx4 ... nt) keeps it from displacing L2 / MALL lines
        double2 v;
        v.x = __builtin_nontemporal_load(p);
        v.y = __builtin_nontemporal_load(p + 1);
        return v;
    } else {
        return *reinterpret_cast<const double2*>(p);
    }
}

// ---- the packed template rows: a lane's two bins of one chunk (the layout is described at kPkChunk) ----
// What the three loads bring, nothing decoded yet: a batch of rows keeps all of its loads in flight before the first decode.
struct PkRaw {
    unsigned lo0, lo1;         // mantissa bits 0..31 of the two bins
    unsigned mid;              // bits 32..47 of both
    unsigned top;              // bits 48..51 | code << 4 of both (low half-word)
};

// chunk: the tile's number in ps, (row's element offset >> 9) + tile -- wave-uniform.  Buffer loads: the chunk's address stays
// in scalar registers (a descriptor per chunk), the three lane offsets are the same for every row, so a row costs no vector
// address arithmetic; and the descriptor's 3584 bytes bound every access to the chunk.
template <bool NT>
__device__ __forceinline__ PkRaw pk_load(const uint8_t* __restrict__ pk, int64_t chunk) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pk + chunk * kPkChunk), 0, kPkChunk, 0x00020000);
    constexpr int aux = NT ? 2 : 0;                                  // (the nontemporal hint the fp64 rows carry)
    const auto lo = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)threadIdx.x * 8, 0, aux);
    PkRaw r;
    r.lo0 = lo[0];
    r.lo1 = lo[1];
    r.mid = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)threadIdx.x * 4, kPkMidOff, aux);
    r.top = __builtin_amdgcn_raw_buffer_load_b16(rsrc, (int)threadIdx.x * 2, kPkTopOff, aux);
    return r;
}

// the word that holds a chunk's base (two bases per word: a scalar load), and (base - 1) << 20 from it -- wave-uniform
__device__ __forceinline__ unsigned pk_base_word(const uint32_t* __restrict__ pk_base, int64_t chunk) { return pk_base[chunk >> 1]; }
__device__ __forceinline__ unsigned pk_exp_add(unsigned word, int64_t chunk) {
    return (((word >> (((unsigned)chunk & 1u) * 16u)) & 0xffffu) - 1u) << 20;
}

// the stored doubles, bit for bit.  High word = [mid half-word | top byte << 16], which has the code in bits 20..23: a non-zero
// code c becomes the exponent base + c - 1 by adding (base - 1) << 20; code 0 is +0.0, all bits 0.  `add` stays a scalar operand.
__device__ __forceinline__ double2 pk_decode(const PkRaw& r, unsigned add) {
    unsigned hx = __builtin_amdgcn_perm(r.top, r.mid, 0x0c040100u);
    unsigned hy = __builtin_amdgcn_perm(r.top, r.mid, 0x0c050302u);
    hx = hx ? hx + add : 0u;                 // (code 0 <=> every stored bit of the value is 0)
    hy = hy ? hy + add : 0u;
    double2 v;
    v.x = __longlong_as_double(((unsigned long long)hx << 32) | r.lo0);
    v.y = __longlong_as_double(((unsigned long long)hy << 32) | r.lo1);
    return v;
}

// Poisson log-pmf without the data-only lgamma(n+1) term, scipy semantics
// (scipy/stats/_distn_infrastructure.py logpmf + _discrete_distns.py poisson._logpmf):
//   mu not >= 0 (negative or nan) or n nan -> nan
//   n negative or non-integer             -> -inf
//   else xlogy(n, mu) - mu                  (xlogy(0, mu) = 0, also for mu = 0)
__device__ __forceinline__ double poisson_term(double n, double mu) {
    double t;
    if (n > 0.0) {
        t = n * bin_log(mu) - mu;  // mu = 0 -> -inf; mu < 0 -> nan
    } else {
        t = -mu;
    }
    if (!(mu >= 0.0) || n != n) t = __builtin_nan("");
    else if (n < 0.0 || n != floor(n)) t = -__builtin_inf();
    return t;
}

// The same term without a branch, for unrolled loops (the compiler can then batch the table reads of many terms).
// Only valid where n > 0 implies that mu is a positive normal number -- the caller checks that for the whole wave
// (needs_checked_term) and takes poisson_term otherwise.  Same operations, same bits.
__device__ __forceinline__ bool needs_checked_term(double n, double mu) { return n > 0.0 && !pos_normal(mu); }

__device__ __forceinline__ double poisson_term_fast(double n, double mu) {
    const double lg = bin_log_fast(mu);            // not used where n <= 0
    double t = (n > 0.0) ? n * lg - mu : -mu;
    if (!(mu >= 0.0) || n != n) t = __builtin_nan("");
    else if (n < 0.0 || n != floor(n)) t = -__builtin_inf();
    return t;
}

// ... for a bin column in which no lane has n > 0
__device__ __forceinline__ double poisson_term_nolog(double n, double mu) {
    double t = -mu;
    if (!(mu >= 0.0) || n != n) t = __builtin_nan("");
    else if (n < 0.0 || n != floor(n)) t = -__builtin_inf();
    return t;
}

// Beeston-Barlow roots, evaluated in the reference's own operation order without FMA
// contraction (blueice/likelihood.py:693-712) so that the sign tests behind its two asserts
// see the same rounding.
__device__ __forceinline__ void bb_roots(double a, double p, double U, double d, double& r1, double& r2) {
#pragma clang fp contract(off)
    double U2 = U * U, p2 = p * p, a2 = a * a, d2 = d * d;
    double disc = U2 * p2 + 2 * U2 * p + U2 + 2 * U * a * p2 + 2 * U * a * p - 2 * U * d * p2 - 2 * U * d * p +
                  a2 * p2 + 2 * a * d * p2 + d2 * p2;
    double lead = -U * p - U + a * p + d * p;
    double den = 2 * p * (p + 1);
    double sq = sqrt(disc);
    r1 = (lead - sq) / den;
    r2 = (lead + sq) / den;
}

// ---- in-launch finishing through mailboxes -------------------------------------------------------------------
// A work item's blocks post their partial sums into 8-byte mailbox slots and EXIT; the item's last block in dispatch
// order (blockIdx.x == gridDim.x - 1: every sibling was dispatched before it, so they are running or done) collects
// them, sums them in block order (fixed order => bitwise reproducible) and writes the result -- what the k_finish
// launch did, without the launch.  A slot is one naturally aligned 8-byte granule written by ONE system-scope
// (sc0 sc1, write-through) store and read with system-scope loads (MI355X_MICROARCH.md "Valid forms": sc0 sc1
// stores and loads on both sides need no fence); "empty" is a signalling-NaN bit pattern that no arithmetic result
// can have (posted NaNs are canonicalised), and the collector puts it back as it takes a value, so the slots are
// empty again when the launch ends.  Posting costs a block one store and no wait: round 2 first tried arrival
// tickets (publish, drain, returning atomics) and measured +27 us on a 300 us launch -- every one of 8192 blocks
// held its CU slot for ~4 us of round trips -- and round 1's release fence per block was worse still.
// The collector's wait is bounded (LaunchArgs::mail_timeout ticks of the 100 MHz wall clock, 2 s by default): if a value never arrives it gives
// up, reports BI_ST_INTERNAL and the result is nan -- no wave can spin forever.
constexpr unsigned long long kMailEmpty = 0x7FF4B10E1CE00001ull;

__device__ __forceinline__ void mail_post(double* slot, double v) {
    if (v != v) v = __builtin_nan("");                                   // never the "empty" pattern
    __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// take the value out of a slot (waiting for it), leave the slot empty; *late is set if the wait ran out
__device__ __forceinline__ double mail_take(double* slot, long long deadline, bool* late) {
    unsigned long long bits;
    for (;;) {
        bits = __hip_atomic_load(reinterpret_cast<unsigned long long*>(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (bits != kMailEmpty) break;
        if ((long long)wall_clock64() > deadline) { *late = true; return __builtin_nan(""); }
        __builtin_amdgcn_s_sleep(4);
    }
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot), kMailEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return __longlong_as_double(bits);
}

// The collector's inner step: the values of slots q0, q0 + stride, ... (up to 4, below `total`) added to s in that order.
// The four loads go out together -- a system-scope load takes about a microsecond, and by the time the last block
// collects nearly every sibling has posted, so polling one slot after the other would only add their latencies up
// (measured on a one-item launch of 1954 blocks x 8 columns: 86 us with sequential takes, the kernel proper 45).
__device__ __forceinline__ double mail_take4(double* mail, int q0, int stride, int total, double s, long long deadline, bool* late) {
    unsigned long long bits[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = q0 + u * stride;
        bits[u] = q < total ? __hip_atomic_load(reinterpret_cast<unsigned long long*>(mail + q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                            : 0ull;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = q0 + u * stride;
        if (q >= total) break;
        if (bits[u] == kMailEmpty) {
            s += mail_take(mail + q, deadline, late);            // not there yet: wait for this one
        } else {
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(mail + q), kMailEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            s += __longlong_as_double(bits[u]);
        }
    }
    return s;
}

// Beeston-Barlow status bits travel through one word per result slot: a block that has any ORs them in BEFORE it
// posts its partial (returning atomic: performed when it returns), the collector swaps the word for 0 after the
// partials have arrived
__device__ __forceinline__ void flags_post(unsigned* word, unsigned f) {
    if (f) {
        const unsigned old = __hip_atomic_fetch_or(word, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("" ::"v"(old) : "memory");                           // the post below must not be hoisted above the return
    }
}
__device__ __forceinline__ unsigned flags_take(unsigned* word) {
    return __hip_atomic_exchange(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the post of a block's partial sum with the two injected faults (both -1 in production: two scalar compares per block)
__device__ __forceinline__ void mail_post_checked(const LaunchArgs& a, double* slot, double v) {
    if ((int)blockIdx.x == a.skip_post) return;
    if ((int)blockIdx.x == a.late_post) {
        const long long until = (long long)wall_clock64() + 2 * a.mail_timeout;
        while ((long long)wall_clock64() < until) __builtin_amdgcn_s_sleep(32);
    }
    mail_post(slot, v);
}

// sum of a double over the 4 DPP rows of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48): one half-row exchange and one half-wave
// exchange (v_permlane16_swap / v_permlane32_swap, gfx950), every lane ends up with the total
__device__ __forceinline__ double rows4_sum(double v) {
#define BI_SWAP_ADD(SWAP)                                                                                          \
    do {                                                                                                           \
        const unsigned long long u = __double_as_longlong(v);                                                      \
        const auto lo = SWAP((unsigned)u, (unsigned)u, false, false);                                              \
        const auto hi = SWAP((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);                              \
        v = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]) +                                      \
            __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);                                       \
    } while (0)
    BI_SWAP_ADD(__builtin_amdgcn_permlane16_swap);
    BI_SWAP_ADD(__builtin_amdgcn_permlane32_swap);
#undef BI_SWAP_ADD
    return v;
}

}  // namespace
