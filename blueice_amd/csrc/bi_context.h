// bi_context.h -- the context / plan objects behind the opaque C handles, error and device-memory helpers.
#pragma once

struct bi_ctx;

constexpr int kThreads = 256;           // 4 wave64 per block
constexpr int kBinsPerThread = 2;       // one 16-byte load per stream per lane
constexpr int kTile = kThreads * kBinsPerThread;  // 512 bins = 4 KiB per stream per block tile
constexpr int kMaxDim = 8;              // shape parameters
constexpr int kMaxG = 16;               // points per cell pass
constexpr int kFacMaxDim = 32;          // source-wise models (bi_factored.h): shape axes,
constexpr int kFacMaxSources = 8;       // ... sources,
constexpr int kFacMaxOwn = 3;           // ... and axes one source responds to

// (the library is several translation units -- one per heavy kernel family, compiled in parallel: types that cross them
//  sit at global scope, state that must exist once is `inline`)
inline thread_local std::string g_create_error;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    struct bi_ctx* owner = nullptr;    // context whose recycle cache takes the buffer back on dev_free
    bool view = false;                 // a window into somebody else's allocation: dev_free only forgets it
};

struct bi_plan {
    int64_t P = 0;
    struct Class {
        int G = 0;
        int64_t n_items = 0;
        int nbx = 0;
        DevBuf rowoff, coef, aux, item_cnt, item_tiles, perm, slot_lg, partial, pflags;
        DevBuf rowoff_full;        // split scans: offsets of the FULL rows of every item (validity pass)
    };
    std::vector<Class> classes;
    DevBuf bad_idx;            // points answered on the host side with -inf
    int64_t n_bad = 0;
    DevBuf nan_idx;            // ... and with nan (infinite rates whose expectation is nan somewhere, or meets data)
    int64_t n_nan = 0;
    DevBuf out, status;        // internal result buffers [P]
    std::vector<int32_t> h_status;
    int64_t epoch = 0;         // ctx->epoch at creation: a plan dies with the model / data it was made for
    DevBuf slab;                  // transient small plans: every descriptor array is a view into this one buffer
    bool host_results = false;    // ... and out / status are views into the context's pinned block
    bool use_scan = false;        // evaluated by the matrix-core scan kernel (groups of items per cell)
    int64_t n_groups = 0;
    int scan_cb = 4;              // its strip width in 16-bin blocks
    DevBuf grp_first, grp_items;
    std::vector<int64_t> h_grp_first;   // host copies of cut group tables (device planner: their upload is asynchronous)
    std::vector<int32_t> h_grp_items;
    int bb_kgt = 0;               // Beeston-Barlow batch on the matrix cores (k_scan_bb<bb_kgt>): items of 16 points, group tables
    bool valid = false;           // split dense scan: classes hold the non-empty-bin pass, k_scan_valid checks every bin
    int valid_nslots = 0;         // its waves per group
    DevBuf bad;                   // [items][16] flags it raises
    bool shared = false;          // a share of a scan dealt over several contexts (plan_points_device, share_world > 1): results
    int share_world = 1;          // come out in sorted order, out[0 .. share_hi - share_lo); sorted_idx [P] maps sorted positions
    int64_t share_lo = 0, share_hi = 0, n_valid = 0;   // back to the caller's point indices
    DevBuf sorted_idx;
    DevBuf keep_z, keep_rs;       // gradient batches on the matrix cores: the points' z / rate_scale stay on the device for the finish kernel
    int64_t max_group_items = 0;  // ... the largest number of work items a (cell, dataset) group holds (scan plans: after chunk_groups)
    int max_item_tiles = 0;       // ... and the tiles of the longest rows
    bool device_planned = false;  // built by plan_points_device: rejected points are found through the status array
    bool no_reuse = false;     // no anchor model is touched by two items of the plan
    bool sparse = false;       // rows / counts refer to the compacted (non-empty-bin) copies
    bool narrow = false;       // every dataset the plan's items refer to has an exact narrow copy of its counts (decided when the plan is built)
    bool sorted = false;       // rows / counts refer to the count-sorted copy of all bins (dense-data scans, ensure_sorted_rows)
    bool by_count = false;     // the rows the scan kernel reads are ordered by count (sorted, or a count-sorted compacted copy)
    int64_t bytes = 0;         // algorithmic HBM bytes per run
    int64_t launches = 0;
};

struct bi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop{};
    std::string err;

    // model
    bool model_ready = false, model_open = false;
    int d = 0, S = 0;
    int64_t B = 0, Bp = 0, A = 0;
    std::vector<int> n_anchor;
    std::vector<std::vector<double>> grid;
    std::vector<int64_t> astride;  // anchor-index stride per axis
    std::vector<int> eff_axes;     // axes with >= 2 anchors
    int bb_source = -1;
    std::vector<int32_t> allow_neg;
    DevBuf ps, nm, nm_tot;
    std::vector<double> h_mus;     // [A][S]
    std::vector<double> h_nm_tot;  // [A]
    std::vector<char> anchor_set;

    // analysis space (bin edges) for device-side binning of events
    int space_k = 0;
    std::vector<int32_t> space_n_edges;
    DevBuf space_edges;

    // data
    bool unbinned = false;      // extended unbinned likelihood: rows are pdf values at the events
    double outlier = 0.0;
    bool ps_finite = true;
    bool data_ready = false;
    bool dense_counts = false;  // counts [T][Bp] resident (false for device-generated toys: CSR lists only)
    int64_t T = 0;
    // unbinned: the event sets held side by side on the event axis (bi_score_event_sets / bi_simulate_event_toys); set t is
    // columns [set_first[t], set_first[t] + set_n[t]), every first even.  With several sets T = n_sets and B = set_n[0]: what
    // knows nothing of sets evaluates set 0 (its columns start at 0; the tiles behind them are masked by B)
    int64_t n_sets = 1;
    std::vector<int64_t> set_first, set_n;
    int64_t n_set_launches = 0;                  // read-only: launches of k_morph_sets
    DevBuf counts, lgsum;
    std::vector<double> h_lgsum;
    // the narrow copy of the dense counts: [T][Bp] bytes beside the doubles, rebuilt by every writer of `counts`
    // (build_narrow_counts); the dense morph kernels stream it instead of the doubles for datasets it represents exactly
    DevBuf cnt8, cnt8_bad;                       // ... and [T] words, non-zero: the dataset has a value with no one-byte form
    std::vector<uint32_t> h_cnt8_bad;            // host copy of the flags (arrives with the upload's own synchronisation)
    bool cnt8_valid = false;                     // the copy matches `counts` (false: never read)
    int cnt8_all = -1;                           // every dataset has a narrow form: 1 / 0, -1 = not looked at yet
    int64_t narrow_counts = 1;                   // parameter: 0 = never read the narrow copy
    int64_t last_streamed_bytes = 0;             // read-only: bytes the last bi_run_plan streamed (plan bytes less 7 per bin of every item read narrow)
    int64_t n_narrow_launches = 0;               // read-only: morph launches that read the narrow copy
    // the packed shadow of the template rows: 7 bytes per value of ps in 3584-byte chunks and one exponent base per chunk
    // (build_packed_rows, at the end of every model upload); the dense value kernels stream it instead of ps when every chunk
    // of the model has a packed form
    DevBuf pk, pk_base, pk_bad;
    bool pk_valid = false;                       // the shadow matches `ps` and represents it exactly (false: never read)
    bool pk_skip = false;                        // the model being closed is an event tensor (score_events_impl): no shadow
    int64_t packed_rows = 1;                     // parameter: 0 = never build or read the shadow
    int64_t n_packed_launches = 0;               // read-only: morph launches that read the shadow
    int64_t last_packed_saved = 0;               // read-only: bytes the last bi_run_plan did NOT stream thanks to it (Bp per row and item)
    // read-only: the grid of the most recent k_morph_reduce / k_morph_single launch (gridDim.x blocks per item, gridDim.y items)
    // and whether it finished through the mailbox (0: k_finish, k_finish_single or the two-kernel fallback ran behind it)
    int64_t last_morph_nbx = 0, last_morph_items = 0, last_morph_fused = 0;
    // read-only: the device pieces the most recent per-point entry point cut its live items into on the host (the chunks of
    // run_item_chunks, summed over FacBatch::run's sub-batches and panels; the iterations of a bin-writing call's chunk loop)
    int64_t last_point_pieces = 0;

    // real-valued datasets [real_T][Bp] (bi_set_real_counts / bi_set_asimov_counts; bi_real.h): a store of its own beside
    // `counts`, read by bi_eval_real / bi_fit_batched_real only and released by a new model
    DevBuf real_counts;
    int64_t real_T = 0;

    // the source-wise (factored) model and its counts (bi_factored.h): one anchor grid per source over the axes that source
    // owns.  A store of its own beside the grid model: model_ready says nothing about it, no other entry point reads it, and
    // a new grid model leaves it alone.  Released by bi_factored_begin and bi_destroy.
    struct Factored {
        bool ready = false, open = false;
        int d = 0, S = 0;
        int64_t B = 0, Bp = 0;
        std::vector<std::vector<double>> grid;       // [d] anchors of every axis, ascending
        std::vector<int> n_own;                      // [S] e_s
        std::vector<int> own;                        // [S][kFacMaxOwn] the owned axes, ascending
        std::vector<int64_t> row_first;              // [S + 1] first row of source s in `ps` / `h_mus` (C order over its own axes)
        std::vector<int64_t> own_stride;             // [S][kFacMaxOwn] row stride of every owned axis
        std::vector<double> h_mus;                   // [rows]
        std::vector<char> row_set;                   // [rows] the anchor has been uploaded
        DevBuf ps;                                   // [rows][Bp], zero behind B
        int64_t T = 0;
        DevBuf counts;                               // [T][Bp], zero behind B
        std::vector<double> h_lgsum;                 // [T] sum_b lgamma(n_b + 1)
        // real-valued datasets (bi_sourcewise_set_real_counts / bi_sourcewise_set_asimov_counts; bi_sourcewise_real.h): a store
        // of its own beside `counts`, read by bi_eval_sourcewise_real / bi_fit_batched_sourcewise_real only
        int64_t real_T = 0;
        DevBuf real_counts;                          // [real_T][Bp], zero behind B
        int n_rows_point = 0;                        // rows one evaluation reads: sum_s 2^e_s
        int max_own = 0;                             // largest e_s
        // the device planner's copy of the geometry (k_sourcewise_plan, bi_sourcewise_plan.h): one slab of anchors, anchor_off,
        // n_own, own, own_stride, row_first, h_mus at geom_off[0 .. 7), uploaded by bi_factored_end; and of h_lgsum, uploaded
        // wherever that changes (fac_sync_lgsum)
        DevBuf geom, lgsum_dev;
        size_t geom_off[8] = {};                     // (the eighth part: h_rowsum, for the non-empty-bin form's planner)
        // the non-empty-bin form of the data (bi_sourcewise_build_nonempty; bi_sourcewise_nonempty.h): h_rowsum [rows], the total
        // R_{s,c} of every anchor row over all bins (long double, rounded once; bi_factored_set_anchor); per dataset t the
        // compacted copy ne_ps + ne_off[t] of all rows over its list, [rows][ne_np[t]] with ne_np[t] the list length padded to
        // whole tiles (at least one; zeros in the padding), and its compacted counts ne_cnt + ne_cnt_off[t] [ne_np[t]].  ne_tab:
        // the three tables back to back [3][T] for the device planner.  ne_max_nbx: the most blocks an item of any dataset takes.
        std::vector<double> h_rowsum;
        bool ne_ready = false;
        int64_t ne_bytes = 0;
        int ne_max_nbx = 1;
        std::vector<int64_t> ne_off, ne_np, ne_cnt_off;
        DevBuf ne_ps, ne_cnt, ne_tab;
        // the event store (bi_sourcewise_events.h): the pdf value of every event at every anchor row, ev_ps [rows][ev_cols]; set t
        // of ev_T at the columns [ev_first[t], ev_first[t] + ev_n[t]), every set padded to whole tiles (at least one; zeros in
        // the padding).  While it exists (ev_ready, or ev_open between _events_begin and _events_end) the context is an
        // unbinned source-wise likelihood: bi_eval_factored and the native fit read it, every other source-wise call refuses.
        bool ev_ready = false, ev_open = false;
        int64_t ev_T = 0, ev_cols = 0, ev_bytes = 0;
        double ev_outlier = 0.0;
        std::vector<int64_t> ev_first, ev_n;
        std::vector<char> ev_row_set;                // [rows] the row has been uploaded (bi_sourcewise_events_set_row)
        DevBuf ev_ps;
        // ev_tab: ev_first and ev_n back to back [2][ev_T] for the device planner's event variant (bi_sourcewise_plan.h), uploaded
        // when the store is finished (events_finish) and released with it.  ev_max_nbx: the most blocks an item of any set takes.
        DevBuf ev_tab;
        int ev_max_nbx = 1;
        // the events of a store drawn on the device (bi_sourcewise_simulate_event_toys; bi_sourcewise_sim.h): coordinates
        // [sim_k][ev_cols] and the source of every column (-1: padding) in the store's padded layout, sim_n events in all.  They
        // belong to that store: whatever releases or replaces it releases them (fac_drop_events).  sim_n < 0: none
        DevBuf sim_coords, sim_source;
        int sim_k = 0;
        int64_t sim_n = -1;
    } fac;
    int64_t sim_truth_chunk = 0;                 // bi_sourcewise_simulate_event_toys: truths per sub-batch (0: by the scratch bound)
    int64_t sim_part_ns[4] = {};                 // ... while profiling, the device time of its last call: layout, pmf + scans, events, scoring
    int64_t sourcewise_form = 1;                 // 0: source-wise evaluations read the dense store although the non-empty-bin form is built
    int64_t sourcewise_scan_timed = 3;           // profiling: bit 0 = the scan route's planner, bit 1 = its matrix-core launches are timed

    // the coarse binning of bi_set_coarse_binning (bi_coarse.h): tensor-product groups of fine bins, b = r L + x with L the
    // fine bins of the last analysis axis.  Released by a new model.
    struct Coarse {
        bool set = false;
        int64_t C = 0, CR = 0, Cx = 0;   // cells = coarse rows (leading axes) x coarse columns (last axis)
        int64_t L = 0, NR = 0;           // fine bins of the last axis, fine rows
        int64_t x_lo = 0, Lx = 0;        // the fine columns [x_lo, x_lo + Lx) that belong to a cell
        int64_t max_rows = 0;            // fine rows of the longest coarse row
        int64_t max_width = 0;           // fine columns of the widest column group
        DevBuf row_off, row_list;        // [CR + 1] int64, [rows] int32: the fine rows of every coarse row (left-out rows are absent)
        DevBuf xb;                       // [Cx + 1] int32: the column groups' boundaries
        DevBuf row_map, x_map;           // [NR], [L] int32: fine row -> coarse row, fine column -> coarse column, -1 = left out
    } coarse;
    // ... and the one of bi_sourcewise_set_coarse_binning (bi_sourcewise_coarse.h) over the bins of the source-wise store `fac`:
    // a second binning beside the grid model's, released by bi_factored_begin and bi_destroy
    Coarse sw_coarse;

    // model statistics (for the sparse forms)
    std::vector<double> h_rowsum;  // [A*S] sum over bins of every ps row
    std::vector<double> h_rowmin;  // [A*S] smallest entry of every ps row
    bool ps_nonneg = false;        // every ps entry is finite and >= 0

    // sparse forms of the data: CSR lists of the non-empty bins, and per-dataset compacted templates
    bool csr_ready = false, compact_ready = false;
    bool compact_sorted = false;               // the compacted copy holds the non-empty bins ordered by their count (build_compact_templates)
    DevBuf nz_idx, nz_n, nz_off, ps_c, cnt_c;
    DevBuf tm_entries, tm_off;                // tile-major copy of the non-empty-bin lists (k_dataset_dot_tiled): 4-byte entries, [n_tiles * T + 1] offsets
    int64_t nz_tile_epoch = -1;               // data epoch the copy was built for
    bool tm_ok = false;                       // ... and whether every count fits an entry (1 ... 32767: 15 bits)
    // the same lists over tiles of kDotTileMulti bins, for the toy-MC call over several parameter points (bi_eval_datasets_points:
    // the log mu tiles of four points side by side in LDS)
    DevBuf tmm_entries, tmm_off;
    int64_t tmm_epoch = -1;
    bool tmm_ok = false;
    int tmm_width = 4;
    int64_t toy_points_pp = 0;                // parameter: points per pass of that call (0 = by the batch: 4, or 2 for two points; 1 = point by point)
    int64_t toy_points_lanes = 0;             // parameter: lanes per (dataset, tile) run of its kernel (0 = measured default)
    int64_t toy_points_overlap = 0;           // parameter: the log mu pass and the finish of neighbouring pass groups run on a second stream beside the dot kernel (measured: no gain)
    hipStream_t stream2 = nullptr;            // ... that stream and its events (created on first use)
    hipEvent_t tp_ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t n_toy_points_passes = 0;          // read-only: passes over the entry lists the multi-point kernel has made
    int64_t dot_tiled = 1;                    // parameter: 0 = always the row kernel
    int64_t score_sorted = 1;                 // parameter: bi_score_events / bi_simulate_events order the events by cell before the gathers
    DevBuf ev_perm;                           // [events] sorted position -> the caller's event (valid while ev_sorted)
    bool ev_sorted = false;                   // the unbinned tensor's columns are in sorted order
    int64_t toy_fast_call = 7;                // parameter, bits: 1 descriptors in the kernel arguments, 2 parallel finish (k_dataset_finish_tiled), 4 poll the completion word
    DevBuf toy_blocks_done;                   // the finish kernel's block counter (zero between calls)
    bool toy_blocks_done_zeroed = false;
    unsigned long long toy_seq = 0;
    int64_t n_toy_polled = 0;                 // calls that returned on the completion word
    int64_t dot_entry16 = 1;                  // parameter: two-byte entries in the tile-major lists where every count is <= 7
    int tm_width = 4;                         // bytes per entry of the lists as built (2 or 4)
    int64_t dot_blocks_per_cu = 0;            // parameter: blocks of the tiled kernel per CU the dataset split aims at (0 = as many as are resident)
    int64_t dot_lanes = 0;                    // parameter: lanes per (dataset, tile) run of the tiled kernel: 0 = by entry width (8 with four-byte entries, 4 with two-byte ones), or 4 / 8 / 16
    int64_t toy_events = 1;                   // parameter: toys of sparse expectations are drawn event by event (0 = always one draw per bin)
    int64_t last_toy_method = 0;              // read-only: 1 = the last bi_generate_toys drew event by event, 0 = bin by bin
    std::vector<int64_t> h_nz_off;            // [T+1]
    std::vector<int64_t> h_c_off, h_cnt_off;  // [T] element offsets into ps_c / cnt_c
    std::vector<int64_t> h_c_np;              // [T] padded non-empty bins per dataset
    std::vector<double> h_Tz;                 // [T][A*S] sum of every ps row over the EMPTY bins of the dataset

    // persistent single-point slot (the lf(**kw) call shape): no allocation, one H2D, one D2H per call
    DevBuf slot_dev, slot_partial, slot_pflags, slot_counter;
    DevBuf mail, mail_flags;    // mailbox slots / status words of in-launch finishing: empty / zero between launches
    void* pack_host = nullptr;  // pinned staging of packed_upload (small-batch descriptors in, results out)
    void* bounce_host = nullptr;  // pinned bounce buffer of bi_memcpy_to_host / _to_device for copies of up to kBounceBytes
    size_t pack_host_bytes = 0;
    DevBuf pack_dev;
    void* plan_host = nullptr;  // pinned: what the device planner reports back (counters, group tables) + the word the host polls for it
    unsigned long long plan_seq = 0;
    void* slot_host = nullptr;  // pinned staging: descriptors in, {ll, status} out
    size_t slot_host_bytes = 0;
    unsigned long long slot_seq = 0;  // sequence number of single-point calls (the kernel echoes it when done)
    int64_t single_ns[3] = {0, 0, 0}; // accumulated wall time of single-point calls: host half, launch calls, wait
    int64_t single_calls = 0;
    int pending = 0;                  // bi_eval_begin without its bi_eval_end: 1 = launch in flight, 2 = answer parked
    unsigned long long pending_seq = 0;
    double pending_ll = 0.0;
    int32_t pending_status = 0;

    // device mirrors of the small tables the planning kernels read (bi_planning_device.h)
    DevBuf pt_grid, pt_mus, pt_coff, pt_allow, pt_c_off, pt_cnt_off, pt_c_np, pt_Tz, pt_rowsum, pt_rowmin, pt_nm_tot;
    int64_t plan_tables_epoch = -1;
    bool plan_tables_sparse = false;
    int64_t n_valid_launches = 0;                // how often the validity pass of a split scan ran
    int64_t n_scan_launches = 0;                 // how often the matrix-core scan kernel ran (observability)
    int64_t last_scan_nslots = 0, last_scan_resident = 0, last_valid_nslots = 0;   // what the planner chose last (read-only parameters)
    // the most recent scan launch (read-only parameters, all set in bi_run_plan beside the launch): the plan's groups and its longest
    // group's items after chunk_groups (a split scan: those of its validity pass, which sets these two only), the strip width in
    // 16-bin blocks, 1 = k_scan_sorted took it, 1 = k_scan_mfma's PROD = 1 instantiation did (set where it is chosen)
    int64_t last_scan_groups = 0, last_scan_max_items = 0, last_scan_cb = 0, last_scan_by_count = 0, last_scan_prod = 0;
    int64_t grad_mfma = 1;                       // bi_eval_grad: large single-dataset batches of plain binned likelihoods on the matrix cores (k_grad_mfma)
    int64_t grad_mfma_min = 2048;                // ... from this many points on (below, the planning of the batch costs more than the kernel saves)
    int64_t grad_slices = 0;                     // ... slices a cell's 16-bin blocks are split into (0 = by the batch)
    int64_t n_grad_mfma_launches = 0;
    int64_t scan_xcd = 1;                        // k_scan_sorted: how the (group, block) pairs are dealt to the 8 XCDs (0 launch order, 1 contiguous ranges, 2 group g -> XCD g mod 8)
    int64_t scan_share_slow = 1;                 // parameter: k_scan_sorted deals the items of mixed-count strips over all waves of the cell
    int64_t plan_count_sort = 1;                 // parameter: device planner: the one-pass counting sort where the keys take at most 1024 values (0: radix sort)
    int64_t plan_tables = 1;                     // parameter: device planner: group structure from per-key tables where the keys are few (0: scans over the points)
    int64_t scan_chunk = 1;                      // parameter: few groups with long item lists are cut into chunks of items, each a group of its own
    int64_t scan_waves_per_cu = 0;               // scan kernels: 0 = the planner sizes the split by occupancy; > 0 forces that many waves per CU
    int64_t keep_rows = -1;                      // single dense evaluations in a repeated cell: rows that keep the default cache policy (-1: as many as fit the Infinity Cache, 0: none)
    int64_t last_single_cell = -1, last_single_ds = -1;
    int64_t poll_result = 1;                     // single evaluations: poll the pinned result word instead of a stream sync
    int64_t tile_chunks = 8;                     // blocks walk the tiles in this many far-apart regions: block b (XCD b % 8) streams region b % 8
    int64_t scan_min_items = 4;                  // ... at least this many 16-point items per cell on average (x2: dense data)
    int64_t toy_offset = 0;                      // bi_generate_toys: toy t of the call is dataset toy_offset + t of the seed's stream
    int64_t scan_cb = 0;                         // scan kernel strip width in 16-bin blocks: 2, 4, or 0 = by the data
    int64_t bb_exact = 2;                        // single-point Beeston-Barlow calls: N(z) in numpy's summation order: 0 never, 1 always, 2 when some bin can have U_b == 0
    int64_t n_bb_exact = 0;                      // how often that pass ran
    int64_t scan_sparse_max_items = (int64_t)1 << 40;   // compacted rows: items per cell up to which the matrix-core scan kernel is used (round 1: 384;
                                                 // since the kernel leaves the linear term to the host it wins at every size: 46 vs 40 M evaluations/s at 10^6 points)
    int64_t scan_split = 1;                      // dense scans over mostly empty data: non-empty-bin pass + matrix-core validity pass
    int64_t sparse_at_upload = 1;                // value of `sparse` when the resident data were uploaded
    int64_t scan_mfma = 1;                       // scans: fp64 matrix-core kernel when many points share a cell
    int64_t scan_pow = 1;                        // dense-data scans run on a copy of the rows with the bins ordered by their count, where n log mu
                                                 // over a lane's bins becomes n log of their product (ensure_sorted_rows, k_scan_mfma PROD = 2)
    DevBuf ps_sorted, cnt_sorted;                // that copy: [A*S][Bp] rows and [Bp] counts of dataset 0
    int64_t sorted_epoch = -1;                   // data epoch it was (or could not be) built for
    bool sorted_ok = false;
    int64_t n_sorted_scans = 0;                  // how often a scan ran on it (observability)
    int64_t mail_timeout_ms = 2000;              // in-launch finish: how long a collecting block waits for a partial sum before BI_ST_INTERNAL
    int64_t debug_skip_post = -1, debug_late_post = -1;   // fault injection for the next mailbox launch (bi_params.h)
    int64_t n_mail_resets = 0;                   // how often the mailbox had to be emptied after a collector gave up
    std::vector<void*> user_allocs;              // bi_device_alloc buffers still alive: freed with the context
    int64_t bb_max_group = 8;                    // points per Beeston-Barlow work item (16: one wave per SIMD, accumulators partly in AGPRs)
    int64_t scan_bb = 1;                         // parameter: device-planned Beeston-Barlow batches on the matrix cores (k_scan_bb)
    int64_t scan_bb_min = 64;                    // ... from this many points on
    int64_t n_bb_scan_launches = 0;              // read-only
    int64_t plan_refused = 0;                    // read-only last_plan_refused: the last device-planner call refused its batch (1 exact Beeston-Barlow totals, 2 infinite rates)
    int64_t n_sampler_half_steps = 0;            // read-only: half-steps of bi_sample_stretch run so far
    int64_t device_plan_min = 512;               // batches at least this large are planned on the device

    // the events of the last bi_simulate_events into this context: coordinates [k][N], source index [N]
    DevBuf sim_coords, sim_source;
    int sim_k = 0;
    int64_t sim_n = -1;
    int64_t sim_epoch = -1;     // ... and the data epoch they belong to
    int64_t sim_cols = -1;      // bi_simulate_event_toys: the buffers hold this many columns in the padded layout of the sets (-1: one toy)

    // scratch
    DevBuf scratch, scratch2, logmu;

    // recycle cache for the small transient buffers of a call (descriptors, partials): hipMalloc / hipFree
    // cost tens of microseconds each and every call needs about ten of them.  All work of a context is
    // ordered on its one stream, so handing a buffer to the next call is safe without a sync.
    std::vector<DevBuf> cache;
    size_t cache_bytes = 0;

    int64_t epoch = 0;  // bumped by every model / data upload

    // tunables
    int64_t blocks_per_cu = 8;
    int64_t max_group = kMaxG;
    int64_t xcd_affine = 1;                      // multi-item launches: tile chunks keep their XCD across items
    int64_t fuse_max_blocks = (int64_t)1 << 20;  // single evaluations: finish inside the launch up to this many blocks
    int64_t single_blocks_per_cu = 4;            // single evaluations: blocks per CU the launch shape aims for
    int64_t fuse_finish = 1;                     // batched launches of few items: the last block of an item finishes it (no k_finish launch)
    int64_t single_kernel = 1;                   // bi_eval(P = 1): one fused launch (0: two-kernel fallback)
    int64_t nt_loads = 2;                        // nontemporal template loads: 0 never, 1 always, 2 when no reuse
    int64_t sparse = 1;                          // use the sparse forms when they are exactly equivalent
    int64_t compact_budget = (int64_t)16 << 30;  // bytes of HBM the compacted templates may take

    // profiling
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    int64_t prof_launches = 0;
    double prof_ms = 0.0;
};

namespace {

inline bool multi_set(const bi_ctx* c) { return c->unbinned && c->n_sets > 1; }

int fail(bi_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

int refuse_sets(bi_ctx* c, const char* what) {
    return fail(c, BI_ERR_INVALID, "%s is not available on an unbinned context that holds several event sets (%lld)", what, (long long)c->n_sets);
}

#define HIP_TRY(c, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((c), BI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

constexpr size_t kCacheMaxBuf = (size_t)1 << 30;      // only buffers up to 1 GiB are recycled (a 10^6-point scan: 256 + 640 MB)
constexpr size_t kCacheMaxTotal = (size_t)4 << 30;    // at most 4 GiB parked (given back when an allocation fails)
constexpr size_t kCacheMaxEntries = 256;

void dev_free(DevBuf& b) {
    if (b.p && !b.view) {
        bi_ctx* c = b.owner;
        if (c && b.bytes <= kCacheMaxBuf && c->cache.size() < kCacheMaxEntries && c->cache_bytes + b.bytes <= kCacheMaxTotal) {
            c->cache.push_back(b);
            c->cache_bytes += b.bytes;
        } else {
            (void)hipFree(b.p);
        }
    }
    b.p = nullptr;
    b.bytes = 0;
    b.view = false;
}

// The scratch of one function call: a DevBuf that goes back to its context's recycle cache when its scope ends, on every
// exit path.  dev_alloc, dev_upload and dev_free take it as the DevBuf it is; to release it before later work of the same
// function, close an inner { } scope or call dev_free(b), which leaves b empty.  What outlives a call -- the members of
// bi_ctx and bi_plan, the entries of the cache -- stays a plain DevBuf, copied by value.
struct ScratchBuf : DevBuf {
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf&) = delete;
    ScratchBuf& operator=(const ScratchBuf&) = delete;
    ~ScratchBuf() { dev_free(*this); }
};

void release_coarse(bi_ctx::Coarse& q) {
    dev_free(q.row_off); dev_free(q.row_list); dev_free(q.xb); dev_free(q.row_map); dev_free(q.x_map);
    q.set = false;
    q.C = 0;
}
void release_coarse(bi_ctx* c) { release_coarse(c->coarse); }

void drop_recycle_cache(bi_ctx* c) {
    (void)hipGetLastError();
    for (auto& q : c->cache) (void)hipFree(q.p);
    c->cache.clear();
    c->cache_bytes = 0;
}

int dev_alloc(bi_ctx* c, DevBuf& b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return BI_OK;
    if (b.p) dev_free(b);
    if (bytes == 0) bytes = 16;
    if (bytes <= kCacheMaxBuf) {  // smallest parked buffer that fits without wasting more than 4x
        size_t best = (size_t)-1;
        for (size_t i = 0; i < c->cache.size(); ++i)
            if (c->cache[i].bytes >= bytes && c->cache[i].bytes <= 4 * bytes + 4096 &&
                (best == (size_t)-1 || c->cache[i].bytes < c->cache[best].bytes))
                best = i;
        if (best != (size_t)-1) {
            b = c->cache[best];
            c->cache_bytes -= b.bytes;
            c->cache[best] = c->cache.back();
            c->cache.pop_back();
            return BI_OK;
        }
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        drop_recycle_cache(c);                  // give parked memory back and retry once
        e = hipMalloc(&b.p, bytes);
    }
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, BI_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    b.bytes = bytes;
    b.owner = c;
    return BI_OK;
}

template <class T>
int dev_upload(bi_ctx* c, DevBuf& b, const std::vector<T>& h) {
    int rc = dev_alloc(c, b, h.size() * sizeof(T));
    if (rc) return rc;
    if (!h.empty()) HIP_TRY(c, hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return BI_OK;
}

// Several small host arrays -> the device with ONE copy: they are laid out back to back (64-byte aligned) in the
// context's pinned staging block and moved with a single hipMemcpyAsync into one device slab.  `out_bytes` more
// bytes of the pinned block are reserved behind them for results a kernel writes straight to host memory.
// Sub-pointers: dev(i), host_out().  The block is owned by the context and reused by the next call, so the caller
// synchronises the stream before returning.
struct PackedUpload {
    std::vector<size_t> off;
    size_t in_bytes = 0, out_off = 0;
    char* dev_base = nullptr;
    char* host_base = nullptr;
    template <typename T>
    const T* dev(size_t i) const { return reinterpret_cast<const T*>(dev_base + off[i]); }
    void* host_out() const { return host_base + out_off; }
};

inline int packed_upload(bi_ctx* c, const std::vector<std::pair<const void*, size_t>>& parts, size_t out_bytes, PackedUpload& pu,
                         DevBuf* slab = nullptr) {   // slab: a caller-owned device buffer instead of the context's
    pu.off.clear();
    size_t total = 0;
    for (const auto& part : parts) {
        pu.off.push_back(total);
        total += (part.second + 63) / 64 * 64;
    }
    pu.in_bytes = total;
    pu.out_off = total;
    const size_t need = total + (out_bytes + 63) / 64 * 64 + 64;
    if (c->pack_host_bytes < need) {
        if (c->pack_host) { HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipHostFree(c->pack_host)); c->pack_host = nullptr; c->pack_host_bytes = 0; }
        const size_t grow = std::max<size_t>(2 * need, 65536);
        HIP_TRY(c, hipHostMalloc(&c->pack_host, grow, hipHostMallocDefault));
        c->pack_host_bytes = grow;
    }
    DevBuf& dst = slab ? *slab : c->pack_dev;
    int rc = dev_alloc(c, dst, std::max<size_t>(total, 64));
    if (rc) return rc;
    pu.host_base = (char*)c->pack_host;
    pu.dev_base = (char*)dst.p;
    for (size_t i = 0; i < parts.size(); ++i)
        if (parts[i].second) memcpy(pu.host_base + pu.off[i], parts[i].first, parts[i].second);
    if (total) HIP_TRY(c, hipMemcpyAsync(pu.dev_base, pu.host_base, total, hipMemcpyHostToDevice, c->stream));
    return BI_OK;
}

void free_plan_buffers(bi_plan* p) {
    for (auto& k : p->classes) {
        dev_free(k.rowoff); dev_free(k.coef); dev_free(k.aux); dev_free(k.item_cnt); dev_free(k.item_tiles);
        dev_free(k.perm); dev_free(k.slot_lg); dev_free(k.partial); dev_free(k.pflags); dev_free(k.rowoff_full);
    }
    dev_free(p->bad_idx); dev_free(p->nan_idx); dev_free(p->out); dev_free(p->status); dev_free(p->grp_first); dev_free(p->grp_items);
    dev_free(p->slab); dev_free(p->bad); dev_free(p->sorted_idx); dev_free(p->keep_z); dev_free(p->keep_rs);
}

}  // namespace
