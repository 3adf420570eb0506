/* blueice_hip.h -- C ABI of libblueice_hip.so: the MI355X (gfx950) binned-likelihood hot path.
 *
 * The reference (JelleAalbers/blueice v1.2.1) is pure Python and has no FFI; its extension
 * points for this path are Python-level.  Every entry point below cites the reference
 * interface (file:line under /root/reference) whose work it takes over.  Python binds this
 * header with ctypes (blueice_amd/_capi.py); INTEGRATION.md shows the stub a blueice
 * maintainer would add.
 *
 * Conventions
 *   - All host buffers are borrowed for the duration of the call; the library copies what it
 *     needs.  Device memory is owned by the context until bi_destroy.
 *   - Return value: 0 = BI_OK, negative = error (message via bi_last_error).  Nothing throws
 *     across the boundary.  Numerical edge cases are VALUES (-inf / nan as the reference
 *     produces them), not errors.
 *   - One context = one device + one HIP stream.  A context is not re-entrant; distinct
 *     contexts are independent (one per GPU / per process in multi-GPU runs).
 *   - All floating point is IEEE binary64.  Layouts are C order.
 */
#ifndef BLUEICE_HIP_H
#define BLUEICE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these are its only exports */
#endif

typedef struct bi_ctx bi_ctx;

enum {
    BI_OK = 0,
    BI_ERR_INVALID = -1, /* bad argument / shape mismatch */
    BI_ERR_HIP = -2,     /* HIP runtime failure (message has the hipError string) */
    BI_ERR_STATE = -3,   /* model or data not uploaded yet (reference: NotPreparedException,
                            blueice/likelihood.py:30-50) */
    BI_ERR_NOMEM = -4
};

/* per-point status bits written by bi_eval (reference behaviour in brackets) */
enum {
    BI_ST_OUT_OF_BOUNDS = 1, /* z outside the anchor box or nan [-inf, likelihood.py:345-347] */
    BI_ST_UNPHYSICAL = 2,    /* rates not in [0, inf) [-inf or ValueError, likelihood.py:397-415] */
    BI_ST_BB_ROOT1 = 4,      /* Beeston-Barlow `assert all(A1 <= 0)` would fail [likelihood.py:649] */
    BI_ST_BB_NEG = 8,        /* Beeston-Barlow `assert all(0 <= A)` would fail [likelihood.py:655] */
    BI_ST_BAD_DATASET = 16,  /* dataset index out of range */
    BI_ST_INTERNAL = 32      /* the in-launch reduction gave up waiting for a partial sum (result nan): a device fault */
};

/* ---- lifetime ------------------------------------------------------------------------- */
int bi_create(int device, bi_ctx** out);
void bi_destroy(bi_ctx* ctx);
const char* bi_last_error(const bi_ctx* ctx); /* ctx == NULL: last error of a failed bi_create */
const char* bi_version(void);
/* name (<= len bytes), compute units, total HBM bytes, gfx arch string (<= len bytes) */
int bi_device_info(bi_ctx* ctx, char* name, char* arch, int len, int* n_cu, int64_t* hbm_bytes);

/* ---- model: the anchor tensors built by GridInterpolator.make_interpolator ---------------
 * (blueice/pdf_morphers.py:57-67 fills `anchor_scores[A_0..A_{d-1}, *extra_dims]` and wraps it
 * in a RegularGridInterpolator; BinnedLogLikelihood.prepare builds three of them,
 * blueice/likelihood.py:248-251 (mus), :593-596 (ps), :598-601 (n_model_events)).
 *
 *   d          number of shape parameters (0 allowed: no morphing, likelihood.py:359-363)
 *   n_anchor   [d]   anchors per axis
 *   anchor_z   concatenated, ascending per axis (pdf_morphers.py:48)
 *   S, B       sources, total analysis bins (product of the analysis-space shape)
 *   ps         [A_0..A_{d-1}][S][B]
 *   mus        [A_0..A_{d-1}][S]
 *   n_model    NULL or [A_0..A_{d-1}][S][B]; only row `bb_source` is kept (likelihood.py:643)
 *   bb_source  -1 = no Beeston-Barlow, else the 'bb_single_source' index (likelihood.py:625-630)
 */
int bi_upload_model(bi_ctx* ctx, int d, const int32_t* n_anchor, const double* anchor_z, int S, int64_t B,
                    const double* ps, const double* mus, const double* n_model, int bb_source);

/* Streaming variant of the same: declare the grid, then hand over one anchor model at a time in
 * any order -- exactly the loop of pdf_morphers.py:62-65 -- so no dense host tensor is needed. */
int bi_model_begin(bi_ctx* ctx, int d, const int32_t* n_anchor, const double* anchor_z, int S, int64_t B,
                   int bb_source);
/* anchor_index: C-order linear index into the anchor grid; ps [S][B]; mus [S];
 * n_model_row NULL or [B] (= n_model_events[bb_source]) */
int bi_model_set_anchor(bi_ctx* ctx, int64_t anchor_index, const double* ps, const double* mus,
                        const double* n_model_row);
int bi_model_end(bi_ctx* ctx);

/* Bin-sharded models (a tensor too large for one GPU: every rank holds a slice of the bins of every row and
 * the per-rank log likelihoods add up).  Everything is additive over bins except the Beeston-Barlow
 * normalisation N_c = sum over ALL bins of n_model[c, bb_source, :] (likelihood.py:645): read the local sums,
 * all-reduce them across ranks, and write the global ones back before evaluating.  totals: [A]. */
int bi_get_bb_totals(bi_ctx* ctx, double* totals);
int bi_set_bb_totals(bi_ctx* ctx, const double* totals);

/* per-source `allow_negative` flags (likelihood.py:82-83,397-415); default all 0 */
int bi_set_allow_negative(bi_ctx* ctx, const int32_t* allow /*[S]*/);

/* ---- data: what BinnedLogLikelihood.set_data leaves in data_events_per_bin.histogram ------
 * (blueice/likelihood.py:603-609).  T datasets of B float64 counts each (toy MC: T > 1). */
int bi_upload_counts(bi_ctx* ctx, int64_t T, const double* counts /*[T][B]*/);

/* set_data on the device: declare the analysis space once (config['analysis_space'] = [[name, edges], ...],
 * blueice/likelihood.py:607), then bin N events into dataset 0 there -- numpy.histogramdd semantics, which is
 * what multihist's Histdd.add applies in likelihood.py:608-609 (right-most edge inclusive, events outside the
 * range dropped).  coords: [k][N] (one column per analysis dimension).  Replaces the context's data. */
int bi_set_analysis_space(bi_ctx* ctx, int k, const int32_t* n_edges /*[k]*/, const double* edges /*concatenated*/);
int bi_upload_events(bi_ctx* ctx, int64_t N, const double* coords);

/* Template building: the same binning as a stand-alone service, for the histograms the sources fill while the anchor
 * models are built -- DensityEstimatingSource.build_histogram's `mh.add(...)`, blueice/source.py:287-299, i.e.
 * numpy.histogramdd of N events in k dimensions (about a second per 10^6 three-dimensional events on a host core, times
 * sources x anchor models; ~3 ms here, most of it PCIe).  Needs no model and touches none of the context's state:
 * coords [k][N] and the edges are borrowed for the call, counts [prod(n_edges - 1)] (C order, host) is OVERWRITTEN with
 * the number of events per bin.  Unweighted events only. */
int bi_histogram_events(bi_ctx* ctx, int k, const int32_t* n_edges /*[k]*/, const double* edges /*concatenated*/,
                        int64_t N, const double* coords, double* counts);

/* Extended unbinned likelihood on the same machinery (UnbinnedLogLikelihood, blueice/likelihood.py:528-573;
 * extended_loglikelihood :678-690).  Upload the model with B = number of events and `ps` = the pdf values
 * of every source at every event for every anchor (what `Model.score_events(d)` returns,
 * likelihood.py:557-560, model.py:97-99), then switch the context:
 *     ll = -sum_s mu_s + sum_events log( sum_s mu_s p_s(x_e) ),
 * events whose summed density is not > 0 get `outlier_likelihood` instead when it is non-zero
 * (config 'outlier_likelihood', default 1e-12, likelihood.py:573,687-689).  No counts are needed;
 * bi_eval / bi_plan_* / bi_interpolate / bi_eval_full work as for the binned case.  A nan pdf value drops that
 * source's term for that event (numpy.nansum, likelihood.py:686).  B = 0 (no events) is allowed. */
int bi_set_unbinned(bi_ctx* ctx, double outlier_likelihood);

/* set_data of the unbinned likelihood on the device, for sources whose pdf is a histogram (HistogramPdfSource.pdf,
 * blueice/source.py:218-243): `templates` holds the DENSITY histograms of every source at every anchor as its model
 * rows ([A..][S][B], uploaded once like a binned model); this call evaluates all of them at N events and leaves the
 * result -- the [A..][S][N] tensor `Model.score_events(d)` would have produced anchor by anchor on the host,
 * likelihood.py:557-560 -- as the model of `target` (same device), copies the expected-event table, and switches
 * `target` to the unbinned likelihood as bi_set_unbinned does.  Only the k x N event coordinates cross PCIe.
 *   method 0 'piecewise': the density of the bin the event falls in; `grid` = the bin EDGES of every axis; an event
 *            on an edge belongs to the bin on its left, events outside take the first / last bin (the lookup of the
 *            package's Histdd);
 *   method 1 'linear':    scipy's RegularGridInterpolator over the bin CENTRES (`grid` = the centres of every axis,
 *            as the host computed them; >= 2 per axis), in its operation order; coords must already be clipped to
 *            [first centre, last centre] and finite, as source.py:232-241 does.
 * n_grid[k], grid concatenated; coords [k][N]. */
int bi_score_events(bi_ctx* templates, bi_ctx* target, int method, int k, const int32_t* n_grid, const double* grid,
                    int64_t N, const double* coords, double outlier_likelihood);

/* Event-level toy Monte Carlo on the device, for the unbinned likelihood with histogram-pdf sources: what
 * `Model.simulate` (blueice/model.py:69-91) does source by source on the host -- N_s ~ Poisson(mu_s) events, each drawn
 * from the source's pdf, for a histogram pdf a bin with probability density x volume and a uniform position inside it
 * (`HistogramPdfSource.simulate`, blueice/source.py:248-264) -- followed by `set_data` (likelihood.py:531-563), without
 * the events ever leaving HBM.  `templates` holds the density histograms of every source at every anchor (as for
 * bi_score_events); the events are drawn at parameter point (z, rate_scale) from the MORPHED densities, scored at every
 * anchor model, and become the (unbinned) data of `target`.  Philox4x32-10 keyed by the seed; counters are (event within
 * its source, source), so a toy does not depend on launch geometry.
 *   method 0 / 1   the sources' pdf_interpolation_method 'piecewise' / 'linear' (as bi_score_events; with 'linear' the
 *                  coordinates are clipped to the outer bin centres before scoring, source.py:232-241)
 *   n_edges [k], edges concatenated: the BIN EDGES of the analysis space
 *   n_per_source [S] or NULL: receives the number of events drawn per source
 * bi_download_events copies the simulated coordinates [k][N] (and the source index of every event) to the host,
 * N = bi_simulated_event_count.
 *
 * The random stream, exactly (Philox, u53, poisson_small and poisson_ptrs as defined at bi_generate_toys below; binary64):
 *   rates   r_s = mus_s(z) rate_scale_s.  N_s = 0 where r_s = 0; otherwise N_s is the event count of bi_generate_toys' stream B
 *           with M = r_s, dataset number t = s and the key taken from  seed ^ 0x9E3779B97F4A7C15  (everything below is keyed
 *           by the seed itself).  The count travels as a 32-bit int: rates of 2^30 and above are refused (BI_ERR_INVALID,
 *           "... at most 2^30 expected events per source"), so that no count can pass 2^31.
 *   pmf     bins are numbered in C order over the axes (axis 0 slowest; stride_i = prod_{i' > i} (n_edges_i' - 1)); the decode
 *           of bin b is, axis by axis from 0:  i_ax = rem / stride_ax, rem -= i_ax stride_ax.  vol_b = prod_ax (e_ax[i_ax + 1] -
 *           e_ax[i_ax]) (multiplied in axis order from 1), pmf_s,b = max(density_s,b(z) vol_b, 0) (nan counts as 0), F_s = the
 *           running sums of pmf_s over b (a device prefix sum: a fixed tree order, not left to right).
 *   events  are stored -- and downloaded -- in drawn order: source by source, event j = 0 .. N_s - 1 of source s at position
 *           first_s + j, first_s = sum_{s' < s} N_s'.  score_sorted orders a private index of the events by histogram cell for
 *           the scoring gathers only; the stored coordinates, their order and the per-event values handed back are untouched.
 *           bin:       (r0, r1, ., .) = Philox(counter = (j mod 2^32, j >> 32, s, 0x53494D45), key);  target = u53(r0, r1) F_s[B-1];
 *                      the bin is the first b with F_s[b] > target, clamped to B - 1 (so never a bin of zero pmf below the last).
 *           position:  per axis ax, (r0, r1, ., .) = Philox(counter = (j mod 2^32, j >> 32, s | ax << 24, 0x53494D46), key),
 *                      u = u53(r0, r1),  x_ax = e_ax[i_ax] + u (e_ax[i_ax + 1] - e_ax[i_ax])  (the multiply-add may be fused). */
int bi_simulate_events(bi_ctx* templates, bi_ctx* target, const double* z, const double* rate_scale, int method, int k,
                       const int32_t* n_edges, const double* edges, uint64_t seed, double outlier_likelihood,
                       int64_t* n_per_source);
int bi_download_events(bi_ctx* target, double* coords /*[k][N] or NULL*/, int32_t* source /*[N] or NULL*/);
int64_t bi_simulated_event_count(const bi_ctx* target);

/* Several event sets in one unbinned context: an ensemble of T event-level datasets (toys) side by side on the event axis
 * of the [A..][S][columns] tensor.  Set t occupies columns [first_t, first_t + N_t); every first_t is even (first_0 = 0,
 * first_{t+1} = first_t + N_t rounded up to even), so a set starts 16-byte aligned; the at most one padding column behind a
 * set holds 1.0 in every row and enters no sum; N_t = 0 is allowed.  Point evaluations take the set from their `dataset`
 * column (bi_eval, bi_eval_grad, bi_fit_batched*, the `dataset` of bi_eval_begin and bi_eval_full; no column: set 0); the expected-event
 * term -sum_s mu_s is per point as before.  With T = 1 the two calls below ARE bi_score_events / bi_simulate_events.
 * Not available on a context with T > 1 sets (BI_ERR_INVALID, "... several event sets ..."): bi_plan_points*, bi_eval_hess
 * with a dataset column, bi_sample_stretch* with more than one ensemble or another set than 0, and bi_eval_datasets*.
 * bi_eval_full(dataset = t) hands back ps_out [S][N_t], the pdf values at the events of set t; bi_interpolate(0) those of
 * set 0.  Beeston-Barlow and binned contexts have no event sets.
 *
 * bi_score_event_sets: bi_score_events for a stack of T datasets; coords [k][N] holds the events of set t at
 * [offsets[t], offsets[t + 1]), offsets[0] = 0, offsets[T] = N, ascending.  One scoring launch fills the tensor.
 *
 * bi_simulate_event_toys: T toys at one truth point, drawn, placed and scored without a host round trip per toy (one
 * read-back: the counts, which size the tensor).  Toy t of the call is toy D = toy_offset + t (the context parameter, as
 * for bi_generate_toys) of the seed's ensemble, and toy D is -- event for event, bit for bit -- what bi_simulate_events
 * draws with the seed toy_seed(seed, D):
 *     toy_seed(seed, D):  x = seed + (D + 1) 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) 0xBF58476D1CE4E5B9;
 *                         x = (x ^ x >> 27) 0x94D049BB133111EB;  toy_seed = x ^ x >> 31        (all modulo 2^64)
 * D -> seed + (D + 1) c is one-to-one modulo 2^64 (c is odd) and the three mixing steps are bijections, so two toys of one
 * ensemble never share a stream; an ensemble depends on neither T, nor the chunking, nor the launch geometry.  The
 * per-source limits of bi_simulate_events hold per toy; the total event count is 64-bit.
 *   n_per_toy_source [T][S] or NULL: receives the events drawn per toy and source
 * bi_event_set_offsets: offsets [T + 1] receives first_0 .. first_{T-1} and, last, the number of columns in use;
 * bi_event_set_counts: counts [T] receives N_t.  bi_event_set_count: T (1 for every other unbinned context, 0 otherwise).
 * bi_download_events after bi_simulate_event_toys hands back all events set by set, in drawn order, without the padding:
 * coords [k][N], N = bi_simulated_event_count = sum_t N_t, set t at [sum_{t' < t} N_t', ...). */
int bi_score_event_sets(bi_ctx* templates, bi_ctx* target, int method, int k, const int32_t* n_grid, const double* grid,
                        int64_t T, const int64_t* offsets /*[T+1]*/, const double* coords /*[k][N]*/, double outlier_likelihood);
int bi_simulate_event_toys(bi_ctx* templates, bi_ctx* target, const double* z, const double* rate_scale, int method, int k,
                           const int32_t* n_edges, const double* edges, int64_t T, uint64_t seed, double outlier_likelihood,
                           int64_t* n_per_toy_source /*[T][S] or NULL*/);
int bi_event_set_offsets(bi_ctx* target, int64_t* offsets /*[T+1]*/);
int bi_event_set_counts(bi_ctx* target, int64_t* counts /*[T]*/);
int64_t bi_event_set_count(const bi_ctx* target);
/* after bi_set_unbinned on a model whose columns the caller filled in that layout (pdf values scored on the host; padding
 * columns finite): declare the T sets, counts [T]; the padded sets must take exactly the model's B columns */
int bi_set_event_sets(bi_ctx* ctx, int64_t T, const int64_t* counts);
/* the pdf values of set t as they are resident: out [A..][S][N_t] (BI_ERR_STATE while the columns are ordered by cell, score_sorted) */
int bi_download_event_set(bi_ctx* target, int64_t t, double* out);

/* Toy-MC datasets generated on the device: n_{t,b} ~ Poisson(mu_b), mu_b = sum_s r_s p_{s,b}(z) -- the binned
 * equivalent of Model.simulate (blueice/model.py:69-91: Poisson number of events per source, each drawn from
 * the source's pdf) followed by set_data's binning (blueice/likelihood.py:603-609).  Philox4x32-10 keyed by
 * (seed; dataset, bin): reproducible and independent of launch geometry.  The T datasets REPLACE the
 * context's data and are stored as non-empty-bin lists only (no [T][B] array, no host transfer);
 * bi_eval_datasets works on them directly, point evaluations when the compacted templates fit the budget.
 *
 * The random streams, exactly (binary64; tests/toy_oracle.py is written from this text).  Toy t of a call is dataset
 * D = toy_offset + t of the seed's stream, whatever the launch geometry; key = (seed mod 2^32, seed >> 32); Dlo = D mod 2^32,
 * Dhi = (D >> 32) & 0xFFFF (dataset numbers are told apart up to 2^48).  Philox = Philox4x32-10 as written out at
 * bi_sample_stretch.  u53(a, b) = ((a >> 5) 2^26 + (b >> 6)) 2^-53, uniform on [0, 1).
 *   poisson_small(lam, u), lam < 10: inversion by sequential search.  p = F = exp(-lam), n = 0; while u > F and n < 1000:
 *       n += 1, p *= lam / n, F += p; the draw is n -- in exact arithmetic the smallest n with u <= CDF(n; lam).  The cap:
 *       where the rounded F stalls below a u within a few ulp of 1 the loop runs out and the draw is 1000 (probability
 *       ~2^-50 per draw; it is returned as drawn, not clamped).
 *   poisson_ptrs(lam, D, b), lam >= 10: PTRS (Hoermann 1993).  slam = sqrt(lam), loglam = log(lam), bb = 0.931 + 2.53 slam,
 *       aa = -0.059 + 0.02483 bb, invalpha = 1.1239 + 1.1328 / (bb - 3.4), vr = 0.9277 - 3.6224 / (bb - 2).  Attempt a = 0, 1, ...:
 *         (r0, r1, r2, r3) = Philox(counter = (b mod 2^32, b >> 32, Dlo, Dhi | (a + 1) << 16), key)
 *         U = u53(r0, r1) - 0.5, V = u53(r2, r3), us = 0.5 - |U|, k = floor((2 aa / us + bb) U + lam + 0.43)
 *         if us >= 0.07 and V <= vr: the draw is k
 *         if k < 0 or (us < 0.013 and V > us): next attempt
 *         if log(V) + log(invalpha) - log(aa / (us us) + bb) <= -lam + k loglam - lgamma(k + 1): the draw is k
 *       (after 4096 rejected attempts the draw is floor(lam); the acceptance is above 0.9 per attempt).
 *   A, one draw per bin (toy_events = 0, B < 4096, templates that may be negative, or expectations not sparse -- see
 *   toy_events): bins 2q and 2q + 1 share the block (r0, r1, r2, r3) = Philox(counter = (q mod 2^32, q >> 32, Dlo, Dhi), key):
 *       the even bin draws poisson_small(mu, u53(r0, r1)), the odd one poisson_small(mu, u53(r2, r3)), each where 0 < mu < 10;
 *       a bin with mu >= 10 draws poisson_ptrs(mu, D, b) with its own bin number b; mu = 0 (or nan, or below 0) gives 0.
 *   B, event by event (last_toy_method = 1): M = sum_b mu_b and the running sums F of mu come from a device prefix sum (a
 *   fixed tree order).  The call goes this way iff 0 < M < B / 8 and M + 12 sqrt(max(M, 1)) + 32 <= 32768, and no toy of
 *   the call draws more events than the smallest power of two >= that bound (at least 1024); else all of it goes by A.
 *       events of the toy:  N = poisson_ptrs(M, D, 2^40 + 7) for M >= 10 (a bin no model has); for M < 10
 *                           N = poisson_small(M, u53(r0, r1)), (r0, r1, ., .) = Philox(counter = (0xFFFFFFFF, 0x45564E54, Dlo, Dhi), key)
 *       bin of event e < N: (r0, r1, ., .) = Philox(counter = (e, 0x45564E54, Dlo, Dhi), key), target = u53(r0, r1) M; the bin
 *                           is the first b with F[b] > target, clamped to B - 1: bins of mu = 0 below the last never get one.
 *       The toy's counts are the histogram of its events' bins (sorted per toy in LDS -- a 4-bit LSD radix sort up to 16384
 *       keys, a bitonic network for 32768 -- and run-length encoded); the lists come out in ascending bin order by A and B. */
int bi_generate_toys(bi_ctx* ctx, const double* z, const double* rate_scale, int64_t T, uint64_t seed);
/* T = sum_h n_toys[h] toys at H truth points in one call: n_toys[h] >= 0 toys at (z[h], rate_scale[h]), truth-major.  The
 * stream, exactly: with first_h = sum_{h' < h} n_toys[h'], toy t of the call is toy D = toy_offset + t of the seed's ensemble,
 * and the toys first_h .. first_h + n_toys[h] - 1 of the call -- their non-empty-bin lists, lgsum entries and numbers of
 * non-empty bins -- are bit for bit what bi_generate_toys(z[h], rate_scale[h], n_toys[h], seed) leaves with the context
 * parameter toy_offset at toy_offset + first_h.  The ensemble therefore does not depend on how truths are grouped into calls.
 * Every truth chooses between A and B by the rules above as a call of its own would: with its own M_h, its own bound and
 * power of two (which enters both the test "no toy draws more events" and the size of the sort), and its own fall-back to A
 * when one of ITS toys draws more events than that; the toys of the other truths are not affected.  method_out (when given)
 * [H]: 1 = B, 0 = A, -1 = a truth with n_toys[h] = 0; last_toy_method = 1 iff every truth that has toys went by B.
 * bi_generate_toys is the H = 1 case of this call.
 * All truths are validated before the context changes: one outside the anchor box, or with rates outside [0, inf), refuses
 * the whole call with bi_generate_toys' error, which names the truth ("toy generation (truth 1) point is outside the anchor
 * box"), and the data held so far stay usable.  z: [H][d] (NULL when d = 0), rate_scale: [H][S] or NULL; n_toys [H] with
 * 1 <= T < 2^31.  Afterwards the context is as bi_generate_toys leaves it, with T datasets.  Scratch: H * Bp doubles each for
 * mu and exp(-mu), H * B for the running sums where B applies: callers bound H per call. */
int bi_generate_toys_points(bi_ctx* ctx, int64_t H, const double* z, const double* rate_scale, const int64_t* n_toys, uint64_t seed,
                            int32_t* method_out);
/* Expands device-generated toys (non-empty-bin lists) into the dense [T][B] counts array as well, on the device: what
 * the paths that visit every bin need -- Beeston-Barlow point evaluations and gradients (likelihood.py:618-660 read n in
 * every bin), sparse = 0.  T * B * 8 bytes of HBM; a no-op when the counts are dense already. */
int bi_counts_to_dense(bi_ctx* ctx);
/* dense counts [B] of dataset t, from whatever form is resident */
int bi_download_counts(bi_ctx* ctx, int64_t t, double* out);

/* ---- the hot path -----------------------------------------------------------------------
 * P independent evaluations of LogLikelihoodBase.__call__ (blueice/likelihood.py:318-427)
 * without the Python-callable priors:
 *   mus = mus_interpolator(z); ps = ps_interpolator(z) [; n_model_events_interpolator(z)]
 *   (:355-357, scipy RegularGridInterpolator semantics, pdf_morphers.py:67-70)
 *   mus *= rate_scale (rate multiplier :366-368, livetime :374-382, efficiency :385-393)
 *   unphysical check (:397-415) -> -inf
 *   adjust_expectations ('bb_single', :618-660)
 *   _compute_likelihood = sum_bins poisson.logpmf(n | sum_s mus_s ps_s) (:662-675)
 *
 *   z          [P][d]   (ignored when d == 0)
 *   rate_scale [P][S]   or NULL (= all ones)
 *   dataset    [P]      or NULL (= dataset 0)
 *   out        [P]      log likelihoods (-inf / nan exactly where the reference gives them)
 *   status     [P]      or NULL; BI_ST_* bits
 * Points are grouped by (grid cell, dataset) internally so that corner templates are read once
 * per group. */
int bi_eval(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
            double* out, int32_t* status);

/* bi_eval(P = 1) in two halves, for a caller that evaluates several contexts at once -- a sum of likelihoods with
 * one context per term (LogLikelihoodSum, blueice/likelihood.py:867-955): bi_eval_begin on every context, then
 * bi_eval_end on every context, and the launches overlap.  One bi_eval_begin may be outstanding per context; any
 * other call on that context in between is a caller error, except bi_eval_end. */
int bi_eval_begin(bi_ctx* ctx, const double* z, const double* rate_scale, int64_t dataset);
int bi_eval_end(bi_ctx* ctx, double* out, int32_t* status);

/* Value and analytic gradient in ONE pass over the templates (no counterpart in the reference, whose
 * fits differentiate `make_objective`'s f numerically: blueice/inference.py:111-124,153-155).
 *   ll   [P]          as bi_eval
 *   grad [P][d + S]   d ll / d z_i (i < d; through the morph weights AND through mus(z)), then
 *                     d ll / d rate_scale_s.  Inside a grid cell ll is smooth; on an anchor the
 *                     derivative is the one of the cell the point is assigned to.  NaN where ll = -inf.
 * Needs 1 + d + S <= 16.
 * With Beeston-Barlow (bb_source >= 0; blueice/likelihood.py:618-660,693-712) the chain rule runs through the per-bin root:
 * mu_b = U_b + A_b p_b with p_b = r_i P_b / a_b, d mu = dU + p dA + A dp, dA from the root formula's partial derivatives;
 * in bins with U_b == 0 exactly the derivative of the reference's special case A = (n + a) / (1 + p_cal) is taken (on that
 * measure-zero set the two branches of the reference differ, so ll itself is not differentiable across it).  d <= 7 there.
 * status carries the Beeston-Barlow assertion bits of the value, as bi_eval does.
 * Extended unbinned likelihood (bi_set_unbinned / bi_score_events; blueice/likelihood.py:678-690): the same call returns
 *   d ll = -sum_s d mu_s + sum_events (sum_s d(mu_s p_s(x_e))) / (sum_s mu_s p_s(x_e));
 * an event that takes the outlier likelihood (density not > 0) is a constant and contributes no slope, a source whose term is
 * nan at an event is dropped from value and slopes alike (numpy.nansum, likelihood.py:686); `dataset` is ignored. */
int bi_eval_grad(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                 double* grad, int32_t* status);

/* Value, gradient and Hessian of ll in one pass over the corner rows of each point.  ll [P], grad [P][d + S] and status [P]
 * are what bi_eval_grad returns; hess [P][d + S][d + S] holds d2 ll / (d theta_q d theta_r), theta = (z_0 .. z_{d-1},
 * rate_scale_0 .. rate_scale_{S-1}): full and symmetric (written from one triangle), rows and columns of axes with a single
 * anchor 0, NaN wherever ll = -inf.  Inside a grid cell the morph is multilinear, so every second derivative of mu_b is
 * another fixed combination of the cell's corner rows:
 *   H_qr = sum_b [ (n_b / mu_b - 1) d_qr mu_b - (n_b / mu_b^2) d_q mu_b d_r mu_b ]      (binned; n_b = 0: -d_qr mu_b)
 *   H_qr = -sum_s d_qr mu_s + sum_e [ d_qr lambda_e / lambda_e - d_q lambda_e d_r lambda_e / lambda_e^2 ]   (unbinned)
 * an event on the outlier clamp contributes nothing.  On an anchor the Hessian is that of the cell the point is assigned to
 * (the convention of bi_eval_grad).  Covers binned likelihoods without Beeston-Barlow (dense and non-empty-bin forms,
 * device-generated toys) and the extended unbinned likelihood with finite pdfs, up to 1 + D + D2 <= 64 coefficient columns
 * and D <= 16 first-order parameters (D = effective axes + S; D2 = the non-zero second-order columns,
 * d_eff (d_eff + 1) / 2 + d_eff S).  Anything else returns BI_ERR_INVALID with the reason in bi_last_error. */
int bi_eval_hess(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                 double* grad, double* hess, int32_t* status);

/* Goodness of fit of the data term: per point p, against dataset dataset[p] (NULL: dataset 0), with mu_b the expectation of
 * bin b at (z, rate_scale) and n_b the dataset's count,
 *   half_deviance [P]   sum_b  mu_b - n_b - n_b log(mu_b / n_b)      (n_b = 0: mu_b)    -- the deviance is twice this
 *   pearson       [P]   sum_b  (n_b - mu_b)^2 / mu_b                   (n_b = 0: mu_b)
 * each summed bin by bin in this form, never as a difference of two log-likelihoods.  A bin with n_b = 0 and mu_b = 0
 * contributes 0 to both.  Points are screened as by bi_eval_grad (same status bits); a point outside the anchor box or with
 * unphysical rates gets +inf in both.  For a live point both are +inf where bi_eval returns ll = -inf (an event in a bin
 * where nothing is expected) and nan where it returns nan (a negative expectation).  Priors are no part of either.
 * Dense and non-empty-bin forms of the data (device-generated toys included), chosen as bi_eval_hess chooses.  Binned
 * likelihoods without Beeston-Barlow only: BI_ERR_INVALID with the reason in bi_last_error otherwise. */
int bi_eval_gof(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                double* half_deviance, double* pearson, int32_t* status);

/* The expectation itself: out [P][B] holds mu_b at every point (per_source = 0), or out [P][S][B] the expectation
 * mu_{s,b} of every source (per_source != 0; their sum over s is mu_b).  Read from the dense template tensor: no data
 * are needed.  The row(s) of a point outside the anchor box or with unphysical rates are nan.  Binned likelihoods without
 * Beeston-Barlow only (there the expectation depends on the data): BI_ERR_INVALID otherwise. */
int bi_expected_counts(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int per_source, double* out);

/* Coarse views: the expectation, and the data, summed over tensor-product groups of fine bins -- projections on one or two
 * analysis axes, a rebinned space, a signal box -- without the fine bins ever leaving the device.
 *   bi_set_coarse_binning   the binning of the context.  k analysis axes with n_fine[j] fine bins each (their product must be
 *                           the model's B; bins are in C order, the last axis fastest); axis j is cut into n_groups[j] >= 1
 *                           groups of adjacent fine bins by the n_groups[j] + 1 boundaries e_0 < ... < e_m, 0 <= e_0 and
 *                           e_m <= n_fine[j] (group g holds the fine bins e_g <= i < e_g+1; bins below e_0 or from e_m on
 *                           belong to no cell); `bounds` holds the axes' boundaries one after the other.  A cell is one group
 *                           per axis, C = prod_j n_groups[j] cells in C order; *n_cells (nullable) gets C.  An axis that is
 *                           summed over has one group.  k = 0 clears the binning, and a new model releases it.
 *                           BI_ERR_INVALID: prod_j n_fine[j] != B, n_groups[j] < 1, boundaries that are not strictly ascending
 *                           or leave [0, n_fine[j]]; Beeston-Barlow and unbinned contexts, as bi_expected_counts.
 *   bi_expected_coarse      out [P][C] (per_source = 0) or [P][S][C]: the expectation of every cell at every point, with the
 *                           screen of bi_expected_counts: a point outside the anchor box or with unphysical rates gets nan in
 *                           every cell and its bit in status [P] (nullable; 0 for a live point).  The corner rows are streamed
 *                           once per point and reduced as they arrive; no floating-point atomics: every sum runs in an order
 *                           fixed by the binning and the device, a repeated call is bitwise identical, and a point's result
 *                           does not depend on the other points of the call.
 *   bi_coarse_counts        out [n][C]: the counts of datasets dataset[0 .. n) (NULL: all of them, n = T) in the cells, from
 *                           the resident data in whichever form they are held (dense, or the non-empty-bin lists of
 *                           device-generated toys); a dataset index outside [0, T) is BI_ERR_INVALID.
 *   bi_expected_coarse_jacobian   mu [P][C], bit for bit bi_expected_coarse's total, and jac [P][d + S][C], its first
 *                           derivatives J_C = d mu_C / d theta over theta = (z_0 .. z_{d-1}, then the rate scales; bi_eval_hess's
 *                           order; rate_scale NULL: ones): what turns a covariance of the parameters into an uncertainty band of
 *                           a projection, sigma_C^2 = J_C^T Sigma J_C, and J_C J_C^T / mu_C is the Fisher information of the
 *                           likelihood at that binning, cell by cell.  One pass over the corner rows of a point for all
 *                           columns: the per-bin derivative columns of bi_eval_fisher are summed over the cells as they are
 *                           formed, and no per-bin derivative is ever written.  Rows of single-anchor axes are 0; on an anchor
 *                           the slopes are those of the cell the point is assigned to (bi_eval_grad's convention).  Screen,
 *                           status [P] (nullable) and order of every sum as bi_expected_coarse: a dead point gets nan in every
 *                           entry of mu and jac, a repeated call is bitwise identical, and a point's result does not depend on
 *                           the other points of the call.  Limit: 1 + d_eff + S <= 16 coefficient columns, BI_ERR_INVALID
 *                           naming the figure otherwise (as bi_eval_fisher).
 * Without a binning the last three return BI_ERR_STATE. */
int bi_expected_coarse_jacobian(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, double* mu, double* jac,
                                int32_t* status);
int bi_set_coarse_binning(bi_ctx* ctx, int k, const int32_t* n_fine, const int32_t* n_groups, const int32_t* bounds, int64_t* n_cells);
int bi_expected_coarse(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int per_source, double* out,
                       int32_t* status);
int bi_coarse_counts(bi_ctx* ctx, int64_t n, const int64_t* dataset, double* out);

/* Real-valued datasets: Asimov data (n_b = mu_b(truth), Cowan, Cranmer, Gross, Vitells, Eur. Phys. J. C 71 (2011) 1554) and
 * weighted histograms used as pseudo-data.  They live in a store of their own, per context and independent of its ordinary
 * data, which stay resident and keep their semantics (a count that is no integer is -inf in every other entry point):
 *   bi_set_real_counts       counts [T][B]: every count finite and >= 0, otherwise BI_ERR_INVALID naming dataset and bin;
 *                            T = 0 or counts = NULL drops the store
 *   bi_set_asimov_counts     H datasets made on the device: set h holds mu_b at truth (z[h], rate_scale[h]; rate_scale NULL:
 *                            ones), bit for bit the row bi_expected_counts(per_source = 0) returns there.  Every truth is
 *                            screened first (outside the anchor box, unphysical rates: BI_ERR_INVALID naming the truth), and
 *                            a truth whose expectation is negative or nan in some bin (sources that may go negative) is
 *                            refused as well
 *   bi_real_count_sets       the number of sets in the store (0: none)
 *   bi_download_real_counts  out [B] = set t
 * A new store replaces the previous one; on any refusal the previous one stays as it was.  bi_destroy and a new model
 * release it.  Binned likelihoods without Beeston-Barlow only: BI_ERR_INVALID with the reason otherwise.
 *
 * bi_eval_real: per point p, against set dataset[p] of the store (NULL: set 0; an index outside it: BI_ERR_INVALID),
 *   half_deviance [P]        sum_b  (mu_b - n_b) - n_b log(mu_b / n_b)        (n_b = 0: mu_b)
 *   grad [P][d + S] or NULL  sum_b  d_q mu_b (1 - n_b / mu_b)                 (n_b = 0: d_q mu_b)
 * q over z_0 .. z_{d-1}, then the rate scales; on an anchor the slope of the cell the point is assigned to (bi_eval_grad's
 * convention).  The log-likelihood ratio to the saturated model is -half_deviance: a constant below ll, summed bin by bin
 * without the cancellation of two log-likelihoods.  n_b > 0 with mu_b = 0 gives +inf, a negative or nan mu_b nan; points
 * outside the box or with unphysical rates get +inf and bi_eval_grad's status bits; grad is nan wherever the value is not
 * finite.  With grad, 1 + d + S <= 16 (BI_ERR_INVALID otherwise); value-only calls have no such limit.  At the truth of an
 * Asimov set the value and every slope are 0.0 exactly (the same fused multiply-add chain makes mu_b on both sides). */
int bi_set_real_counts(bi_ctx* ctx, int64_t T, const double* counts);
int bi_set_asimov_counts(bi_ctx* ctx, int64_t H, const double* z, const double* rate_scale);
int64_t bi_real_count_sets(bi_ctx* ctx);
int bi_download_real_counts(bi_ctx* ctx, int64_t t, double* out);
int bi_eval_real(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                 double* half_deviance, double* grad, int32_t* status);

/* The expected (Fisher) information of the binned Poisson likelihood at P truths, without data:
 *   info [P][F][F], F = d + S     I_qr = sum_b d_q mu_b d_r mu_b / mu_b      over the bins with mu_b > 0
 *   total [P] or NULL             sum_b mu_b
 *   unbounded [P][F] or NULL      the number of bins with mu_b == 0 and d_q mu_b != 0
 * q, r over z_0 .. z_{d-1}, then the rate scales (bi_eval_hess's order; rate_scale NULL: ones).  Minus the expectation of
 * bi_eval_hess's Hessian over data drawn at the point itself; every diagonal entry is a sum of non-negative terms and the
 * matrix is positive semi-definite by construction.  A bin that expects nothing and whose expectation does not move with any
 * parameter (a bin no template fills) adds nothing.  A bin that expects nothing but would with another value of parameter q
 * (a rate scale of 0 for the only source in the bin; a point on an anchor and a bin only the cell's other anchor fills)
 * holds unbounded information on q -- one event there would decide it: such a bin is left out of the sums of `info` and
 * counted in unbounded[p][q], and the caller decides what that means (blueice_amd.hessian.covariance_from_information: variance
 * 0).  A negative or nan mu_b in any bin (sources that may go negative) makes the point's whole matrix and its total nan.
 * Rows and columns of single-anchor axes are zero; on an anchor the matrix is that of the cell the point is assigned to
 * (bi_eval_grad's convention).  Points outside the anchor box or with unphysical rates get their bi_eval_grad status bit in
 * status [P] (nullable; 0 for a live point), a nan matrix, a nan total and zero counts.  The context needs a model and nothing
 * else: no dataset, no real-valued store, and none of them is touched.  The dense template rows are streamed once per point,
 * no floating-point atomics: a repeated call is bitwise identical and a point's result does not depend on the other points of
 * the call.  Limits: 1 + d_eff + S <= 16 coefficient columns (d_eff: the axes with more than one anchor), BI_ERR_INVALID
 * naming the figure otherwise; Beeston-Barlow and unbinned contexts: BI_ERR_INVALID, as bi_expected_counts.
 * bi_fisher_variant: the kernel variant bi_eval_fisher takes for D = d_eff + S first-order columns -- *G (nullable) the padded
 * 1 + D of {4, 8, 16}, *DM (nullable) the padded D of {4, 8, 16}; BI_ERR_INVALID when 1 + D > 16.  Needs no context. */
int bi_eval_fisher(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, double* info, double* total,
                   int64_t* unbounded, int32_t* status);
int bi_fisher_variant(int D, int* G, int* DM);

/* The batched profile-fit engine's inner loop (host code): P minimisations of F variables each advance in lock-step, every
 * optimiser iteration ONE evaluation call over the problems still running -- what replaces the reference's loops of sequential
 * scipy fits (bestfit_scipy, blueice/inference.py:131-178, inside one_parameter_interval / plot_likelihood_ratio, :332-443).
 * BFGS per problem (Hessian estimate in direct form, exact reduced steps at bounds), Armijo backtracking with a ladder of
 * three trial steps per call, box constraints lo / hi [F] (+-inf = none); `kinks` (n_kinks [F] counts, values concatenated,
 * ascending; NULL = none): points along a variable where the function has a kink -- the interior anchors of a shape parameter,
 * the morph is linear between them (pdf_morphers.py:67-70) -- at which both one-sided slopes are taken and steps end.
 *   bi_minimize_batched   over a caller's objective: fun(user, n, F, x [n][F], rows [n], f [n], g [n][F]) evaluates f and its
 *                         gradient for problems `rows` at `x`; non-zero return aborts.  Needs no context and no GPU.
 *   bi_fit_batched        with the context's likelihood as the objective, f = -ll (bi_eval_grad), no caller code between the
 *                         iterations: variable j is shape parameter var_index[j] (var_kind 0: z_i = x_j) or the rate
 *                         multiplier of source var_index[j] (var_kind 1: rate_scale_s = x_j * unit[p][s]); z0 [P][d] and
 *                         scale0 [P][S] are the problems' other settings, dataset [P] or NULL.  Points at which a
 *                         Beeston-Barlow assertion would fire count as nan (to be stepped around), rejected points as +inf.
 * x_out [P][F], f_out [P]; flags_out [P]: 1 converged (projected gradient below gtol, or the rounding floor), 2 stalled (no
 * descent step / crawling across a kink), 4 failed (the start was not finite); counters [4]: iterations, evaluation calls,
 * of which one-sided-slope calls, evaluations (bi_fit_batched) -- or NULL. */
typedef int (*bi_objective_fn)(void* user, int64_t n, int F, const double* x, const int64_t* rows, double* f, double* g);
int bi_minimize_batched(bi_objective_fn fun, void* user, int64_t P, int F, const double* x0, const double* lo, const double* hi,
                        const int32_t* n_kinks, const double* kinks, double gtol, int max_iter, double* x_out, double* f_out,
                        int32_t* flags_out, int64_t* counters);
int bi_fit_batched(bi_ctx* ctx, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                   const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                   const double* hi, const int32_t* n_kinks, const double* kinks, double gtol, int max_iter, double* x_out,
                   double* f_out, int32_t* flags_out, int64_t* counters);

/* Gaussian constraint terms inside the two native loops (bi_fit_batched_gauss below, bi_sample_stretch_gauss after
 * bi_sample_stretch): the log density is ll + p, with p a sum of normal log densities on the OPTIMISER VARIABLES x_v -- the
 * multiplier itself for var_kind 1, not rate_scale -- which is what the reference adds for add_rate_uncertainty /
 * add_shape_uncertainty and any Gaussian log_prior (blueice/likelihood.py:280-296,341-372).  Three more arrays:
 *   prior_mean [F], prior_sigma [F]   the term on variable v; prior_sigma[v] = +inf: no term on that variable
 *   prior_const [P] ([E] for the sampler) or NULL for 0: filled in by the caller with everything of p that does not depend on
 *                                     x -- the normalisation constants -log(sigma) - log(2 pi)/2 of the floating terms plus
 *                                     the complete priors of the problem's fixed parameters
 * The arithmetic, exactly (binary64, every operation rounded on its own, no fused multiply-add), for problem / ensemble e:
 *     p = prior_const[e]
 *     for v = 0 .. F-1 with finite prior_sigma[v]:  t = (x_v - prior_mean[v]) / prior_sigma[v]   (IEEE division)
 *                                                   p = p - 0.5 (t t)
 * A finite prior_sigma <= 0, or a NaN in any of the three arrays, returns BI_ERR_INVALID with the reason in bi_last_error
 * before anything is launched.  bi_fit_batched and bi_sample_stretch are these entry points without terms.
 *
 * bi_fit_batched_gauss: f = -(ll + p) and g_v gains + t_v / prior_sigma[v]; rejected points stay +inf with nan slopes, points
 * at which a Beeston-Barlow assertion would fire stay nan. */
int bi_fit_batched_gauss(bi_ctx* ctx, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                         const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                         const double* hi, const int32_t* n_kinks, const double* kinks, double gtol, int max_iter,
                         const double* prior_mean, const double* prior_sigma, const double* prior_const, double* x_out,
                         double* f_out, int32_t* flags_out, int64_t* counters);

/* ... against the real-valued store (bi_eval_real): f = half_deviance - p, `dataset` indexes the store; the three prior
 * arrays may all be NULL (no terms).  Needs no ordinary data. */
int bi_fit_batched_real(bi_ctx* ctx, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                        const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                        const double* hi, const int32_t* n_kinks, const double* kinks, double gtol, int max_iter,
                        const double* prior_mean, const double* prior_sigma, const double* prior_const, double* x_out,
                        double* f_out, int32_t* flags_out, int64_t* counters);

/* ---- source-wise (factored) binned models: one anchor grid per source --------------------------------------------------
 * The grid model above is ONE tensor product of all d shape axes: it holds prod_i n_i anchor models and a point reads
 * S 2^d rows.  A source-wise model lets every source morph over the axes IT responds to only (the reference's
 * source_wise_interpolation, for binned likelihoods): source s owns the axes O_s (ascending, e_s = |O_s|, possibly none;
 * every owned axis has at least two anchors), keeps p_s [n_{O_s[0]}] .. [n_{O_s[e_s - 1]}][B] template rows and as many
 * rates M_s in C order, and a point reads sum_s 2^e_s rows.  At (z [d], rs [S]) against counts n [B]:
 *     per axis           cell k and fraction t as everywhere (scipy's convention, the last cell closed)
 *     per source         corners numbered with the first own axis as the most significant bit; w_c = the product of t or
 *                        1 - t in own-axis order from 1.0; M_s(z) = sum_c M_s,c w_c left to right from 0.0; r_s = M_s(z) rs_s;
 *                        tau_s,b = sum_c w_c p_s,c,b, one fused multiply-add per corner from 0.0
 *     mu_b               = sum_s r_s tau_s,b, one fused multiply-add per source from 0.0
 *     ll                 = sum_b [n_b log mu_b - mu_b] - sum_b lgamma(n_b + 1)     (n_b = 0: -mu_b; n_b > 0, mu_b = 0: -inf)
 *     d ll / d rs_s      = M_s sum_b f_b tau_s,b,   f_b = n_b / mu_b - 1  (n_b = 0: -1)
 *     d ll / d z_i       = sum_{s: i in O_s} rs_s (M_s sum_b f_b ups_s,i,b + d_i M_s sum_b f_b tau_s,b),
 *                        ups_s,i,b = sum_c d_i w_c p_s,c,b; an axis nobody owns has slope 0; on an anchor the slope of the cell
 *                        the point is assigned to (bi_eval_grad's convention)
 * Early exits, in this order: dataset outside [0, T) BI_ST_BAD_DATASET; a z_i outside its axis' anchors or nan, on any of
 * the d axes, BI_ST_OUT_OF_BOUNDS; an r_s not in [0, inf) BI_ST_UNPHYSICAL.  All three give ll = -inf.  Wherever ll is not
 * finite the gradient entries are nan.  A point's result does not depend on the batch it is evaluated in, and repeated
 * calls agree bit for bit.
 *
 * Limits: d <= 32, S <= 8, e_s <= 3 (a source that responds to more axes belongs on the grid model).  Out of scope, and
 * refused where they can be asked for: sources that may go negative (template entries must be finite and >= 0),
 * Beeston-Barlow.  Unbinned data: the event store of bi_sourcewise_score_events / bi_sourcewise_events_begin below, a second form
 * of the data with which bi_eval_factored and bi_fit_batched_factored are the extended unbinned likelihood.  The store's counts
 * are dense doubles, [T][B]: the caller's (bi_factored_set_counts) or toys
 * drawn on the device at truth points of this model (bi_sourcewise_generate_toys below, with the expectation per bin and the
 * goodness-of-fit sums).
 *
 * The model is a store of its own inside the context, beside the grid model and released by bi_destroy (or the next
 * bi_factored_begin).  It does not make the context "ready": every other entry point of this header keeps refusing a context
 * without a grid model with BI_ERR_STATE, and none of them reads this store.
 *   bi_factored_begin        n_anchor [d], anchor_z: the axes' anchors back to back; n_own [S] = e_s; own_axes: the sources' O_s
 *                            back to back.  Drops the previous source-wise model and its counts.
 *   bi_factored_set_anchor   row `local_index` (C order over the source's own axes) of source s: ps_row [B] and its rate mu;
 *                            in any order, each anchor exactly once (a second upload of one: BI_ERR_INVALID)
 *   bi_factored_end          BI_ERR_STATE naming the first anchor that is missing
 *   bi_factored_set_counts   counts [T][B], T >= 1, dense doubles, every count finite and >= 0 (a count that is no integer
 *                            gives -inf, scipy's poisson.logpmf); replaces earlier counts; sum_b lgamma(n_b + 1) per dataset is
 *                            computed once, here
 *   bi_eval_factored         ll [P], grad [P][d + S] or NULL (values only: the same bits of ll), status [P] or NULL;
 *                            rate_scale NULL: ones; dataset NULL: dataset 0
 *   bi_fit_batched_factored  bi_fit_batched_gauss with this likelihood as the objective: the same optimiser and the same
 *                            constraint terms; the three prior arrays may all be NULL (no terms); `dataset` indexes the
 *                            counts of bi_factored_set_counts; var_index refers to the d axes and S sources of this model */
int bi_factored_begin(bi_ctx* ctx, int d, const int32_t* n_anchor, const double* anchor_z, int S, int64_t B,
                      const int32_t* n_own, const int32_t* own_axes);
int bi_factored_set_anchor(bi_ctx* ctx, int s, int64_t local_index, const double* ps_row, double mu);
int bi_factored_end(bi_ctx* ctx);
int bi_factored_set_counts(bi_ctx* ctx, int64_t T, const double* counts);
int bi_eval_factored(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                     double* grad, int32_t* status);
int bi_fit_batched_factored(bi_ctx* ctx, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                            const double* scale0, const double* unit, const int64_t* dataset, const double* x0,
                            const double* lo, const double* hi, const int32_t* n_kinks, const double* kinks, double gtol,
                            int max_iter, const double* prior_mean, const double* prior_sigma, const double* prior_const,
                            double* x_out, double* f_out, int32_t* flags_out, int64_t* counters);

/* ... second derivatives of a source-wise model.  theta = (z_0 .. z_{d-1}, rs_0 .. rs_{S-1}), F = d + S.  Source s is multilinear
 * over its own axes, so with the per-bin basis columns tau_s, ups_s,j (above) and chi_s,jk = sum_c d_j d_k w_c p_s,c,b (j < k;
 * d_jj = 0) every derivative of mu_b is a fixed combination of at most sum_s (1 + e_s) <= 32 columns, whatever d is:
 *     d_q mu_b = sum_a C_qa u_a,b      u = (tau_s, ups_s,j);   C[rs_s, tau_s] = M_s;   for i = O_s[j]:   C[z_i, tau_s] += rs_s d_j M_s,
 *                                      C[z_i, ups_s,j] += rs_s M_s
 * The device forms the linear sums L_x = sum_b f_b x_b over x = tau_s, ups_s,j, chi_s,jk and the Gram matrix of u (in panels of
 * whole sources where it exceeds the registers of a thread), the host contracts them in extended precision in a fixed order.
 *   bi_eval_sourcewise_hess     ll [P], grad [P][F]: bit for bit what bi_eval_factored returns with a gradient, and the same status
 *                               [P] (nullable), early exits and defaults.  hess [P][F][F] = -C Q C^T + the second-order terms,
 *                               Q = sum_b (n_b / mu_b^2) u u^T:
 *                                   (rs_s, z_i)   d_j M_s L_tau_s + M_s L_ups_s,j
 *                                   (z_i, z_i)    2 rs_s d_j M_s L_ups_s,j
 *                                   (z_i, z_k)    rs_s (d_j d_k M_s L_tau_s + d_j M_s L_ups_s,k + d_k M_s L_ups_s,j + M_s L_chi_s,jk)
 *                               summed over the sources that own the axes; full and exactly symmetric (written from one
 *                               triangle); rows and columns of axes nobody owns are 0; nan wherever ll is not finite; on an
 *                               anchor the Hessian of the cell the point is assigned to.  Needs counts (BI_ERR_STATE without).
 *   bi_eval_sourcewise_fisher   bi_eval_fisher's contract for this model: info [P][F][F] = C Q' C^T, Q' = sum_{mu_b > 0} u u^T / mu_b,
 *                               positive semi-definite by construction; total [P] or NULL = sum_b mu_b, from the fma chain of
 *                               the value kernel's mu_b; unbounded [P][F] or NULL = the number of bins with mu_b == 0 and
 *                               d_q mu_b != 0, which are left out of info; rejected points: a nan matrix, a nan total, zero
 *                               counts and their status bit (box and rate tests alone: no dataset).  Needs the source-wise
 *                               model and nothing else: no counts are read or touched.
 * Both: P = 0 returns BI_OK with no device work; no floating-point atomics; a repeated call is bitwise identical and a point's
 * result does not depend on the batch it is evaluated in.  The limits are the model's own (d <= 32, S <= 8, e_s <= 3).
 * (The names say "sourcewise": these two are layers over the model, not parts of the bi_factored_* store's life cycle.) */
int bi_eval_sourcewise_hess(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                            double* grad, double* hess, int32_t* status);
int bi_eval_sourcewise_fisher(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, double* info, double* total,
                              int64_t* unbounded, int32_t* status);

/* ... the expectation per bin, goodness of fit and toy ensembles of a source-wise model.  mu_b is the chain stated above, to the
 * bit: w_c from 1.0 in own-axis order, tau_s,b one fused multiply-add per corner from 0.0, M_s left to right, r_s = M_s rs_s,
 * mu_b one fused multiply-add per source from 0.0.  rate_scale NULL: ones.
 *   bi_sourcewise_expected_counts   out [P][B] = mu_b, or with per_source != 0 out [P][S][B] = r_s tau_s,b (ONE multiplication of
 *                               the two; the S rows sum to mu_b up to rounding).  Rows of a rejected point -- the box test on
 *                               all d axes, then the rates; no dataset test -- are nan in every entry; no status is reported.
 *                               Needs the source-wise model and nothing else: no counts are read or touched.  The points are
 *                               processed in sub-batches: the device scratch is bounded (64 MiB of rows, or one point's) however
 *                               large P B is.
 *   bi_eval_sourcewise_gof      bi_eval_gof's contract on the store's dense counts: per point p, against dataset[p] (NULL: dataset 0),
 *                                   half_deviance [P]   sum_b  (mu_b - n_b) - n_b log(mu_b / n_b)     (n_b = 0: mu_b)
 *                                   pearson [P]         sum_b  (n_b - mu_b)^2 / mu_b                  (n_b = 0: mu_b)
 *                               both summed bin by bin without the cancellation of two log-likelihoods.  n_b = 0 and mu_b = 0
 *                               adds 0 to both; wherever ll at the point is -inf (an event where mu_b = 0, a count that is
 *                               negative or no integer) BOTH are +inf, wherever it is nan both are nan.  Early exits in
 *                               bi_eval_factored's order and with its status bits (status [P] or NULL): dataset outside [0, T),
 *                               box, rates; all three give +inf in both.  Needs counts (BI_ERR_STATE without).
 *   bi_sourcewise_generate_toys     T = sum_h n_toys[h] toys at H truths, n_toys[h] >= 0 of them at (z[h], rate_scale[h]),
 *                               truth-major; z [H][d] (NULL when d = 0), rate_scale [H][S] or NULL; 1 <= T < 2^31.  Toy t of the
 *                               call is toy D = toy_offset + t of the seed's ensemble (the context parameter), and its counts are
 *                               ALWAYS stream A of bi_generate_toys' text with mu_b the expectation above: bins 2q and 2q + 1
 *                               share one Philox block, a bin with 0 < mu_b < 10 draws poisson_small, one with mu_b >= 10
 *                               poisson_ptrs with its own bin number, mu_b = 0 gives 0.  The ensemble does not depend on how
 *                               truths are grouped into calls: the toys of truth h are bit for bit those of an H = 1 call with
 *                               toy_offset advanced by the toys before it.  All truths are validated before the store changes:
 *                               one outside the anchor box, or with a rate outside [0, inf), refuses the whole call with
 *                               BI_ERR_INVALID naming the truth ("... (truth 1): point is outside the anchor box") and the
 *                               counts held so far stay usable.  The toys REPLACE the store's counts as T dense datasets
 *                               ([T][Bp] doubles on the device, Bp = B rounded up to 512), with sum_b lgamma(n_b + 1) per
 *                               dataset as bi_factored_set_counts computes it; where those T Bp 8 bytes cannot be allocated the
 *                               call fails with BI_ERR_NOMEM and the old counts stay.  Scratch: H Bp doubles each for mu and
 *                               exp(-mu): callers bound H per call.  Needs no counts.
 *   bi_sourcewise_download_counts   out [B] = dataset t of whatever the store holds (uploaded counts or toys); t outside [0, T):
 *                               BI_ERR_INVALID.
 * All four: P = 0 / H = 0 returns BI_OK with no device work; no floating-point atomics; a repeated call is bitwise identical
 * and a point's result does not depend on the batch it is evaluated in.  The limits are the model's own. */
int bi_sourcewise_expected_counts(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int per_source, double* out);
int bi_eval_sourcewise_gof(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                           double* half_deviance, double* pearson, int32_t* status);
int bi_sourcewise_generate_toys(bi_ctx* ctx, int64_t H, const double* z, const double* rate_scale, const int64_t* n_toys,
                                uint64_t seed);
int bi_sourcewise_download_counts(bi_ctx* ctx, int64_t t, double* out /*[B]*/);

/* ... and its coarse views: the expectation and the data summed over tensor-product groups of fine bins, the layer that
 * bi_set_coarse_binning ... bi_coarse_counts are for the grid model, without a bin tensor in between.
 *   bi_sourcewise_set_coarse_binning   bi_set_coarse_binning's contract over the B bins of the source-wise model (the product of
 *                               n_fine must be that B; the same boundaries, errors and n_cells).  The binning is a state of its
 *                               own beside the grid model's: neither call touches the other's.  k = 0 clears it; a new
 *                               bi_factored_begin releases it.
 *   bi_sourcewise_expected_coarse   out [P][C] (per_source = 0) or [P][S][C]: the cells of mu_b, or of r_s tau_s,b, formed per fine
 *                               bin with the bits of bi_sourcewise_expected_counts and summed in an order that the binning and
 *                               the device fix (never the number of points).  The screen is bi_sourcewise_expected_counts's; a
 *                               dead point gets nan in every cell and its bit in status [P] (nullable).
 *   bi_sourcewise_coarse_counts out [n][C]: the counts of datasets dataset[0 .. n) (NULL: all of them, n = T) of the store --
 *                               uploaded or drawn on the device -- in the cells; sums of integer counts are exact.  A dataset
 *                               outside [0, T): BI_ERR_INVALID.
 *   bi_sourcewise_expected_coarse_jacobian   the cells and their first derivatives over theta = (z [d], then rate_scale [S]), the
 *                               order of bi_eval_factored's gradient, in one pass over the point's rows.  With R = per_source ? S : 1
 *                               and F = d + S: mu [P][R][C], jac [P][R][F][C].  per_source = 0: mu has the bits of
 *                               bi_sourcewise_expected_coarse's total; jac[p][d + s] = M_s T_s and jac[p][i] = the sum over the
 *                               sources s that own axis i (ascending) of rs_s (M_s Y_s,j + dM_s,j T_s), with T_s, Y_s,j the cell
 *                               sums of tau_s,b and d tau_s,b / d z_i the device forms and M_s the source's rate at rate scale 1;
 *                               an axis nobody owns has a row of exactly 0.0.  per_source = 1: mu[p][s] = r_s T_s (equal to
 *                               bi_sourcewise_expected_coarse's per-source cells to rounding, not to the bit) and jac[p][s] holds
 *                               the single terms of source s: every entry of another source's scale, or of an axis s does not
 *                               own, is exactly 0.0, and the per-source rows summed over s in ascending order in long double
 *                               reproduce the per_source = 0 rows bit for bit.  The contraction runs per cell on the host in long
 *                               double; no limit on the columns beyond the model's own.  The screen and the status are
 *                               bi_sourcewise_expected_coarse's; a dead point is nan throughout mu and jac.  mu or jac NULL with
 *                               P > 0: BI_ERR_INVALID.  On an anchor the slopes are those of the cell the point is assigned to.
 * The last three without a binning: BI_ERR_STATE.  No floating-point atomics; a repeated call is bitwise identical and a point's
 * cells do not depend on the batch it is evaluated in.  The real-valued store has no coarse view. */
int bi_sourcewise_set_coarse_binning(bi_ctx* ctx, int k, const int32_t* n_fine, const int32_t* n_groups, const int32_t* bounds,
                                     int64_t* n_cells);
int bi_sourcewise_expected_coarse(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int per_source, double* out,
                                  int32_t* status);
int bi_sourcewise_expected_coarse_jacobian(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int per_source,
                                           double* mu, double* jac, int32_t* status);
int bi_sourcewise_coarse_counts(bi_ctx* ctx, int64_t n, const int64_t* dataset, double* out);

/* ... and real-valued datasets of a source-wise model: Asimov data (n_b = mu_b(truth)) and weighted histograms, the layer that
 * bi_set_real_counts ... bi_fit_batched_real are for the grid model.  The store is [T][Bp] doubles (Bp = B rounded up to 512,
 * zero behind B) inside the source-wise model BESIDE its ordinary counts, which stay resident and keep scipy's integer
 * semantics; nothing else reads it, and none of these calls needs ordinary counts.  bi_factored_begin and bi_destroy release
 * it.  A new store replaces the previous one; on ANY refusal the previous one stays as it was.
 *   bi_sourcewise_set_real_counts      counts [T][B], every one finite and >= 0: otherwise BI_ERR_INVALID naming dataset and
 *                                  bin.  T = 0 or counts = NULL drops the store.
 *   bi_sourcewise_set_asimov_counts    H >= 1 sets, set h = mu_b at truth (z[h], rate_scale[h]) (rate_scale NULL: ones), written
 *                                  on the device straight into the store by the kernel of bi_sourcewise_expected_counts: bit
 *                                  for bit the row that call returns with per_source = 0.  All truths are screened (box on all
 *                                  d axes, then the rates) before the store changes: a refused call returns BI_ERR_INVALID
 *                                  naming the truth ("... (truth 1): point is outside the anchor box"), as does a truth whose
 *                                  expectation is not finite in some bin.  BI_ERR_NOMEM where the H Bp 8 bytes cannot be
 *                                  allocated; the old store stays.
 *   bi_sourcewise_real_count_sets      the number of sets in the store (0: none)
 *   bi_sourcewise_download_real_counts out [B] = set t; t outside the store: BI_ERR_INVALID; no store: BI_ERR_STATE
 *   bi_eval_sourcewise_real        bi_eval_real's contract on this model: per point p, against set dataset[p] (NULL: set 0),
 *                                      half_deviance [P]   sum_b  (mu_b - n_b) - n_b log(mu_b / n_b)         (n_b = 0: mu_b)
 *                                      grad [P][d + S]     sum_b  d_q mu_b (1 - n_b / mu_b)                  (n_b = 0: d_q mu_b)
 *                                  grad may be NULL; it is formed from per-source sums by bi_eval_factored's chain rule, in its
 *                                  fixed order.  There is no integer test on n_b.  n_b > 0 where mu_b = 0 gives +inf, an
 *                                  expectation that comes out negative or nan gives nan; the gradient is nan wherever the value
 *                                  is not finite.  Box and rate rejections give +inf with bi_eval_factored's status bits
 *                                  (status [P] or NULL); a dataset index outside the store is BI_ERR_INVALID for the whole
 *                                  call, no store at all BI_ERR_STATE.  mu_b is the chain stated above to the bit, so at the
 *                                  truth of an Asimov set mu_b == n_b and the value and every gradient entry are exactly 0.0.
 *                                  No 16-column limit: the limits are the model's own (d <= 32, S <= 8, e_s <= 3).  The value
 *                                  of a call without the gradient has the bits of the value of the call with it; P = 0 returns
 *                                  BI_OK with no device work; no floating-point atomics; a repeated call is bitwise identical
 *                                  and a point's result does not depend on the batch it is evaluated in.
 *   bi_fit_batched_sourcewise_real bi_fit_batched_real's signature and contract with this evaluation as the objective:
 *                                  f = half_deviance - p, `dataset` [P] or NULL indexes the real-valued store (outside it:
 *                                  BI_ERR_INVALID), and prior_mean / prior_sigma / prior_const may all be NULL (no terms). */
int bi_sourcewise_set_real_counts(bi_ctx* ctx, int64_t T, const double* counts /*[T][B]*/);
int bi_sourcewise_set_asimov_counts(bi_ctx* ctx, int64_t H, const double* z, const double* rate_scale);
int64_t bi_sourcewise_real_count_sets(bi_ctx* ctx);
int bi_sourcewise_download_real_counts(bi_ctx* ctx, int64_t t, double* out /*[B]*/);
int bi_eval_sourcewise_real(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                            double* half_deviance, double* grad, int32_t* status);
int bi_fit_batched_sourcewise_real(bi_ctx* ctx, int64_t P, int F, const int32_t* var_kind, const int32_t* var_index,
                                   const double* z0, const double* scale0, const double* unit, const int64_t* dataset,
                                   const double* x0, const double* lo, const double* hi, const int32_t* n_kinks,
                                   const double* kinks, double gtol, int max_iter, const double* prior_mean,
                                   const double* prior_sigma, const double* prior_const, double* x_out, double* f_out,
                                   int32_t* flags_out, int64_t* counters);

/* The ensemble sampler: n_steps steps of Goodman & Weare's affine-invariant stretch move for E independent ensembles of W
 * walkers over F variables, the context's log likelihood as the log density -- what the reference hands to emcee as
 * n_walkers x n_steps scalar likelihood calls (bestfit_emcee, blueice/inference.py:254-321).  The variables are described as
 * for bi_fit_batched (var_kind / var_index, z0 [E][d], scale0 [E][S], unit [E][S], dataset [E] or NULL: ensemble e samples
 * the likelihood of dataset[e] with its other settings z0[e], scale0[e]).  x0 [E][W][F]: the start; lo / hi [F]: the box
 * (+-inf = none).  Between the likelihood evaluations nothing leaves the device: a half-step is k_stretch_propose, the device
 * planner and evaluation kernels of bi_plan_points_resident / bi_run_plan on the proposal buffers, k_stretch_accept; the host
 * reads the plan's status OR once per half-step, and chain [n_steps][E][W][F], ll [n_steps][E][W] (state of every walker after
 * step t and its log likelihood) and n_accepted [E][W] once at the end.  counters [4] or NULL: half-steps, likelihood
 * evaluations, accepted moves, evaluation launches.
 *
 * The random stream and the arithmetic, exactly (binary64, every operation rounded on its own, no fused multiply-add):
 *   step t = 0 .. n_steps-1, half h = 0, 1: walkers k in [h W/2, (h+1) W/2) of every ensemble move, the others are the
 *   complementary set; the state they see is the one the previous half-step left.  For ensemble e and moving walker k
 *     (r0, r1, r2, r3) = Philox4x32-10(counter = (k, first_ensemble + e, t, 0x53545200 | h), key = (seed mod 2^32, seed >> 32))
 *     (round constants 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85: per round, from counter (c0, c1, c2, c3)
 *      and key (k0, k1):  c0' = hi(0xCD9E8D57 c2) ^ c1 ^ k0, c1' = lo(0xCD9E8D57 c2), c2' = hi(0xD2511F53 c0) ^ c3 ^ k1,
 *      c3' = lo(0xD2511F53 c0), then the key is incremented; ten rounds)
 *     u_z = ((r0 >> 5) 2^26 + (r1 >> 6)) 2^-53              uniform in [0, 1)
 *     j   = (1 - h) W/2 + ((r2 (W/2)) >> 32)                the partner, in the other half (64-bit product)
 *     u_a = (r3 + 0.5) 2^-32
 *     g = (a - 1) u_z + 1;  z = (g g) / a                    (IEEE division)
 *     y_i = x_j,i + z (x_k,i - x_j,i)                        i.e. s = x_k,i - x_j,i; p = z s; y_i = x_j,i + p
 *   the point evaluated is z_i = y_v for a shape variable, rate_scale_s = y_v unit[e][s] for a rate multiplier.  The move is
 *   accepted iff lo <= y <= hi in every variable, ll(y) is finite with status word 0, and
 *     log(u_a) < (((F - 1) log z) + ll(y)) - ll(x_k)
 *   (proposals outside the anchor box or with unphysical rates are -inf as in bi_eval and never accepted; so is a point at
 *   which a Beeston-Barlow assertion would fire).  Ensemble e of a call is ensemble first_ensemble + e of the seed's stream:
 *   a joint run over E ensembles and E runs of one ensemble each draw the same numbers.
 * Errors (BI_ERR_INVALID unless noted, reason in bi_last_error): W odd or < 2, F < 1, a <= 1, a start walker outside [lo, hi]
 * or whose log likelihood is not finite (so no stored position ever lies outside the box), a chain larger than the free
 * device memory (BI_ERR_NOMEM), and whatever bi_plan_points_resident
 * refuses (Beeston-Barlow points that need exact totals, infinite rates of sources that may go negative).  Read-only parameter
 * n_sampler_half_steps counts the half-steps run on the context. */
int bi_sample_stretch(bi_ctx* ctx, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                      const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                      const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble, double* chain, double* ll,
                      int64_t* n_accepted, int64_t* counters);
/* ... with Gaussian constraint terms (prior_mean / prior_sigma [F], prior_const [E] or NULL: see bi_fit_batched_gauss): the
 * quantity held per walker, compared in the accept step -- log(u_a) < (((F - 1) log z) + (ll(y) + p(y))) - (ll(x_k) + p(x_k)) --
 * and written to `ll` is the log density ll + p (one addition, after p has been summed as above); the start walkers' values
 * include it, and it is the density that must be finite at the start and at an accepted proposal.  p of a proposal is
 * computed on the device from the proposal's coordinates: nothing more crosses to the host inside a half-step.  With every
 * prior_sigma +inf and prior_const NULL the chain is bit for bit that of bi_sample_stretch. */
int bi_sample_stretch_gauss(bi_ctx* ctx, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index,
                            const double* z0, const double* scale0, const double* unit, const int64_t* dataset, const double* x0,
                            const double* lo, const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble,
                            const double* prior_mean, const double* prior_sigma, const double* prior_const, double* chain,
                            double* ll, int64_t* n_accepted, int64_t* counters);

/* ... of a source-wise model (bi_factored_begin above), with a planner on the device between the staged points and the work items
 * of the evaluation kernel.  The geometry that bi_eval_factored's host screen reads -- anchors, own axes, row strides, the
 * anchors' rates, sum_b lgamma(n_b + 1) per dataset -- has a device copy (uploaded by bi_factored_end; the sums by
 * bi_factored_set_counts and bi_sourcewise_generate_toys), and one kernel turns n points into status words and descriptors: no
 * descriptor crosses the bus, and no result is read to size a launch.
 *   bi_eval_sourcewise_planned    bi_eval_factored's values-only contract through that planner: z [P][d], rate_scale [P][S] or
 *                                 NULL (ones), dataset [P] or NULL (dataset 0) are uploaded as they are; ll [P] and status [P]
 *                                 (or NULL) are bit for bit bi_eval_factored's -- the early exits in its order with its bits and
 *                                 ll = -inf, the same blocks per item and sub-batches.  P = 0: BI_OK without device work;
 *                                 BI_ERR_STATE without counts.  A rejected point streams no row.
 *   bi_sample_stretch_sourcewise  bi_sample_stretch_gauss's arguments, random stream, arithmetic and acceptance rule (above) with
 *                                 this model's likelihood as the log density; the three prior arrays may all be NULL (no terms);
 *                                 var_index refers to the d axes and S sources of this model, `dataset` [E] (or NULL) to the
 *                                 sets of bi_factored_set_counts or of the toy generator.  The same argument errors, reported
 *                                 under this name.  A half-step is k_stretch_propose, the planner, the evaluation kernel
 *                                 (values only), k_finish and k_stretch_accept, queued on one stream: after the start -- whose
 *                                 log densities and status words are read back once, to refuse a walker outside [lo, hi] or of
 *                                 zero likelihood -- the host reads nothing and waits for nothing until the one copy of chain, ll
 *                                 and n_accepted at the end.  counters [5] or NULL: [0] half-steps, [1] likelihood evaluations,
 *                                 [2] accepted moves, [3] launches (counted on the host from what was queued), [4] stream
 *                                 synchronisations inside the step loop: 0.  n_sampler_half_steps advances.  The chain must fit
 *                                 the free device memory (BI_ERR_NOMEM).  No floating-point atomics: a repeated call gives the
 *                                 same bits, and ensemble e is ensemble first_ensemble + e of the seed's stream whatever E is. */
int bi_eval_sourcewise_planned(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                               double* ll, int32_t* status);
int bi_sample_stretch_sourcewise(bi_ctx* ctx, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index,
                                 const double* z0, const double* scale0, const double* unit, const int64_t* dataset,
                                 const double* x0, const double* lo, const double* hi, int64_t n_steps, double a, uint64_t seed,
                                 int64_t first_ensemble, const double* prior_mean, const double* prior_sigma,
                                 const double* prior_const, double* chain, double* ll, int64_t* n_accepted, int64_t* counters);

/* ... and the non-empty-bin form of its data.  The store's counts are dense, and every evaluation of every point walks all B
 * bins; data and toys of a large binned analysis hold events in a small fraction of them.  Templates of a source-wise model are
 * finite and >= 0 and rates outside [0, inf) are BI_ST_UNPHYSICAL, so mu_b >= 0 in every bin, and for dataset t with the list
 * Z_t = {b : n_b != 0} (ascending bins)
 *     ll = sum_{b in Z_t} n_b log mu_b  -  sum_s lambda_s  -  sum_b lgamma(n_b + 1),     lambda_s = r_s sum_c w_c R_{s,c}
 * holds without any condition: corners c ascending, one fma per corner from 0.0; sources ascending; R_{s,c} the total of anchor
 * row (s, c) over ALL bins, summed once in long double by bi_factored_set_anchor and rounded to double; the sum of lambda_s and
 * of lgamma is one number per point, subtracted once.  mu_b and the gradient's columns are the dense route's fma chains; the
 * gradient uses g_b = n_b (1 / mu_b) at the listed bins:
 *     d ll / d rs_s = M_s (sum_Z g tau_s - N_s),   N_s = sum_c w_c R_{s,c}
 *     d ll / d z_i  = sum_{s: i in O_s} rs_s [M_s (sum_Z g ups_s,i - d_i N_s) + d_i M_s (sum_Z g tau_s - N_s)]
 * A listed bin with mu_b = 0 or a listed count that is no integer gives -inf, and the gradient is nan wherever ll is not finite;
 * status words and early exits are unchanged.  The results agree with the dense route's to rounding, not bit for bit.
 *   bi_sourcewise_build_nonempty   builds the form for all T datasets of the store as it stands (BI_ERR_STATE without counts): the
 *                                  lists, and per dataset a compacted copy of all the model's rows over its list, padded with
 *                                  zeros to whole tiles of tile_bins (at least one), the compacted counts beside it.  nnz [T] (or
 *                                  NULL) receives the list lengths.  BI_ERR_INVALID, naming the bytes, when the copies would take
 *                                  more than compact_budget: nothing is built then and the context goes on evaluating densely.
 *   bi_sourcewise_drop_nonempty    releases the form.  So does everything that replaces the counts or the model:
 *                                  bi_factored_begin, bi_factored_set_counts, bi_sourcewise_generate_toys.
 * Where the form is built and the parameter sourcewise_form is 1 (the default), bi_eval_factored (value and gradient; with it
 * bi_fit_batched_factored, whose objective it is), bi_eval_sourcewise_planned and bi_sample_stretch_sourcewise run on it, their
 * signatures and contracts unchanged: a point's bits do not depend on the batch or on the other datasets of the call (an item's
 * blocks follow from its own list's length), a values-only call gives the bits of the call with the gradient, the planned route
 * and the sampler equal the host route bit for bit.  Every other source-wise call keeps reading the dense store, which stays
 * resident and valid.  Nothing builds the form unless asked: a context that never calls bi_sourcewise_build_nonempty runs the
 * code it ran without it. */
int bi_sourcewise_build_nonempty(bi_ctx* ctx, int64_t* nnz /*[T] or NULL*/);
int bi_sourcewise_drop_nonempty(bi_ctx* ctx);

/* ... and UNBINNED data: the event store of a source-wise model (the reference's source_wise_interpolation for unbinned
 * likelihoods).  Per anchor row of the model the store holds the pdf value of every event, [rows][columns] with
 * rows = sum_s prod_{i in O_s} n_i, and T event sets side by side in the layout of bi_score_event_sets: set t at the columns
 * [first_t, first_t + N_t), every first_t even, every set padded to whole tiles of tile_bins behind its events and to at least
 * one tile; N_t = 0 is allowed.  Events keep the caller's order.  With it
 *     tau_s,e = sum_c w_c p_s,c,e, ups_s,j,e = sum_c d_j w_c p_s,c,e      the fma chains of the binned route, per event
 *     lam_e   = sum_s r_s tau_s,e      one fma per source from 0.0; a source whose tau_s,e is nan is left out of lam_e and of its
 *                                      own sums for that event (numpy.nansum)
 *     clamped = outlier != 0 and not (lam_e > 0):  lam_e := outlier, g_e := 0;   otherwise g_e = 1 / lam_e
 *     ll      = sum_e log lam_e - sum_s r_s
 *     d ll / d rs_s = M_s (sum_e g tau_s - 1)
 *     d ll / d z_i  = sum_{s: i in O_s} rs_s [M_s sum_e g ups_s,i + d_i M_s (sum_e g tau_s - 1)]
 * With outlier = 0 an event with lam_e = 0 gives ll = -inf; the gradient is nan wherever ll is not finite.  Columns behind N_t
 * are masked by index.  A point's bits do not depend on its batch or on the other sets of the call (an item's blocks follow from
 * its own set's length), a values-only call gives the bits of the call with the gradient, repeated calls agree bit for bit, and
 * a store scored on the device and the same values uploaded row by row give the same bits.
 *   bi_sourcewise_events_begin     T sets of n_events [T] events, pdf values scored on the host.  Needs a finished source-wise
 *   bi_sourcewise_events_set_row   model for its geometry and rates; the model's own rows are not read.  Row `local_index` of
 *   bi_sourcewise_events_end       source s: values [sum_t N_t], set after set; finite or nan (+-inf: BI_ERR_INVALID); each row
 *                                  exactly once (a second upload: BI_ERR_INVALID; _end names the first missing row, BI_ERR_STATE)
 *   bi_sourcewise_score_events     the model's rows are density histograms over the analysis space (B = histogram bins) and the
 *                                  store is filled on the device with bi_score_events' two methods and contract: 0 'piecewise'
 *                                  takes edges, 1 'linear' bin centres, coords [k][N] (N = offsets[T]) arrive clipped and
 *                                  finite.  Every stored value has the bits bi_score_events gives for that row, and those of
 *                                  HistogramPdfSource.pdf on the host -- except that for 'linear' with k = 2, where scipy's
 *                                  RegularGridInterpolator associates the products in a routine of its own, the store follows
 *                                  scipy (bi_score_events differs from it by a rounding there).  BI_ERR_INVALID when the grid
 *                                  does not describe B bins
 *   bi_sourcewise_drop_events      releases the store; so does bi_factored_begin
 *   bi_sourcewise_event_set_counts counts [T] = N_t
 *   bi_sourcewise_download_event_set   (for tests) out [rows][N_t]: the stored values of set t
 * The store's bytes are bounded by compact_budget: beyond it the call fails with BI_ERR_INVALID naming the bytes and nothing is
 * built.  Read-only parameters sourcewise_events_ready, sourcewise_events_bytes, sourcewise_event_sets.
 * While a store exists (from _events_begin on) the context is an unbinned source-wise likelihood: bi_eval_factored and
 * bi_fit_batched_factored evaluate it, signatures unchanged, `dataset` indexing the event sets (an index >= T:
 * BI_ST_BAD_DATASET); every other source-wise entry point (bi_factored_set_counts, bi_sourcewise_generate_toys, the Hessian, the
 * Fisher information, goodness of fit, expectations, coarse views, the real-valued store, bi_sourcewise_build_nonempty,
 * bi_eval_sourcewise_planned, bi_eval_sourcewise_scan, bi_sample_stretch_sourcewise, bi_grid_reduce_sourcewise) refuses with
 * BI_ERR_STATE naming the event store.  A context that never creates one runs the code it ran before. */
int bi_sourcewise_events_begin(bi_ctx* ctx, int64_t T, const int64_t* n_events, double outlier_likelihood);
int bi_sourcewise_events_set_row(bi_ctx* ctx, int s, int64_t local_index, const double* values);
int bi_sourcewise_events_end(bi_ctx* ctx);
int bi_sourcewise_score_events(bi_ctx* ctx, int method, int k, const int32_t* n_grid, const double* grid, int64_t T,
                               const int64_t* offsets, const double* coords, double outlier_likelihood);
int bi_sourcewise_drop_events(bi_ctx* ctx);
int bi_sourcewise_event_set_counts(bi_ctx* ctx, int64_t* counts);
int bi_sourcewise_download_event_set(bi_ctx* ctx, int64_t t, double* out);

/* ... and event-level toys drawn on the device: T = sum_h n_toys[h] toys at H truths (z [H][d], rate_scale [H][S] or NULL),
 * truth-major, scored into the event store above.  The toys become the context's T event sets in that store's layout (every set
 * padded to whole tiles and to at least one, the padding zero and masked by index), so bi_eval_factored,
 * bi_fit_batched_factored and bi_eval_sourcewise_events_hess run on them as on any store.  The model must be a finished
 * source-wise model whose rows are density histograms over `edges` (bi_sourcewise_score_events' condition); method 0
 * 'piecewise' / 1 'linear' is the lookup that scores the events (1 needs three edges per axis).
 * The stream is bi_simulate_event_toys': toy t of the call is toy D = toy_offset + t of the seed's ensemble, keyed by
 * toy_seed(seed, D) -- for T = 1 too; per source N_s ~ Poisson(r_s) with r_s = M_s(z_h) rs_s interpolated over the source's own
 * axes; each event's bin by bisection in the running sums of pmf_s,b = max(tau_s,b(z_h), 0) vol_b (tau_s the source-wise fma
 * chain over the source's own corner rows), its position inside the bin from one uniform per axis; events in drawn order, source
 * by source, positions unclipped (a 'linear' lookup clips only when it scores).  A toy therefore does not depend on T, on the
 * launch geometry, on how truths are grouped into calls (with toy_offset advanced) or on the sub-batches of truths the call works
 * in (parameter sim_truth_chunk), and where no comparison is a near-tie it is event for event the toy bi_simulate_event_toys
 * draws from the expanded grid model.
 *   n_per_toy_source [T][S] (nullable)        the events of every (toy, source); written on success only
 *   bi_sourcewise_simulated_event_count       the events of the resident toys in all, -1 without any
 *   bi_sourcewise_download_events             coords [k][N], source [N] (either nullable): the events without the padding, set by
 *                                             set.  They belong to the simulated store: bi_sourcewise_drop_events and any later
 *                                             store release them, after which the call is BI_ERR_STATE
 * Everything is validated before the previous store is touched (BI_ERR_INVALID: the method, the axes, edges that do not
 * describe B bins, H < 1, a negative n_toys, T < 1 or T >= 2^31, toy numbers beyond 2^48, a truth outside the anchor box, a rate
 * outside [0, 2^30), a store beyond compact_budget); after a device error the context holds no store. */
int bi_sourcewise_simulate_event_toys(bi_ctx* ctx, int method, int k, const int32_t* n_edges, const double* edges, int64_t H,
                                      const double* z, const double* rate_scale, const int64_t* n_toys, uint64_t seed,
                                      double outlier_likelihood, int64_t* n_per_toy_source);
int64_t bi_sourcewise_simulated_event_count(const bi_ctx* ctx);
int bi_sourcewise_download_events(bi_ctx* ctx, double* coords, int32_t* source);

/* ... and its analytic Hessian: bi_eval_sourcewise_hess' contract on the event store.  theta = (z, rs), F = d + S.  The event
 * likelihood is the binned observed form with n = 1 per event, no lgamma and N_s = 1; beside the sums above the kernel
 * (k_sourcewise_events_curv, in the Gram panels of the binned curvature kernel) forms per event chi_s,jk = sum_c d_j d_k w_c p_s,c,e
 * and sums g chi_s,jk and the Gram Q_ab = sum_e ((g u_a) g) u_b over u = (tau_s, ups_s,j) -- no g^2 is formed; nan sources and
 * clamped events (g = 0) as above.  With L_tau_s = sum_e g tau_s - 1, L_ups = sum_e g ups, L_chi = sum_e g chi the host forms
 * H = -C Q C^T plus the (rs_s, z_i), (z_i, z_i) and (z_i, z_k) terms of bi_eval_sourcewise_hess, in long double.
 *   ll [P], grad [P][F], status [P]   bit for bit what bi_eval_factored returns on the store with a gradient
 *   hess [P][F][F]                    full and exactly symmetric (one triangle computed, mirrored); rows and columns of axes nobody
 *                                     owns are 0; nan wherever ll is not finite (outlier = 0 with some lam_e = 0 among them)
 * `dataset` indexes the event sets (an index outside [0, T): BI_ST_BAD_DATASET, ll = -inf, grad and hess nan).  A point's bits do
 * not depend on its batch or on the other sets of the call; repeated calls agree bit for bit.  Needs a finished event store:
 * without one BI_ERR_STATE (the Hessian against counts is bi_eval_sourcewise_hess, which in turn refuses while a store exists). */
int bi_eval_sourcewise_events_hess(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                                   double* grad, double* hess, int32_t* status);

/* ... and the loops over staged points on the event store: the device planner, the ensemble sampler and the gridded likelihood
 * of the binned model (bi_eval_sourcewise_planned, bi_sample_stretch_sourcewise, bi_grid_reduce_sourcewise, which keep refusing
 * while a store exists) under names of their own, signatures equal to theirs.  The planner's event variant writes per point the
 * descriptors bi_eval_factored fills on the host for the store, bit for bit -- rows at the point's set's columns, the set's
 * number of events and tiles, sum_s r_s (sources ascending from 0.0, one rounded addition each) for the finish -- from a device
 * table of the sets uploaded when the store is finished; a rejected point gets zero tiles, so every block of its item returns at
 * entry and the event kernel (k_sourcewise_events, values only) runs the code it ran.  The grid's x is the most blocks any set of
 * the store takes, known on the host: nothing is read and nothing waited for.
 *   bi_eval_sourcewise_events_planned     ll [P] and status [P] (or NULL) bit for bit bi_eval_factored's on the store, values only
 *   bi_sample_stretch_sourcewise_events   bi_sample_stretch_sourcewise's contract and counters [5] with the store's likelihood as the
 *                                         log density: chain, ll and n_accepted are bit for bit those of the same move with one
 *                                         bi_eval_factored call per half-step; counters[4] (synchronisations in the step loop) = 0
 *   bi_grid_reduce_sourcewise_events      bi_grid_reduce_sourcewise's contract and counters [5] on route 0; with one chunk the outputs
 *                                         are bit for bit the reduction of bi_eval_sourcewise_events_planned's values.  route -1
 *                                         takes route 0; route 1 is refused with BI_ERR_INVALID: the matrix-core scan route
 *                                         does not read the event store
 * `dataset` indexes the event sets: an index outside [0, T) is BI_ST_BAD_DATASET in the planned call and BI_ERR_INVALID in the
 * other two, as for the binned calls.  All three need a finished event store: without one (or with an open one) BI_ERR_STATE,
 * naming the binned spelling. */
int bi_eval_sourcewise_events_planned(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                                      double* ll, int32_t* status);
int bi_sample_stretch_sourcewise_events(bi_ctx* ctx, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index,
                                        const double* z0, const double* scale0, const double* unit, const int64_t* dataset,
                                        const double* x0, const double* lo, const double* hi, int64_t n_steps, double a, uint64_t seed,
                                        int64_t first_ensemble, const double* prior_mean, const double* prior_sigma,
                                        const double* prior_const, double* chain, double* ll, int64_t* n_accepted, int64_t* counters);
int bi_grid_reduce_sourcewise_events(bi_ctx* ctx, int64_t E, const int64_t* dataset /*[E] or NULL*/, int F, int n_keep,
                                     const int32_t* var_kind, const int32_t* var_index, const double* z0 /*[E][d]*/,
                                     const double* scale0 /*[E][S]*/, const double* unit /*[E][S]*/, const int32_t* n_nodes /*[F]*/,
                                     const double* nodes, const double* term, const double* logw, int64_t chunk, int route,
                                     double* log_marginal /*[E][K]*/, double* profile /*[E][K]*/, int64_t* argmax /*[E][K]*/,
                                     int64_t* counters /*[5] or NULL*/);

/* The likelihood on a tensor-product grid, reduced over some of its axes on the device: F variables (described as for
 * bi_fit_batched: var_kind / var_index, each parameter at most once), variable j with n_nodes[j] values nodes_j (`nodes`: the F
 * lists one after the other; any order, finite).  The first n_keep variables are kept, the others reduced:
 *   K = prod_{j < n_keep} n_j,  R = prod_{j >= n_keep} n_j,  grid point g = (e K + k) R + r  (variable 0 slowest, the entry e
 *   slowest of all); entry e evaluates dataset[e] (NULL: dataset 0) with its other settings z0[e] [d], scale0[e] [S]; a
 *   shape variable sets z_i = node, a rate variable rate_scale_s = node unit[e][s].
 *   p_g = sum_j term_j[i_j]  (j ascending, from 0.0; `term` laid out as `nodes`: e.g. log priors at the nodes; NULL: none)
 *   q_g = sum_{j >= n_keep} logw_j[i_j]  (log quadrature weights; NULL: none)
 *   t_g = ll_g + p_g,  u_g = t_g + q_g   (binary64, every addition rounded on its own)
 *   profile[e][k] = max_r t_g,  argmax[e][k] = the smallest r that attains it
 *   log_marginal[e][k] = m + log sum_r exp(u_g - m),  m = max_r u_g
 * A point is EXCLUDED from its cell (and counted) when its status word is not 0 (outside the anchor box, unphysical rates, a
 * Beeston-Barlow assertion), when its ll is -inf, or when one of its terms is -inf.  A cell with no point left has -inf, -inf
 * and argmax -1; a ll of nan with status 0 makes both outputs of its cell nan and its argmax -1.  A log weight of -inf takes a
 * point out of the marginal only.
 * The grid is produced, evaluated and reduced in chunks of `chunk` points (0: 2^20) that never leave the device:
 * k_grid_points, the planner and kernels of bi_plan_points_resident / bi_run_plan, k_grid_reduce (an online log-sum-exp
 * and max / argmax per cell, state in HBM; a cell may lie inside one chunk, straddle two or span many).  The host reads the
 * plan's status OR once per chunk and the three output arrays [E][K] once at the end.  No atomics: every sum has a fixed
 * order, so a call is bitwise reproducible for a given chunk; different chunks regroup the sums (agreement to rounding,
 * profile and argmax identical).  counters [4] or NULL: chunks, evaluations, excluded points, evaluation launches.
 * Errors (BI_ERR_INVALID, reason in bi_last_error): F < 1 or > 16, n_keep outside [0, F], a node count < 1, a node that is
 * not finite, +inf or nan in term or logw, E K > 2^24 cells, more than 2^48 points, chunk outside [0, 2^26], a variable that
 * is no parameter of the model or appears twice, and whatever bi_plan_points_resident refuses (as bi_sample_stretch). */
int bi_grid_reduce(bi_ctx* ctx, int64_t E, const int64_t* dataset /*[E] or NULL*/, int F, int n_keep, const int32_t* var_kind,
                   const int32_t* var_index, const double* z0 /*[E][d]*/, const double* scale0 /*[E][S]*/,
                   const double* unit /*[E][S]*/, const int32_t* n_nodes /*[F]*/, const double* nodes, const double* term,
                   const double* logw, int64_t chunk, double* log_marginal /*[E][K]*/, double* profile /*[E][K]*/,
                   int64_t* argmax /*[E][K]*/, int64_t* counters /*[4] or NULL*/);

/* Source-wise models on the matrix-core scan route, and their gridded likelihood.  The per-point kernels of a source-wise model
 * stream a point's NR = sum_s 2^e_s rows once per point; a batch whose points pile up in a handful of cell tuples (one cell per
 * source over the axes it owns) -- a gridded likelihood -- reads the same rows over and over.  The scan route sorts the staged
 * points by (cell tuple, dataset) on the device, chops every group into 16-point work items and hands them to the matrix-core scan
 * kernel of the grid model over the compacted rows of the non-empty-bin form: mu[bin][point] = sum_k row_k[bin] w_k r_s(k), the
 * rows of a group read once per strip of bins; sum_s lambda_s and the lgamma sum are subtracted once per point, as above.
 * Conditions, else BI_ERR_INVALID naming the cause: the non-empty-bin form is built (bi_sourcewise_build_nonempty) and chosen
 * (sourcewise_form = 1); NR <= 32, the scan kernel's row limit; the cell tuples times T fit a 63-bit sort key.
 *   bi_eval_sourcewise_scan       bi_eval_sourcewise_planned's arguments and conventions on that route.  The screen is the same
 *                                 planner kernel: status [P] (or NULL) and the -inf of a rejected point are bit for bit
 *                                 bi_eval_sourcewise_planned's.  A live point's ll agrees with it to rounding, NOT bit for bit,
 *                                 and -- unlike every per-point entry point -- its bits may depend on the batch: which points
 *                                 share a work item, the number of partial sums per item and whether a block of bins takes the
 *                                 product form (counts of 1 and 2: one logarithm of the product of mu^n) follow from the batch.
 *                                 The same call gives the same bits every time (no floating-point atomics outside partial
 *                                 slots that one wave owns, every sum in a fixed order).  A listed bin with mu = 0 or a count
 *                                 that is no integer gives -inf (a nan count cannot reach the store: bi_factored_set_counts refuses it).  One host read per call (the planner's
 *                                 counts).  counters [5] or NULL: [0] groups (cell tuple, dataset; very long groups are cut into
 *                                 several), [1] work items, [2] live points, [3] launches, [4] host reads inside the call.
 *                                 P = 0: BI_OK without device work.  n_scan_launches advances, last_scan_* report the launch.
 *   bi_grid_reduce_sourcewise     bi_grid_reduce's contract, checks, limits and errors (reported under this name) with this
 *                                 model's likelihood: var_index refers to its d axes and S sources, `dataset` to the sets of
 *                                 bi_factored_set_counts or of the toy generator.  Per chunk the staged points are evaluated by
 *                                 route 0: the planner and per-point kernels of bi_eval_sourcewise_planned (on the dense store or
 *                                 the non-empty-bin form, whichever the context evaluates on); route 1: the scan route above;
 *                                 route -1: 1 where the conditions hold, else 0.  The reduction reads the planner's status words;
 *                                 nothing is read by the host per chunk on route 0, the planner's counts on route 1.  With route
 *                                 0 and one chunk the outputs are bit for bit the reduction of bi_eval_sourcewise_planned's
 *                                 values.  counters [5] or NULL: chunks, evaluations, excluded points, launches, the route taken. */
int bi_eval_sourcewise_scan(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll,
                            int32_t* status, int64_t* counters /*[5] or NULL*/);
int bi_grid_reduce_sourcewise(bi_ctx* ctx, int64_t E, const int64_t* dataset /*[E] or NULL*/, int F, int n_keep,
                              const int32_t* var_kind, const int32_t* var_index, const double* z0 /*[E][d]*/,
                              const double* scale0 /*[E][S]*/, const double* unit /*[E][S]*/, const int32_t* n_nodes /*[F]*/,
                              const double* nodes, const double* term, const double* logw, int64_t chunk, int route,
                              double* log_marginal /*[E][K]*/, double* profile /*[E][K]*/, int64_t* argmax /*[E][K]*/,
                              int64_t* counters /*[5] or NULL*/);

/* One parameter point against datasets [t0, t1): the toy-MC form.  mu_b / log mu_b are computed
 * once and every dataset reduces sum_b xlogy(n, mu) against them.  Not available with
 * Beeston-Barlow (mu then depends on the data).  out [t1 - t0]. */
int bi_eval_datasets(bi_ctx* ctx, const double* z, const double* rate_scale, int64_t t0, int64_t t1,
                     double* out, int32_t* status /*[1] or NULL*/);
/* the same with the results left in HBM (out_dev: t1 - t0 doubles of device memory, e.g. the send buffer of the
 * gather that ends a toy-MC run sharded over GPUs); returns when the kernels have finished */
int bi_eval_datasets_device(bi_ctx* ctx, const double* z, const double* rate_scale, int64_t t0, int64_t t1,
                            double* out_dev, int32_t* status /*[1] or NULL*/);

/* The toy-MC form over SEVERAL parameter points: P hypotheses against datasets [t0, t1) in one call -- what the reference's
 * toy-MC users run as a double loop, every simulated dataset (blueice/model.py:69-91 + set_data) evaluated at every hypothesis
 * (the loops of blueice/inference.py:392-443), P x T likelihood calls.  Here the points are ordered by grid cell and taken four
 * at a time: the points of a pass that share a grid cell share one pass over its 2^d S template rows (hypotheses that differ
 * in their rates only always do), and ONE pass over the datasets' non-empty-bin lists serves all four -- their log mu tiles sit
 * side by side in LDS.  Same values as P calls of bi_eval_datasets to rounding (the partial sums are grouped by tiles of 4096
 * instead of 8192 bins); every result is a sum in a fixed order, so a call is bitwise reproducible.
 *   z [P][d], rate_scale [P][S] or NULL; out [P][t1 - t0], row p = point p; status [P] or NULL: a point outside the anchor box
 *   or with unphysical rates has BI_ST_OUT_OF_BOUNDS / BI_ST_UNPHYSICAL and a row of -inf (likelihood.py:345-347, 397-415).
 * Data that the multi-point kernels do not cover (dense counts only, fewer than 64 datasets, counts that fit no list format)
 * are answered point by point through bi_eval_datasets; not available with Beeston-Barlow.  P <= 65535.
 * _device: out_dev [P][t1 - t0] in HBM (the send buffer of a gather when the hypotheses are dealt over GPUs). */
int bi_eval_datasets_points(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int64_t t0, int64_t t1,
                            double* out, int32_t* status /*[P] or NULL*/);
int bi_eval_datasets_points_device(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, int64_t t0, int64_t t1,
                                   double* out_dev, int32_t* status /*[P] or NULL*/);

/* ---- compatibility mode: materialise what the morpher closures return ---------------------
 * `ps_interpolator(zs)` / `mus_interpolator(zs)` / `n_model_events_interpolator(zs)`
 * (pdf_morphers.py:70) and `full_output=True` (likelihood.py:424-425).
 *   which: 0 = ps [S][B], 1 = mus [S], 2 = n_model row [B]
 * returns BI_ERR_INVALID for out-of-bounds z (scipy raises ValueError, bounds_error=True). */
int bi_interpolate(bi_ctx* ctx, int which, const double* z, double* out);
/* adjusted (mus [S], ps [S][B]) after rate scaling and Beeston-Barlow, as full_output returns */
int bi_eval_full(bi_ctx* ctx, const double* z, const double* rate_scale, int64_t dataset, double* ll,
                 double* mus_out, double* ps_out, int32_t* status);

/* ---- asynchronous / device-resident form (inputs already in HBM, no host round trip) -------
 * bi_plan_points does the host-side part of bi_eval once (cell lookup, rates, grouping) and
 * keeps the plan on the device; bi_run_plan launches the kernels on the context stream and
 * writes to a DEVICE buffer of P doubles (e.g. a torch / RCCL tensor's data pointer);
 * bi_sync waits for the stream. */
typedef struct bi_plan bi_plan;
int bi_plan_points(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                   bi_plan** out);
int bi_run_plan(bi_ctx* ctx, bi_plan* plan, double* out_dev /* NULL: internal buffer */);
/* A scan dealt over several GPUs ("sort/group by grid cell first, then deal cells to ranks"; the
 * reference's counterpart is the double loop of blueice/inference.py:424-432).  Every rank passes the SAME P points; the
 * device planner's (cell, dataset) sort IS the dealing: rank `share_rank` of `share_world` takes a contiguous, balanced
 * range [lo, hi) of the sorted list of valid points, so the points of a grid cell stay together (a cell is split over at
 * most two neighbouring ranks) and no host pass over the points is needed.  bi_run_plan then writes hi - lo results in
 * SORTED order to out_dev[0 .. hi - lo); after the ranks' vectors have been gathered into [share_world][stride]
 * (stride >= ceil(n_valid / share_world)), bi_plan_unsort scatters them into the caller's point order, full_dev [P]
 * (rejected points: -inf), on the context's stream.  Beeston-Barlow models too (blueice/likelihood.py:618-660: work items of
 * bb_max_group points, N(z) from the per-anchor totals), unless some point of the batch can have a bin with U_b == 0 -- there
 * the reference's first-root assertion hangs on the last bits of N, which only the host planner's pass in numpy's summation
 * order reproduces: BI_ERR_INVALID then, as for infinite rate scales (the caller deals such a scan on the host). */
int bi_plan_points_share(bi_ctx* ctx, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                         int share_rank, int share_world, bi_plan** out);
int bi_plan_share_info(const bi_plan* plan, int64_t* n_valid, int64_t* lo, int64_t* hi);
/* The same with the points ALREADY IN HBM: z_dev [P][d], rate_scale_dev [P][S] or NULL, dataset_dev [P] or NULL are device
 * arrays on the context's GPU (bi_device_alloc + bi_memcpy_to_device, or any producer that has finished writing them) and are
 * read where they lie -- no host pass, no copy; they may be freed or overwritten as soon as the call returns.
 * share_world = 1: the whole batch (bi_plan_points); > 1: this rank's share of a dealt scan (bi_plan_points_share).
 * Always planned on the device, so the restrictions of the device planner apply as errors instead of a silent host path:
 * no point with an infinite rate of a source that may go negative (likelihood.py:403-415: those are answered on the host),
 * no Beeston-Barlow point that needs exact totals (see bi_plan_points_share), P <= 2^30; BI_ERR_INVALID as well for a
 * pointer that is not device memory of this GPU.
 * The batched callers of the reference hold their points in numpy arrays (inference.py:424-432), so this entry has no
 * counterpart there: it is for drivers that produce hypotheses on the device or reuse one grid for many datasets. */
int bi_plan_points_resident(bi_ctx* ctx, int64_t P, const double* z_dev, const double* rate_scale_dev,
                            const int64_t* dataset_dev, int share_rank, int share_world, bi_plan** out);
int bi_plan_unsort(bi_ctx* ctx, bi_plan* plan, const double* gathered_dev, int64_t stride, double* full_dev);
int bi_plan_read(bi_ctx* ctx, bi_plan* plan, double* out /*[P]*/, int32_t* status /*[P] or NULL*/);
/* The bitwise OR of the plan's per-point status words after the last bi_run_plan (waits for the stream): what a caller
 * that leaves the results in HBM (bi_run_plan(out_dev) -> collective) must look at before it trusts them.
 * BI_ST_INTERNAL in it means a launch gave up collecting a partial sum (result nan): the context's mailbox is
 * emptied again here, so the next launch starts clean. */
int bi_plan_status(bi_ctx* ctx, bi_plan* plan, int32_t* status_or);
int64_t bi_plan_bytes(const bi_plan* plan);    /* algorithmic HBM bytes one bi_run_plan moves */
int64_t bi_plan_launches(const bi_plan* plan); /* morph+reduce launches per bi_run_plan */
void bi_plan_destroy(bi_ctx* ctx, bi_plan* plan);
int bi_sync(bi_ctx* ctx);
void* bi_stream(bi_ctx* ctx); /* the hipStream_t the context launches on */

/* Plain device buffers on the context's GPU, for callers that keep results in HBM between bi_run_plan and a
 * collective (the per-rank result vectors that RCCL gathers over xGMI at the end of a sharded scan: SURVEY.md
 * section 8e; the reference has no counterpart, its scans are Python loops, blueice/inference.py:424-432).
 * The copies run on the context stream and return when the data has arrived. */
int bi_device_alloc(bi_ctx* ctx, int64_t bytes, void** out);
int bi_device_free(bi_ctx* ctx, void* p);
int bi_memcpy_to_host(bi_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);
int bi_memcpy_to_device(bi_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);

/* self-test of the device logarithm used in the per-bin terms: out[i] = log(x[i]) as the kernels compute it */
int bi_selftest_log(bi_ctx* ctx, int64_t n, const double* x, double* out);

/* debug / tests: the packed shadow of the template rows (parameter packed_rows) expanded back to doubles on the device,
 * out_dev [anchors x sources][padded_bins]; BI_ERR_STATE when the resident model has none (packed_rows_valid = 0) */
int bi_unpack_rows(bi_ctx* ctx, double* out_dev);

/* self-tests of the library's own device-wide primitives (csrc/tu_prim.hip: the stable radix sort of (64-bit key, value) pairs over
 * the key bits [begin_bit, end_bit) and the scans behind the device planner, the list builders and toy generation), on caller data:
 *   sort kind 0: uint64 keys, int64 values | 1: int64 keys, int32 values | 2: double keys (numpy's sort order, -nan < -inf ... +inf < +nan), int32 values
 *   scan kind 0: inclusive running maximum of int64 | 1: inclusive sum of int64 | 2: inclusive sum of double | 3: exclusive sum of int64, from `init` */
int bi_selftest_sort(bi_ctx* ctx, int kind, int64_t n, const void* keys, const void* vals, int begin_bit, int end_bit, void* keys_out,
                     void* vals_out);
int bi_selftest_scan(bi_ctx* ctx, int kind, int64_t n, const void* in, int64_t init, void* out);
/* self-test of the reduction kernels of bi_grid_reduce on caller data: t [cells][R] stands for ll + p (-inf: an excluded
 * point, nan: a nan), q [cells][R] or NULL for the log weights; the values are folded in chunks of `chunk` (0: all at once)
 * exactly as a grid's result vectors are -> log_marginal, profile, argmax [cells] */
int bi_selftest_grid_reduce(bi_ctx* ctx, int64_t cells, int64_t R, int64_t chunk, const double* t, const double* q,
                            double* log_marginal, double* profile, int64_t* argmax);

/* ---- measurement ---------------------------------------------------------------------------
 * While enabled, every morph+reduce launch is bracketed by HIP events on the context stream;
 * bi_profile_read drains them: number of launches and summed GPU time in milliseconds.
 * bi_measure_read_bandwidth: the read-only streaming ceiling of the device (SURVEY.md 8d asks for it beside the
 * 8 TB/s vendor figure) -- a plain 16-byte-load sum over the resident template tensor, best of `reps` passes,
 * in GB/s; `nontemporal` selects the load hint, `blocks_per_cu` the grid.
 * bi_measure_copy_bandwidth: the device-to-device copy rate (bytes read + bytes written per second, GB/s) of the runtime's
 * own copy over the first `bytes` of the template tensor into a scratch buffer -- the other usual ceiling. */
int bi_measure_read_bandwidth(bi_ctx* ctx, int nontemporal, int blocks_per_cu, int reps, double* gb_per_s);
int bi_measure_copy_bandwidth(bi_ctx* ctx, int64_t bytes, int reps, double* gb_per_s);
/* the same read-only ceiling with the morph kernel's own access pattern: `items` work items that each stream `rows`
 * template rows concurrently (16 bytes per lane per row, XCD-aware tile order, the grid a batched launch would get)
 * and do nothing with them -- what k_morph_reduce's GB/s is to be held against; best of `reps` passes */
int bi_measure_stream_bandwidth(bi_ctx* ctx, int items, int rows, int nontemporal, int blocks_per_cu, int reps, double* gb_per_s);
int bi_profile_enable(bi_ctx* ctx, int on);
int bi_profile_read(bi_ctx* ctx, int64_t* n_launches, double* total_ms);
/* Tunables (bi_set_param; all have measured defaults) and read-only counters (bi_get_param):
 *   sparse            0 every bin visited | 1 non-empty-bin form when exact (templates >= 0, default) | 2 force
 *   max_group         points per cell pass: 1, 2, 4, 8, 16 (default 16)
 *   blocks_per_cu     resident blocks per CU the launch shapes aim for (8)
 *   nt_loads          0 never | 1 always | 2 nontemporal template loads when no two items share an anchor (default)
 *   tile_chunks       XCD-aware tile order: contiguous regions per row (8; 1 = plain order)
 *   single_kernel, fuse_max_blocks   one-launch path of single evaluations, in-launch finish up to this many blocks
 *   single_blocks_per_cu   single evaluations: blocks per CU the launch shape aims for, equal tiles per block (4)
 *   fuse_finish       batched launches of up to 256 work items whose partial sums fit the context's mailbox (2^20 slots):
 *                     the last block of an item collects the item's partials inside the launch, no finish launch follows (1)
 *   keep_rows         single dense evaluations repeated in one cell: stream rows that keep the default cache policy so
 *                     they stay in the Infinity Cache between calls (-1 = as many as fit, default; 0 = none)
 *   poll_result       single evaluations: poll the pinned result word instead of a stream synchronise (1)
 *   xcd_affine        round block counts to multiples of 8
 *   device_plan_min   batches of at least this many points are planned on the device (512)
 *   scan_mfma, scan_min_items, scan_cb, scan_waves_per_cu   the matrix-core scan kernel: on/off, items per cell from
 *                     which it is used (4; x2 for dense data), strip width (0 = by the data), waves per CU the
 *                     strips of all cells are spread over (0 = sized by the kernel's occupancy so that the blocks run in
 *                     full rounds, default)
 *   grad_mfma, grad_mfma_min, grad_slices   bi_eval_grad: batches of >= grad_mfma_min (2048) points of one dataset (plain binned likelihood, up to 32
 *                     streams) run on the fp64 matrix cores -- points grouped by grid cell, mu = rows x coefficients and
 *                     G = (n / mu) x rows^T as two chained matrix products per 16-bin block, the derivative coefficients
 *                     contracted per point afterwards (k_grad_mfma; 1, default; 0 = one work item per point); grad_slices:
 *                     slices a cell's 16-bin blocks are split into (0 = by the batch).  Read-only n_grad_mfma_launches
 *   host_threads      host threads the planner may start per call (PROCESS-wide): 0 = what the process may run on (its
 *                     scheduling affinity), at most 16 (default); a launcher of N ranks per node sets its share, so that the ranks
 *                     together never run more planner threads than the node has cores for them
 *   scan_xcd          k_scan_sorted (rows in count order): how the (cell, block) pairs of a launch are dealt to the 8 XCDs, whose
 *                     L2s each keep the coefficient lists of the cells they work on: 1 contiguous, equal ranges of the cell-major
 *                     list (default), 2 cell g on XCD g mod 8, 0 plain launch order (every cell on every XCD)
 *   bb_exact          single-point Beeston-Barlow evaluations: N(z) = sum_b n_model[i, b] in numpy's own summation order (one more
 *                     pass over the 2^d rows of MC counts), so that the root formula sees the reference's bits: 0 never, 1
 *                     always, 2 when some bin can have U_b == 0 at the point (default)
 *   toy_events        bi_generate_toys: sparse expectations (sum mu < B/8, templates and rates >= 0) are drawn event by event --
 *                     N ~ Poisson(sum mu), bins by bisection in the cumulative sums, sorted and run-length encoded per toy (1,
 *                     default); 0 = always one Poisson draw per bin.  Read-only `last_toy_method`: 1 / 0 for the last call.
 *   dot_tiled         bi_eval_datasets over non-empty-bin lists: batches of >= 64 datasets take the kernel that stages bin tiles
 *                     of log mu in LDS over tile-major lists (1, default); 0 = always one block per dataset
 *   dot_lanes         ... lanes per (dataset, tile) run of that kernel: 0 = the best measured for the lists' entry width (default: 8
 *                     lanes x three 16-byte loads = 96 entry slots with four-byte entries, 4 lanes x three loads = 96 slots with
 *                     two-byte ones), or 4 / 8 / 16 (16: 128 slots, round 3's shape)
 *   dot_entry16       ... the tile-major lists hold TWO-byte entries (bin within the tile, count) where every count of every dataset is
 *                     at most 7 -- the kernel is bound by reading the lists --, four-byte entries otherwise (1, default; 0 = always
 *                     four bytes; read-only `tm_entry_bytes`: the width of the lists as built, 0 = none: not built yet, or the last
 *                     build met a count outside 1 ... 32767, which fits neither width).  With two-byte entries dot_lanes
 *                     8 and 16 mean 128 entry slots per run (8 lanes, two loads each), 4 means 96 (three loads per lane)
 *   dot_blocks_per_cu ... blocks of that kernel per CU its split of the datasets aims at: 0 = as many as are resident at once (one
 *                     round of blocks; default), n = n per CU
 *   score_sorted      bi_score_events / bi_simulate_events (set on the TARGET context): from 4096 events on, the events are ordered
 *                     by histogram cell before their densities are gathered, so the gathers stream through the histograms; the
 *                     tensor's columns are then in that order, which only sums over events can see -- bi_interpolate and
 *                     bi_eval_full return per-event values in the caller's order (1, default; read-only `events_sorted`)
 *   toy_points_pp     bi_eval_datasets_points: parameter points per pass over the datasets' lists: 0 = by the batch (4; 2 for a
 *                     call of two points), 2, 4, or 1 = point by point through bi_eval_datasets.  toy_points_lanes: lanes per
 *                     (dataset, tile) run of its kernel, 0 = the measured default, or 2 / 4 / 8.  Read-only n_toy_points_passes
 *                     (passes made so far) and tmm_entry_bytes (entry width of the 4096-bin tile lists as built, 0 = none)
 *   toy_fast_call     bi_eval_datasets, bits: 1 = the point's descriptors travel in the kernel arguments (no copy ahead of the launch),
 *                     2 = the tiled kernel's partial sums are finished 64 datasets per block, tiles split over its four waves,
 *                     4 = results of up to 4 MB: the call polls a completion word behind them instead of synchronising the
 *                     stream (needs 2 and poll_result; every 256th call synchronises anyway).  7 (default)
 *   scan_share_slow   k_scan_sorted: a strip whose 64 bins do not carry one count (two runs meet, the end of the data) is worked item by
 *                     item, ~25 times the cost of a uniform strip; with 1 (default) the items of such strips are dealt over ALL waves
 *                     of the cell instead of staying with the wave that owns the strip
 *   scan_bb, scan_bb_min   Beeston-Barlow batches planned on the device (no bin can have U_b == 0, at least scan_bb_min = 64
 *                     points) run on the fp64 matrix cores: four 16-point work items of a grid cell share the rows of a bin
 *                     tile through LDS, U, P and a are three chains of matrix products, the per-bin roots and Poisson terms follow
 *                     on the vector ALU in the reference's operation order (k_scan_bb; 1, default; 0 = k_morph_reduce<bb_max_group,
 *                     true> as for small batches).  Read-only n_bb_scan_launches
 *   plan_tables       device planner: where the (cell, dataset) keys are few (anchors x datasets < 65 536) the group structure of the
 *                     sorted points comes from tables over the KEYS (one small kernel) instead of three scans over the points (1, default)
 *   toy_points_overlap   bi_eval_datasets_points over more than 8 points: the log mu pass of the next group of passes and the finish
 *                     of the last one on a second, low-priority stream beside the dot kernel (1); measured: the kernels run side
 *                     by side but slow each other by as much -- no gain, hence off (0, default).  The same bits either way
 *   plan_count_sort   device planner: keys of at most 1024 values (a profile scan: one dataset, up to 1023 grid cells) are ordered by
 *                     a one-pass counting sort instead of the radix sort's pass per 4 bits; the same stable order (1, default)
 *   scan_chunk        matrix-core scans over few grid cells with long lists of work items (a rank's share of a dealt scan): the
 *                     item lists are cut into chunks, each worked as a group of its own, so that the chip is filled (1, default)
 *   scan_sparse_max_items   non-empty-bin form: items per grid cell up to which the matrix-core scan kernel takes the compacted rows
 *   scan_split        scans with sparse = 0 over mostly empty data: non-empty-bin pass + validity pass of every bin on the
 *                     matrix cores (k_scan_valid) instead of the per-bin terms in every bin (1)
 *   compact_budget    bytes of device memory the compacted templates of the non-empty-bin form may take
 *                     (also the bound of bi_sourcewise_build_nonempty's copies)
 *   sourcewise_form   source-wise models: 1 (default) = bi_eval_factored, bi_fit_batched_factored, bi_eval_sourcewise_planned and
 *                     bi_sample_stretch_sourcewise run on the non-empty-bin form where bi_sourcewise_build_nonempty has built
 *                     it; 0 = they read the dense store although it is built.  Read-only sourcewise_nonempty_ready (1 while the
 *                     form is built) and sourcewise_nonempty_bytes (the bytes of its compacted copies, 0 when it is not)
 *   sourcewise_scan_timed   while profiling (bi_profile_enable), which parts of the source-wise scan route are between events:
 *                     bit 0 = the planner (screen, key, sort, structure, the host read of the counts, fill), bit 1 = the
 *                     matrix-core launches (3: both); bi_profile_read sums what was timed
 *   toy_offset        bi_generate_toys: toy t of a call is dataset toy_offset + t of the seed's random stream, so ranks
 *                     that each generate a range of one toy-MC ensemble draw the same toys as one process would (0)
 *   sim_truth_chunk   bi_sourcewise_simulate_event_toys: truths per sub-batch of the pmf rows, their running sums and the event
 *                     kernel; 0 (default) = as many as 256 MiB of scratch hold at 16 S B bytes per truth.  The toys do not
 *                     depend on it: it places the seam between sub-batches (tests).  Read-only sim_ns_layout, sim_ns_pmf,
 *                     sim_ns_events, sim_ns_score: while profiling (bi_profile_enable), the device time in ns of the last call's
 *                     counts + layout, pmf rows + running sums, event kernel and scoring; 0 otherwise
 *   scan_pow          scans over dense data on the matrix cores run on a copy of the template rows whose bins are ordered by
 *                     their count (one dataset, within compact_budget; built on first use per data upload): a lane's bins then
 *                     carry one count n, and sum n log mu over them is n log of their product -- one logarithm per lane, work
 *                     item and 32-bin strip instead of eight (1, default; 0 = rows in bin order, a logarithm per bin).
 *                     Read-only n_sorted_scans counts the scans that ran on the copy
 *   mail_timeout_ms   in-launch finish: how long an item's collecting block waits for a sibling's partial sum before it gives
 *                     up with BI_ST_INTERNAL (2000)
 *   narrow_counts     dense evaluations (sparse = 0, Beeston-Barlow, sources that may go negative) stream the counts of a dataset
 *                     as ONE byte per bin instead of eight where that is exact: every upload of dense counts also builds a
 *                     [T][padded bins] byte copy on the device (one more byte per bin and dataset; skipped, not an error, if it
 *                     cannot be allocated), and a dataset all of whose values are whole numbers 0 ... 255 (not -0.0, nan, inf)
 *                     is read from it by the morph kernels -- a launch only if EVERY dataset its work items refer to is
 *                     such a dataset; every result bit is the same (1, default; 0 = always the doubles).  Read-only:
 *                     narrow_ready (the copy exists for the resident data), n_narrow_launches (launches that read it),
 *                     last_streamed_bytes (bytes the last bi_run_plan streamed: bi_plan_bytes -- the algorithmic bytes of the
 *                     all-double formulation -- less 7 x padded bins for every work item read narrow)
 *   packed_rows       the dense value kernels (k_morph_reduce / k_morph_single without Beeston-Barlow: single points, batches,
 *                     plans) stream the template rows as 7 bytes per value instead of 8 where that is exact: the end of a model
 *                     upload builds a packed shadow of the tensor on the device -- per 512-bin tile of a row the 52 mantissa
 *                     bits of every value, a 4-bit exponent code, and one exponent base -- if it takes at most a quarter of the
 *                     free device memory and can be allocated (else no shadow, not an error).  A model has one iff in every
 *                     tile of every row each value is +0.0 or a positive normal double and the exponents of the non-zero ones
 *                     span at most 15 values (no -0.0, negative value, subnormal, inf or nan); decoding returns the stored
 *                     doubles, so every result bit is the same (1, default; 0 = never build or read it; read at upload and at
 *                     every launch).  Read-only: packed_rows_valid (the resident model has a shadow), n_packed_launches
 *                     (launches that read it), last_packed_saved_bytes (bytes the last bi_run_plan did not stream thanks to it:
 *                     padded bins x rows x work items; last_streamed_bytes does not include this saving)
 *   single_timing_reset   (write) zero the single-call wall-time accumulators below
 *   bb_max_group      points per work item of a Beeston-Barlow batch (the points of a grid cell share a pass over the streams):
 *                     1, 2, 4, 8 (default) or 16 -- sixteen keep their accumulators partly in AGPRs, one wave per SIMD
 *   drop_recycle_cache   (write) give the device buffers the context keeps for reuse (plan and scratch buffers of up to
 *                     1 GiB each, 4 GiB in total; read-only recycle_cache_bytes) back to the driver now; an allocation that
 *                     fails does the same before it gives up
 *   debug_skip_post, debug_late_post   (write; fault injection for tests) block k of the NEXT launch that finishes through the
 *                     mailbox never posts its partial sum / posts it after the collector has given up; consumed by that launch
 * read-only: n_set_launches (evaluation launches of k_morph_sets: work items with different event sets, see bi_score_event_sets),
 *            n_sampler_half_steps (half-steps of bi_sample_stretch so far), last_plan_refused (the last bi_plan_points_resident /
 *            bi_sample_stretch planning refused its batch: 1 Beeston-Barlow points that need exact totals, 2 infinite rates of sources that may
 *            go negative; 0 otherwise -- how a caller tells the refusals that the host path answers from other BI_ERR_INVALID), tile_bins, padded_bins, n_scan_launches, n_toy_polled (bi_eval_datasets calls that returned on the completion word), tm_entry_bytes, events_sorted, n_valid_launches, n_sorted_scans, n_bb_exact, n_mail_resets, user_allocations, csr_ready, compact_ready, compact_sorted (the compacted copy is ordered by count), split_ready, ps_nonneg, nnz_total, dense_counts (the resident datasets are held as dense rows; 0: as non-empty-bin lists only, device-generated toys), coarse_cells (cells of the coarse binning set by bi_set_coarse_binning, 0: none);
 *            last_morph_nbx / last_morph_items / last_morph_fused (the most recent k_morph_reduce or k_morph_single launch: blocks per
 *            work item, work items of the launch, and 1 if it finished through the mailbox, 0 if a finish kernel ran behind it;
 *            the host route of bi_eval_grad sets them for its kernels, and every source-wise evaluation that adds up per-item
 *            sums -- bi_eval_factored, bi_eval_sourcewise_gof, bi_eval_sourcewise_real, bi_eval_sourcewise_hess and
 *            bi_eval_sourcewise_fisher, the last two once per Gram panel -- for the grid of its most recent launch, fused = 0:
 *            the blocks per item there depend on the rows' length alone);
 *            last_point_pieces (the device pieces that the most recent per-point entry point cut its live items into on the host:
 *            launches of at most 65 535 or 32 768 items, within sub-batches of about 2^23 doubles in flight -- summed over the
 *            sub-batches and Gram panels of a source-wise call.  Set by every source-wise evaluation and by the calls that write
 *            bins or cells -- bi_expected_counts, bi_expected_coarse, bi_expected_coarse_jacobian, bi_coarse_counts,
 *            bi_set_asimov_counts and their bi_sourcewise_ forms, where bi_sourcewise_generate_toys counts the launches over its
 *            truths --, 0 after such a call with no live item; the grid model's item-kernel evaluations (the host route of
 *            bi_eval_grad, bi_eval_hess, bi_eval_fisher, bi_eval_gof, bi_eval_real) set it when they launch);
 *            last_scan_nslots / last_valid_nslots / last_scan_resident (waves per cell the planner chose for the scan kernels of
 *            the last plan, and the resident blocks per CU it sized them by), last_toy_method (1 = event by event);
 *            last_scan_groups / last_scan_max_items (groups of work items of the last scan LAUNCH and the items of the longest
 *            one, after long item lists were cut into groups of their own: scan_chunk; the validity pass of a split scan sets
 *            these two as well), last_scan_cb (strip width of the last matrix-core scan launch in 16-bin blocks: 2 or 4),
 *            last_scan_by_count (1: the kernel for rows in count order took it), last_scan_prod (1: the product form for compacted
 *            rows in bin order did) -- all five are set when a plan runs, so a plan run again describes itself, whereas
 *            last_scan_nslots / last_valid_nslots / last_scan_resident are set when a plan is made;
 *   single_calls, single_ns_host, single_ns_launch, single_ns_wait   wall time (ns, summed over single_calls calls) of
 *                     bi_eval(P = 1): host half (geometry, rates, descriptors), launch calls, wait for the result */
int bi_set_param(bi_ctx* ctx, const char* name, int64_t value);   /* unknown or read-only name: BI_ERR_INVALID */
int64_t bi_get_param(bi_ctx* ctx, const char* name);               /* unknown or write-only name: INT64_MIN (no parameter
                                                                      can hold it) and a message in bi_last_error */
/* every parameter name, one per line as "<name> <rw|r|w>\n", NUL-terminated, into buf (truncated to len); returns
 * the buffer size the whole list needs */
int bi_list_params(char* buf, int len);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BLUEICE_HIP_H */
