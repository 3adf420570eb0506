// libblueice_hip: MI355X (gfx950 / CDNA4) binned-likelihood hot path behind a C ABI.
//
// What runs here, per evaluation (reference: JelleAalbers/blueice v1.2.1):
//   a3  GridInterpolator multilinear morph over the anchor tensor   blueice/pdf_morphers.py:57-70
//   a4  rate scaling + early exits                                    blueice/likelihood.py:345-415
//   a6  Beeston-Barlow single-source adjustment                       blueice/likelihood.py:618-660,693-712
//   a5  sum_bins poisson.logpmf(n | sum_s r_s p_s)                    blueice/likelihood.py:662-675
//
// Design: the anchor tensor lives in HBM as rows [anchor][source][Bp] (bin
// fastest, rows padded to a multiple of the 512-bin block tile, so every lane issues aligned
// 16-byte loads with no bounds checks).  One kernel streams the 2^d * S corner rows of a grid
// cell once, and for up to G parameter points that fall in that cell keeps
//     mu[g][bin] = sum_{corner,source} (w_corner[g] * r_source[g]) * row[corner,source][bin]
// in registers (the per-point coefficients are wave-uniform and arrive through scalar loads),
// applies the Poisson term, and reduces wave -> block -> partial.  A small second kernel sums
// the per-block partials in a fixed order (bitwise reproducible; no float atomics) and
// subtracts the per-dataset sum of lgamma(n+1), which depends on the data only and is computed
// once at upload.  The path is HBM-bandwidth bound: 8*(2^d*S + 1) bytes per bin per cell pass.
//
// No CPU fallback exists: without a HIP device bi_create fails.

#include "bi_common.h"
#include "bi_prim.h"
#include "bi_k_misc.h"
#include "bi_geometry.h"
#include "bi_launch.h"
#include "bi_items.h"
#include "bi_sparse.h"
#include "bi_single.h"
#include "bi_planning.h"
#include "bi_planning_device.h"
#include "bi_grad_mfma.h"
#include "bi_grad.h"
#include "bi_params.h"
#include "bi_events.h"
#include "bi_toys.h"

namespace {

// dense counts [T][Bp] are resident: per-dataset sum lgamma(n+1), then the sparse forms
int finish_counts(bi_ctx* c, int64_t T) {
    int rc;
    // sum_b lgamma(n+1) per dataset, on the device
    const int nblk = (int)std::min<int64_t>(256, (c->B + kThreads - 1) / kThreads);
    if ((rc = dev_alloc(c, c->lgsum, (size_t)T * sizeof(double)))) return rc;
    const int64_t chunk = 32768;  // datasets per launch (gridDim.y limit)
    if ((rc = dev_alloc(c, c->scratch, (size_t)std::min(T, chunk) * nblk * sizeof(double)))) return rc;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t n = std::min(chunk, T - t0);
        hipLaunchKernelGGL(k_counts_lgamma, dim3(nblk, (unsigned)n), dim3(kThreads), 0, c->stream,
                           (const double*)c->counts.p + t0 * c->Bp, c->B, c->Bp, (double*)c->scratch.p, nblk);
        hipLaunchKernelGGL(k_rows_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)c->scratch.p, nblk, (double*)c->lgsum.p + t0, n);
    }
    HIP_TRY(c, hipGetLastError());
    build_narrow_counts(c, T);      // (its flags reach the host with the synchronisation below)
    c->h_lgsum.assign((size_t)T, 0.0);
    HIP_TRY(c, hipMemcpyAsync(c->h_lgsum.data(), c->lgsum.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->T = T;
    c->dense_counts = true;
    if ((rc = build_sparse_forms(c))) return rc;
    c->data_ready = true;
    return BI_OK;
}

}  // namespace

extern "C" {

const char* bi_version(void) { return BI_VERSION; }

const char* bi_last_error(const bi_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int bi_create(int device, bi_ctx** out) {
    if (!out) return fail(nullptr, BI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, BI_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, BI_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    bi_ctx* c = new bi_ctx();
    c->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&c->prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        fail(nullptr, BI_ERR_HIP, "device init failed: %s", hipGetErrorString(e));
        delete c;
        return BI_ERR_HIP;
    }
    *out = c;
    return BI_OK;
}

void bi_destroy(bi_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    dev_free(c->ps); dev_free(c->nm); dev_free(c->nm_tot); dev_free(c->counts); dev_free(c->lgsum); dev_free(c->cnt8); dev_free(c->cnt8_bad);
    dev_free(c->pk); dev_free(c->pk_base); dev_free(c->pk_bad);
    dev_free(c->scratch); dev_free(c->scratch2); dev_free(c->logmu); dev_free(c->toy_blocks_done); dev_free(c->ev_perm);
    dev_free(c->slot_dev); dev_free(c->slot_partial); dev_free(c->slot_pflags); dev_free(c->slot_counter); dev_free(c->space_edges);
    dev_free(c->mail); dev_free(c->mail_flags);
    dev_free(c->ps_sorted); dev_free(c->cnt_sorted);
    dev_free(c->sim_coords); dev_free(c->sim_source);
    dev_free(c->real_counts);
    dev_free(c->fac.ps); dev_free(c->fac.counts); dev_free(c->fac.real_counts); dev_free(c->fac.geom); dev_free(c->fac.lgsum_dev);
    dev_free(c->fac.ne_ps); dev_free(c->fac.ne_cnt); dev_free(c->fac.ne_tab);
    dev_free(c->fac.ev_ps); dev_free(c->fac.ev_tab);
    release_coarse(c);
    release_coarse(c->sw_coarse);
    if (c->slot_host) (void)hipHostFree(c->slot_host);
    if (c->pack_host) (void)hipHostFree(c->pack_host);
    if (c->bounce_host) (void)hipHostFree(c->bounce_host);
    if (c->plan_host) (void)hipHostFree(c->plan_host);
    dev_free(c->pack_dev);
    dev_free(c->nz_idx); dev_free(c->nz_n); dev_free(c->nz_off); dev_free(c->ps_c); dev_free(c->cnt_c); dev_free(c->tm_entries); dev_free(c->tm_off); dev_free(c->tmm_entries); dev_free(c->tmm_off);
    dev_free(c->pt_grid); dev_free(c->pt_mus); dev_free(c->pt_coff); dev_free(c->pt_allow); dev_free(c->pt_c_off);
    dev_free(c->pt_cnt_off); dev_free(c->pt_c_np); dev_free(c->pt_Tz); dev_free(c->pt_rowsum); dev_free(c->pt_rowmin); dev_free(c->pt_nm_tot);
    for (void* q : c->user_allocs) (void)hipFree(q);   // bi_device_alloc buffers nobody freed
    c->user_allocs.clear();
    for (auto& q : c->cache) (void)hipFree(q.p);  // last: the dev_free calls above may have parked buffers
    c->cache.clear();
    for (auto& ev : c->ev_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (hipEvent_t ev : c->tp_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int bi_device_info(bi_ctx* c, char* name, char* arch, int len, int* n_cu, int64_t* hbm_bytes) {
    if (!c) return BI_ERR_INVALID;
    if (name && len > 0) { strncpy(name, c->prop.name, len - 1); name[len - 1] = 0; }
    if (arch && len > 0) { strncpy(arch, c->prop.gcnArchName, len - 1); arch[len - 1] = 0; }
    if (n_cu) *n_cu = c->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)c->prop.totalGlobalMem;
    return BI_OK;
}

void* bi_stream(bi_ctx* c) { return c ? (void*)c->stream : nullptr; }

int bi_sync(bi_ctx* c) {
    if (!c) return BI_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

int bi_set_param(bi_ctx* c, const char* name, int64_t v) {
    if (!c || !name) return BI_ERR_INVALID;
    const ParamDef* p = find_param(name);
    if (!p) return fail(c, BI_ERR_INVALID, "unknown parameter %s", name);
    if (!p->set) return fail(c, BI_ERR_INVALID, "parameter %s is read-only", name);
    return p->set(c, v);
}

int64_t bi_get_param(bi_ctx* c, const char* name) {
    if (!c || !name) return INT64_MIN;
    const ParamDef* p = find_param(name);
    if (!p || !p->get) {
        fail(c, BI_ERR_INVALID, p ? "parameter %s is write-only" : "unknown parameter %s", name);
        return INT64_MIN;
    }
    return p->get(c);
}

int bi_list_params(char* buf, int len) {
    std::string all;
    for (const ParamDef& p : kParams) {
        all += p.name;
        all += p.access == kParamRW ? " rw\n" : (p.access == kParamRead ? " r\n" : " w\n");
    }
    if (buf && len > 0) {
        const size_t n = std::min<size_t>(all.size(), (size_t)len - 1);
        memcpy(buf, all.data(), n);
        buf[n] = 0;
    }
    return (int)all.size() + 1;
}

// ---- model ---------------------------------------------------------------------------------

int bi_model_begin(bi_ctx* c, int d, const int32_t* n_anchor, const double* anchor_z, int S, int64_t B,
                   int bb_source) {
    if (!c) return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (d < 0 || d > kMaxDim) return fail(c, BI_ERR_INVALID, "d=%d outside [0,%d]", d, kMaxDim);
    if (S < 1 || B < 0) return fail(c, BI_ERR_INVALID, "need S >= 1 and B >= 0 (got S=%d B=%lld)", S, (long long)B);
    if (bb_source < -1 || bb_source >= S) return fail(c, BI_ERR_INVALID, "bb_source %d outside [-1,%d)", bb_source, S);
    if (d > 0 && (!n_anchor || !anchor_z)) return fail(c, BI_ERR_INVALID, "anchor arrays are NULL");
    c->model_ready = false;
    c->data_ready = false;  // a new model invalidates the data (likelihood.py:253)
    c->cnt8_valid = false;
    c->pk_valid = false;        // (the packed shadow of the previous model's rows: bi_model_end builds the new one)
    dev_free(c->real_counts);   // (rows of the previous model's padded length)
    c->real_T = 0;
    release_coarse(c);          // (groups of the previous model's bins)
    ++c->epoch;
    c->d = d; c->S = S; c->B = B; c->bb_source = bb_source;
    c->Bp = std::max<int64_t>(kTile, (B + kTile - 1) / kTile * kTile);
    c->unbinned = false;
    c->ev_sorted = false;
    c->n_sets = 1;
    c->set_first.clear();
    c->set_n.clear();
    c->n_anchor.assign(d, 0);
    c->grid.assign(d, {});
    c->A = 1;
    const double* zp = anchor_z;
    for (int i = 0; i < d; ++i) {
        if (n_anchor[i] < 1) return fail(c, BI_ERR_INVALID, "axis %d has %d anchors", i, n_anchor[i]);
        c->n_anchor[i] = n_anchor[i];
        c->grid[i].assign(zp, zp + n_anchor[i]);
        for (int j = 1; j < n_anchor[i]; ++j)
            if (!(c->grid[i][j] > c->grid[i][j - 1]))
                return fail(c, BI_ERR_INVALID, "anchor z values of axis %d are not strictly ascending", i);
        zp += n_anchor[i];
        c->A *= n_anchor[i];
    }
    c->astride.assign(d, 1);
    for (int i = d - 2; i >= 0; --i) c->astride[i] = c->astride[i + 1] * c->n_anchor[i + 1];
    c->eff_axes.clear();
    for (int i = 0; i < d; ++i)
        if (c->n_anchor[i] >= 2) c->eff_axes.push_back(i);
    c->allow_neg.assign(S, 0);
    c->h_mus.assign((size_t)c->A * S, 0.0);
    c->h_nm_tot.assign((size_t)c->A, 0.0);
    c->anchor_set.assign((size_t)c->A, 0);
    // (one tile of slack behind the last row: an event set that starts inside a tile is read in whole tiles from its first column)
    const size_t ps_bytes = ((size_t)c->A * S * c->Bp + kTile) * sizeof(double);
    int rc = dev_alloc(c, c->ps, ps_bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->ps.p, 0, ps_bytes, c->stream));
    if (bb_source >= 0) {
        const size_t nm_bytes = (size_t)c->A * c->Bp * sizeof(double);
        if ((rc = dev_alloc(c, c->nm, nm_bytes))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->nm.p, 0, nm_bytes, c->stream));
        if ((rc = dev_alloc(c, c->nm_tot, (size_t)c->A * sizeof(double)))) return rc;
    }
    c->model_open = true;
    return BI_OK;
}

int bi_model_set_anchor(bi_ctx* c, int64_t ai, const double* ps, const double* mus, const double* nm_row) {
    if (!c || !c->model_open) return fail(c, BI_ERR_STATE, "bi_model_begin first");
    if (ai < 0 || ai >= c->A) return fail(c, BI_ERR_INVALID, "anchor index %lld outside [0,%lld)", (long long)ai, (long long)c->A);
    if (!ps || !mus) return fail(c, BI_ERR_INVALID, "ps / mus are NULL");
    if (c->bb_source >= 0 && !nm_row) return fail(c, BI_ERR_INVALID, "Beeston-Barlow model needs the n_model row");
    HIP_TRY(c, hipSetDevice(c->device));
    double* dst = (double*)c->ps.p + (size_t)ai * c->S * c->Bp;
    if (c->B > 0) HIP_TRY(c, hipMemcpy2DAsync(dst, c->Bp * sizeof(double), ps, c->B * sizeof(double), c->B * sizeof(double), c->S,
                                hipMemcpyHostToDevice, c->stream));
    for (int s = 0; s < c->S; ++s) c->h_mus[(size_t)ai * c->S + s] = mus[s];
    if (c->bb_source >= 0 && c->B > 0) {
        double* nd = (double*)c->nm.p + (size_t)ai * c->Bp;
        HIP_TRY(c, hipMemcpyAsync(nd, nm_row, c->B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    // the host buffers are borrowed only for the duration of the call
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->anchor_set[(size_t)ai] = 1;
    return BI_OK;
}

int bi_model_end(bi_ctx* c) {
    if (!c || !c->model_open) return fail(c, BI_ERR_STATE, "bi_model_begin first");
    for (int64_t a = 0; a < c->A; ++a)
        if (!c->anchor_set[(size_t)a]) return fail(c, BI_ERR_STATE, "anchor %lld was never set", (long long)a);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->bb_source >= 0) {
        // N_c = sum_b n_model[c, i, b]; N(z) is linear in the corner weights (likelihood.py:645)
        hipLaunchKernelGGL(k_row_total, dim3((unsigned)c->A), dim3(kThreads), 0, c->stream, (const double*)c->nm.p, c->B,
                           c->Bp, (double*)c->nm_tot.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(c->h_nm_tot.data(), c->nm_tot.p, (size_t)c->A * sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
    }
    {
        // row sums T_k and non-negativity of the templates: preconditions / constants of the sparse forms
        const int64_t rows = c->A * c->S;
        int rc = dev_alloc(c, c->scratch, (size_t)rows * 3 * sizeof(double));
        if (rc) return rc;
        hipLaunchKernelGGL(k_row_stats, dim3((unsigned)rows), dim3(kThreads), 0, c->stream, (const double*)c->ps.p, c->B,
                           c->Bp, (double*)c->scratch.p);
        HIP_TRY(c, hipGetLastError());
        std::vector<double> st((size_t)rows * 3);
        HIP_TRY(c, hipMemcpyAsync(st.data(), c->scratch.p, st.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->h_rowsum.assign((size_t)rows, 0.0);
        c->h_rowmin.assign((size_t)rows, 0.0);
        c->ps_nonneg = true;
        c->ps_finite = true;
        for (int64_t r = 0; r < rows; ++r) {
            c->h_rowsum[(size_t)r] = st[(size_t)r * 3];
            c->h_rowmin[(size_t)r] = st[(size_t)r * 3 + 1];
            if (!(st[(size_t)r * 3 + 1] >= 0.0) || st[(size_t)r * 3 + 2] != 0.0) c->ps_nonneg = false;
            if (st[(size_t)r * 3 + 2] != 0.0) c->ps_finite = false;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    build_packed_rows(c);       // (ps is final: no writer of it runs outside bi_model_begin ... bi_model_end)
    c->model_open = false;
    c->model_ready = true;
    return BI_OK;
}

int bi_upload_model(bi_ctx* c, int d, const int32_t* n_anchor, const double* anchor_z, int S, int64_t B,
                    const double* ps, const double* mus, const double* n_model, int bb_source) {
    if (!c) return BI_ERR_INVALID;
    if (!ps || !mus) return fail(c, BI_ERR_INVALID, "ps / mus are NULL");
    if (bb_source >= 0 && !n_model) return fail(c, BI_ERR_INVALID, "bb_source given but n_model is NULL");
    int rc = bi_model_begin(c, d, n_anchor, anchor_z, S, B, bb_source);
    if (rc) return rc;
    // one strided copy for the whole tensor: rows are (anchor, source)
    if (B > 0) HIP_TRY(c, hipMemcpy2DAsync(c->ps.p, c->Bp * sizeof(double), ps, B * sizeof(double), B * sizeof(double),
                                (size_t)c->A * S, hipMemcpyHostToDevice, c->stream));
    std::copy(mus, mus + (size_t)c->A * S, c->h_mus.begin());
    if (bb_source >= 0) {
        // only row bb_source of every anchor is ever used (likelihood.py:643)
        if (B > 0) HIP_TRY(c, hipMemcpy2DAsync(c->nm.p, c->Bp * sizeof(double), n_model + (size_t)bb_source * B,
                                    (size_t)S * B * sizeof(double), B * sizeof(double), (size_t)c->A,
                                    hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::fill(c->anchor_set.begin(), c->anchor_set.end(), 1);
    return bi_model_end(c);
}

int bi_set_allow_negative(bi_ctx* c, const int32_t* allow) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!allow) return fail(c, BI_ERR_INVALID, "allow is NULL");
    c->allow_neg.assign(allow, allow + c->S);
    return BI_OK;
}

int bi_set_bb_totals(bi_ctx* c, const double* totals) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->bb_source < 0) return fail(c, BI_ERR_INVALID, "the model has no Beeston-Barlow source");
    if (!totals) return fail(c, BI_ERR_INVALID, "totals is NULL");
    c->h_nm_tot.assign(totals, totals + c->A);
    ++c->epoch;
    return BI_OK;
}

int bi_get_bb_totals(bi_ctx* c, double* totals) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->bb_source < 0 || !totals) return fail(c, BI_ERR_INVALID, "no Beeston-Barlow source / totals is NULL");
    std::copy(c->h_nm_tot.begin(), c->h_nm_tot.end(), totals);
    return BI_OK;
}

// ---- data ----------------------------------------------------------------------------------

int bi_upload_counts(bi_ctx* c, int64_t T, const double* counts) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (T < 1 || !counts) return fail(c, BI_ERR_INVALID, "need T >= 1 datasets and a counts pointer");
    if (c->unbinned) return fail(c, BI_ERR_STATE, "the context holds an unbinned likelihood: it has no binned counts");
    if (c->B < 1) return fail(c, BI_ERR_INVALID, "a binned likelihood needs at least one bin");
    HIP_TRY(c, hipSetDevice(c->device));
    c->data_ready = false;
    ++c->epoch;
    const size_t bytes = (size_t)T * c->Bp * sizeof(double);
    if ((rc = dev_alloc(c, c->counts, bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->counts.p, 0, bytes, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(c->counts.p, c->Bp * sizeof(double), counts, c->B * sizeof(double),
                                c->B * sizeof(double), (size_t)T, hipMemcpyHostToDevice, c->stream));
    return finish_counts(c, T);
}


// ---- set_data on the device ---------------------------------------------------------------------

int bi_set_analysis_space(bi_ctx* c, int k, const int32_t* n_edges, const double* edges) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    AxisWalk ax;
    if ((rc = walk_axes(c, k, n_edges, edges, 2, false, kSpaceWords, ax))) return rc;
    if (ax.bins != c->B) return fail(c, BI_ERR_INVALID, "analysis space has %lld bins, the model %lld", (long long)ax.bins, (long long)c->B);
    HIP_TRY(c, hipSetDevice(c->device));
    c->space_k = k;
    c->space_n_edges.assign(n_edges, n_edges + k);
    const std::vector<double> flat(edges, edges + ax.flat);      // (alive until the copy below is complete)
    if ((rc = dev_upload(c, c->space_edges, flat))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

int bi_upload_events(bi_ctx* c, int64_t N, const double* coords) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->space_k < 1) return fail(c, BI_ERR_STATE, "bi_set_analysis_space first");
    if (c->unbinned) return fail(c, BI_ERR_STATE, "the context holds an unbinned likelihood");
    if (N < 0 || (N > 0 && !coords)) return fail(c, BI_ERR_INVALID, "bad N / coords");
    HIP_TRY(c, hipSetDevice(c->device));
    c->data_ready = false;
    ++c->epoch;
    const size_t bytes = (size_t)c->Bp * sizeof(double);
    if ((rc = dev_alloc(c, c->counts, bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->counts.p, 0, bytes, c->stream));
    if (N > 0) {
        ScratchBuf d_ev;
        if ((rc = dev_alloc(c, d_ev, (size_t)N * c->space_k * sizeof(double)))) return rc;
        hipError_t e = hipMemcpyAsync(d_ev.p, coords, (size_t)N * c->space_k * sizeof(double), hipMemcpyHostToDevice, c->stream);
        HistArgs h{};
        h.k = c->space_k;
        int off = 0;
        for (int i = 0; i < c->space_k; ++i) { h.n_edges[i] = c->space_n_edges[(size_t)i]; h.edge_off[i] = off; off += h.n_edges[i]; }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_histogram, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                               (const double*)d_ev.p, N, h, (const double*)c->space_edges.p, (double*)c->counts.p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // coords are borrowed for the call only
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_upload_events: %s", hipGetErrorString(e));
    }
    return finish_counts(c, 1);
}

int bi_histogram_events(bi_ctx* c, int k, const int32_t* n_edges, const double* edges, int64_t N, const double* coords,
                        double* counts) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
    AxisWalk ax;              // (a missing counts buffer is reported with the axes)
    int rc = walk_axes(c, k, n_edges, counts ? edges : nullptr, 2, false, kHistWords, ax);
    if (rc) return rc;
    if (N < 0 || (N > 0 && !coords)) return fail(c, BI_ERR_INVALID, "bad N / coords");
    HistArgs h{};
    h.k = k;
    ax.put(h.n_edges, h.edge_off);
    const int64_t bins = ax.bins;
    const int off = ax.flat;
    HIP_TRY(c, hipSetDevice(c->device));
    ScratchBuf d_ev, d_edges, d_counts;
    if ((rc = dev_alloc(c, d_counts, (size_t)bins * sizeof(double))) || (rc = dev_alloc(c, d_edges, (size_t)off * sizeof(double))) ||
        (N > 0 && (rc = dev_alloc(c, d_ev, (size_t)N * k * sizeof(double))))) return rc;
    hipError_t e = hipMemsetAsync(d_counts.p, 0, (size_t)bins * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_edges.p, edges, (size_t)off * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && N > 0) {
        e = hipMemcpyAsync(d_ev.p, coords, (size_t)N * k * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_histogram, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                               (const double*)d_ev.p, N, h, (const double*)d_edges.p, (double*)d_counts.p);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(counts, d_counts.p, (size_t)bins * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_histogram_events: %s", hipGetErrorString(e));
    return BI_OK;
}

// ---- planning ------------------------------------------------------------------------------

void bi_plan_destroy(bi_ctx* c, bi_plan* p) {
    if (!p) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
    free_plan_buffers(p);
    delete p;
}

int64_t bi_plan_bytes(const bi_plan* p) { return p ? p->bytes : 0; }
int64_t bi_plan_launches(const bi_plan* p) { return p ? p->launches : 0; }

int bi_plan_points(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset,
                   bi_plan** out) {
    if (c && multi_set(c)) return refuse_sets(c, "bi_plan_points");
    return plan_points(c, P, z, rate_scale, dataset, out);
}

int bi_plan_points_share(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, int share_rank,
                         int share_world, bi_plan** out) {
    if (c && multi_set(c)) return refuse_sets(c, "bi_plan_points_share");
    if (share_world < 1) return fail(c, BI_ERR_INVALID, "share_world must be >= 1");
    return plan_points(c, P, z, rate_scale, dataset, out, /*transient=*/false, share_rank, share_world);
}

}  // extern "C"

namespace {

// bi_plan_points_resident; check_pointers = false: the caller made the buffers itself (bi_sample_stretch: its proposal buffers)
int plan_points_resident_impl(bi_ctx* c, int64_t P, const double* z_dev, const double* rate_scale_dev, const int64_t* dataset_dev,
                              int share_rank, int share_world, bi_plan** out, bool check_pointers) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!out) return fail(c, BI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (P < 0 || P > (int64_t)1 << 30) return fail(c, BI_ERR_INVALID, "P outside [0, 2^30]");
    if (share_world < 1 || share_rank < 0 || share_rank >= share_world)
        return fail(c, BI_ERR_INVALID, "share %d outside [0,%d)", share_rank, share_world);
    if (c->d > 0 && P > 0 && !z_dev) return fail(c, BI_ERR_INVALID, "z_dev is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    if (P == 0) return plan_points(c, 0, nullptr, nullptr, nullptr, out);
    const void* ptrs[3] = {c->d > 0 ? (const void*)z_dev : nullptr, rate_scale_dev, dataset_dev};
    const char* names[3] = {"z_dev", "rate_scale_dev", "dataset_dev"};
    for (int i = 0; i < 3 && check_pointers; ++i) {
        if (!ptrs[i]) continue;
        hipPointerAttribute_t at;
        const hipError_t e = hipPointerGetAttributes(&at, ptrs[i]);
        if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != c->device) {
            (void)hipGetLastError();
            return fail(c, BI_ERR_INVALID, "%s is not device memory of GPU %d", names[i], c->device);
        }
    }
    const bool sparse = ItemRoute(c).compact;
    if (!sparse && !c->dense_counts)
        return fail(c, BI_ERR_STATE, "the datasets exist only as non-empty-bin lists (device-generated toys): point "
                                     "evaluations need the compacted templates (sparse mode, budget) or bi_eval_datasets");
    // (sources that may go negative: an infinite rate among the points is found by the planner itself and refused;
    //  Beeston-Barlow: refused when some point needs the host planner's exact totals)
    c->plan_refused = 0;
    rc = plan_points_device(c, P, z_dev, rate_scale_dev, dataset_dev, sparse, out, share_rank, share_world, true, false);
    if (rc == kPlanNeedsHost && (c->plan_refused = 1))
        return fail(c, BI_ERR_INVALID, "resident points are planned on the device: this Beeston-Barlow batch has points at which some bin can "
                                       "have U_b == 0 (or bb_exact = 1) and needs the host planner's exact totals (bi_plan_points)");
    return rc;
}

}  // namespace

extern "C" {

int bi_plan_points_resident(bi_ctx* c, int64_t P, const double* z_dev, const double* rate_scale_dev, const int64_t* dataset_dev,
                            int share_rank, int share_world, bi_plan** out) {
    if (c && multi_set(c)) return refuse_sets(c, "bi_plan_points_resident");
    return plan_points_resident_impl(c, P, z_dev, rate_scale_dev, dataset_dev, share_rank, share_world, out, true);
}

int bi_plan_share_info(const bi_plan* p, int64_t* n_valid, int64_t* lo, int64_t* hi) {
    if (!p || !p->shared) return BI_ERR_INVALID;
    if (n_valid) *n_valid = p->n_valid;
    if (lo) *lo = p->share_lo;
    if (hi) *hi = p->share_hi;
    return BI_OK;
}

int bi_plan_unsort(bi_ctx* c, bi_plan* plan, const double* gathered_dev, int64_t stride, double* full_dev) {
    if (!c || !plan) return BI_ERR_INVALID;
    if (!plan->shared) return fail(c, BI_ERR_INVALID, "bi_plan_unsort: not a share of a dealt scan (bi_plan_points_share)");
    const int64_t per_rank = (plan->n_valid + plan->share_world - 1) / plan->share_world;
    if (!gathered_dev || !full_dev || stride < per_rank) return fail(c, BI_ERR_INVALID, "bi_plan_unsort: NULL buffer or stride %lld < %lld", (long long)stride, (long long)per_rank);
    HIP_TRY(c, hipSetDevice(c->device));
    if (plan->P > 0)
        hipLaunchKernelGGL(k_unsort_share, dim3((unsigned)((plan->P + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, gathered_dev,
                           stride, plan->share_world, plan->n_valid, plan->P, (const int64_t*)plan->sorted_idx.p, full_dev);
    HIP_TRY(c, hipGetLastError());
    return BI_OK;
}

int bi_run_plan(bi_ctx* c, bi_plan* plan, double* out_dev) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!plan) return fail(c, BI_ERR_INVALID, "plan is NULL");
    if (plan->epoch != c->epoch) return fail(c, BI_ERR_STATE, "plan is stale: model or data were uploaded after it was made");
    HIP_TRY(c, hipSetDevice(c->device));
    double* out = out_dev ? out_dev : (double*)plan->out.p;
    const bool bb = c->bb_source >= 0;
    const int nc = 1 << (int)c->eff_axes.size();
    LaunchArgs a{};
    a.ps = plan->sparse ? (const double*)c->ps_c.p : (const double*)c->ps.p;
    a.nm = (const double*)c->nm.p;
    a.counts = plan->sparse ? (const double*)c->cnt_c.p : (const double*)c->counts.p;
    a.B = c->B; a.Bp = c->Bp;
    a.outlier = c->outlier;
    a.nan_S = (c->unbinned && !c->ps_finite) ? c->S : 0;
    a.n0 = bb ? nc * (c->S - 1) : nc * c->S;
    a.n1 = bb ? nc : 0; a.n2 = bb ? nc : 0;
    a.n_tiles = n_tiles_of(c);
    a.chunks = (int)c->tile_chunks;
    const int NS = a.n0 + a.n1 + a.n2;
    c->last_streamed_bytes = plan->bytes;
    // the morph launches below read the one-byte copy of the counts when every dataset of the plan has an exact one
    const bool narrow = plan->narrow && !plan->sparse && narrow_on(c);
    // ... and the packed shadow of the template rows when the model has a valid one: one byte less per value of every row
    const bool packed = !plan->sparse && !bb && packed_on(c);
    c->last_packed_saved = 0;
    if (plan->use_scan) {
        bi_plan::Class& k = plan->classes[0];
        ScanArgs sa{};
        sa.ps = a.ps; sa.counts = a.counts;
        if (plan->sorted) {
            if (c->sorted_epoch != c->epoch || !c->sorted_ok) return fail(c, BI_ERR_STATE, "plan is stale: the count-sorted rows are gone");
            sa.ps = (const double*)c->ps_sorted.p; sa.counts = (const double*)c->cnt_sorted.p;
            ++c->n_sorted_scans;
        }
        sa.rowoff = (const int64_t*)k.rowoff.p; sa.coef = (const double*)k.coef.p;
        sa.item_cnt = (const int64_t*)k.item_cnt.p; sa.item_tiles = (const int32_t*)k.item_tiles.p;
        sa.grp_first = (const int64_t*)plan->grp_first.p; sa.grp_items = (const int32_t*)plan->grp_items.p;
        sa.partial = (double*)k.partial.p; sa.NS = NS; sa.nslots = k.nbx;
        HIP_TRY(c, hipMemsetAsync(k.partial.p, 0, (size_t)k.n_items * k.nbx * k.G * sizeof(double), c->stream));
        {
            EventScope ev(c);
            ++c->n_scan_launches;
            const dim3 sgrid((unsigned)(k.nbx / 4), (unsigned)plan->n_groups);
            c->last_scan_groups = plan->n_groups; c->last_scan_max_items = plan->max_group_items;
            c->last_scan_cb = plan->by_count ? 4 : (plan->scan_cb == 2 ? 2 : 4);
            c->last_scan_by_count = plan->by_count ? 1 : 0;
            c->last_scan_prod = 0;                  // (launch_scan_mfma sets it where it takes the PROD = 1 instantiation)
            if (plan->by_count) {
                // rows ordered by count (all bins of dense data, or the compacted non-empty bins): 64-bin strips, four items at a time
                sa.n_groups = (int)plan->n_groups;
                sa.xcd_mode = (int)c->scan_xcd;
                sa.share_slow = (int)c->scan_share_slow;
                const int64_t scan_blocks = (int64_t)(k.nbx / 4) * (c->scan_xcd == 2 ? (plan->n_groups + 7) / 8 * 8 : plan->n_groups);
                launch_scan_sorted(c, NS, dim3((unsigned)((scan_blocks + 7) / 8 * 8)), sa);
            } else
                launch_scan_mfma(c, plan->scan_cb == 2 ? 2 : 4, plan->sparse, NS, sgrid, sa);
        }
        hipLaunchKernelGGL(k_finish_scan, dim3((unsigned)((k.n_items + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0,
                           c->stream, (const double*)k.partial.p, k.nbx, k.n_items, (const int64_t*)k.perm.p,
                           (const double*)k.slot_lg.p, out);
    }
    if (plan->bb_kgt && !plan->classes.empty()) {
        // Beeston-Barlow batch on the matrix cores: one launch over (tile ranges, groups, quads of a group's items), then the
        // ordinary finish of the per-block partial sums and status bits
        bi_plan::Class& k = plan->classes[0];
        BbScanArgs ba{};
        ba.ps = a.ps; ba.nm = a.nm; ba.counts = a.counts;
        ba.rowoff = (const int64_t*)k.rowoff.p; ba.coef = (const double*)k.coef.p; ba.aux = (const double*)k.aux.p;
        ba.item_cnt = (const int64_t*)k.item_cnt.p;
        ba.grp_first = (const int64_t*)plan->grp_first.p; ba.grp_items = (const int32_t*)plan->grp_items.p;
        ba.partial = (double*)k.partial.p; ba.pflags = (unsigned*)k.pflags.p;
        ba.B = c->B; ba.n0 = a.n0; ba.nc = a.n1; ba.n_tiles = (int)((c->B + 15) / 16);
        const int64_t quads = std::max<int64_t>(1, (plan->max_group_items + 3) / 4);
        {
            EventScope ev(c);
            ++c->n_bb_scan_launches;
            launch_scan_bb(c, plan->bb_kgt, dim3((unsigned)k.nbx, (unsigned)plan->n_groups, (unsigned)quads), ba);
        }
        launch_finish(c, (const double*)k.partial.p, (const unsigned*)k.pflags.p, k.nbx, k.G, k.n_items * k.G, (const int64_t*)k.perm.p,
                      (const double*)k.slot_lg.p, out, (int32_t*)plan->status.p);
    }
    for (auto& k : plan->classes) {
        if (plan->use_scan || plan->bb_kgt) break;
        for (int64_t i0 = 0; i0 < k.n_items; i0 += 65535) {
            const int64_t ni = std::min<int64_t>(65535, k.n_items - i0);
            LaunchArgs b = a;
            b.rowoff = (const int64_t*)k.rowoff.p + i0 * NS;
            b.coef = (const double*)k.coef.p + i0 * NS * k.G;
            b.aux = (const double*)k.aux.p + i0 * k.G * 2;
            b.item_cnt = (const int64_t*)k.item_cnt.p + i0;
            b.item_tiles = (const int32_t*)k.item_tiles.p + i0;
            b.partial = (double*)k.partial.p + i0 * k.nbx * k.G;
            b.pflags = (unsigned*)k.pflags.p + i0 * k.nbx * k.G;
            // nontemporal row loads when no two items touch the same anchor model -- or when an item streams more than the
            // Infinity Cache can keep (> 1 GiB: a shared anchor's rows are gone before the other item asks for them;
            // C5's 5.65 GB passes: 6.4 instead of 6.2 TB/s with 4 ... 16 items per call)
            const bool huge_items = (int64_t)sizeof(double) * (NS + 1) * c->Bp > ((int64_t)1 << 30);
            const bool nt = !plan->sparse && (c->nt_loads == 1 || (c->nt_loads == 2 && (plan->no_reuse || huge_items)));
            // few items (a fit's or a bench step's batch): the last block of every item finishes it inside the launch
            // (at most 256 collecting blocks at a time: they wait for their siblings, and must never be able to hold
            // every slot of the chip while siblings still need one, whatever order the blocks are dispatched in)
            const bool fuse = c->fuse_finish && k.n_items <= 256 && k.n_items * k.nbx * k.G <= kMailSlots &&
                              k.n_items * k.G <= kMailFlagWords && !ensure_mail(c);
            if (fuse) {
                b.fin_mail = (double*)c->mail.p;
                b.fin_flags = (unsigned*)c->mail_flags.p;
                b.fin_perm = (const int64_t*)k.perm.p;
                b.fin_slot_lg = (const double*)k.slot_lg.p;
                b.fin_out = out;
                b.fin_status = (int32_t*)plan->status.p;
                arm_mail(c, b);
            }
            if (narrow) {
                b.cnt8 = (const uint8_t*)c->cnt8.p;
                c->last_streamed_bytes -= 7 * c->Bp * ni;
                ++c->n_narrow_launches;
            }
            if (packed) {
                use_packed_rows(c, b);
                c->last_packed_saved += c->Bp * (int64_t)a.n0 * ni;
            }
            launch_morph_g(c, k.G, b, dim3((unsigned)k.nbx, (unsigned)ni), bb, nt);
            c->last_morph_nbx = k.nbx; c->last_morph_items = ni; c->last_morph_fused = fuse ? 1 : 0;
            if (fuse) continue;
            launch_finish(c, b.partial, b.pflags, k.nbx, k.G, ni * k.G, (const int64_t*)k.perm.p + i0 * k.G,
                          (const double*)k.slot_lg.p + i0 * k.G, out, (int32_t*)plan->status.p);
        }
    }
    if (plan->valid) {
        // split dense scan: the classes above were the non-empty-bin pass; now every bin of every cell, on the matrix cores
        bi_plan::Class& k = plan->classes[0];
        ValidArgs va{};
        va.ps = (const double*)c->ps.p;
        va.rowoff = (const int64_t*)k.rowoff_full.p; va.coef = (const double*)k.coef.p;
        va.grp_first = (const int64_t*)plan->grp_first.p; va.grp_items = (const int32_t*)plan->grp_items.p;
        va.bad = (unsigned*)plan->bad.p; va.NS = NS; va.nslots = plan->valid_nslots;
        va.n_strips = n_tiles_of(c) * (kTile / 64);
        HIP_TRY(c, hipMemsetAsync(plan->bad.p, 0, (size_t)k.n_items * k.G * sizeof(unsigned), c->stream));
        {
            EventScope ev(c);
            ++c->n_valid_launches;
            c->last_scan_groups = plan->n_groups; c->last_scan_max_items = plan->max_group_items;
            const dim3 vgrid((unsigned)(plan->valid_nslots / 4), (unsigned)plan->n_groups);
            launch_scan_valid(c, NS, vgrid, va);
        }
        const int64_t n_slots = k.n_items * k.G;
        hipLaunchKernelGGL(k_apply_bad, dim3((unsigned)((n_slots + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                           (const unsigned*)plan->bad.p, (const int64_t*)k.perm.p, n_slots, out);
    }
    if (plan->shared) {
        // (rejected points belong to no share: bi_plan_unsort answers them)
    } else if (plan->n_bad > 0 && plan->device_planned)
        hipLaunchKernelGGL(k_fill_bad_by_status, dim3((unsigned)((plan->P + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                           (const int32_t*)plan->status.p, plan->P, out);
    else if (plan->n_bad > 0)
        hipLaunchKernelGGL(k_fill_const, dim3((unsigned)((plan->n_bad + 255) / 256)), dim3(256), 0, c->stream, out,
                           (const int64_t*)plan->bad_idx.p, plan->n_bad, -std::numeric_limits<double>::infinity());
    if (plan->n_nan > 0)
        hipLaunchKernelGGL(k_fill_const, dim3((unsigned)((plan->n_nan + 255) / 256)), dim3(256), 0, c->stream, out,
                           (const int64_t*)plan->nan_idx.p, plan->n_nan, std::numeric_limits<double>::quiet_NaN());
    HIP_TRY(c, hipGetLastError());
    return BI_OK;
}

// BI_ST_INTERNAL has been reported for this plan: empty the mailbox, and take the bit out of the plan's (sticky) status words
static void internal_reported(bi_ctx* c, bi_plan* plan) {
    reset_mail(c);
    if (!plan->P) return;
    if (plan->host_results) {
        int32_t* st = (int32_t*)plan->status.p;
        for (int64_t p = 0; p < plan->P; ++p) st[p] &= ~BI_ST_INTERNAL;
    } else {
        hipLaunchKernelGGL(k_status_clear, dim3((unsigned)std::min<int64_t>(1024, (plan->P + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           c->stream, (int32_t*)plan->status.p, plan->P, (int32_t)BI_ST_INTERNAL);
        (void)hipStreamSynchronize(c->stream);
    }
}

int bi_plan_read(bi_ctx* c, bi_plan* plan, double* out, int32_t* status) {
    if (!c || !plan) return BI_ERR_INVALID;
    if (out && plan->shared) return fail(c, BI_ERR_INVALID, "bi_plan_read: a share's results are in sorted order: gather them and call bi_plan_unsort");
    HIP_TRY(c, hipSetDevice(c->device));
    if (out && plan->P)
        HIP_TRY(c, hipMemcpyAsync(out, plan->out.p, (size_t)plan->P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status && plan->P)
        HIP_TRY(c, hipMemcpyAsync(status, plan->status.p, (size_t)plan->P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (status) {
        for (int64_t p = 0; p < plan->P; ++p)
            if (status[p] & BI_ST_INTERNAL) { internal_reported(c, plan); break; }
        return BI_OK;
    }
    int32_t any = 0;
    return bi_plan_status(c, plan, &any);
}

int bi_plan_status(bi_ctx* c, bi_plan* plan, int32_t* status_or) {
    if (!c || !plan) return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int32_t any = 0;
    if (plan->P) {
        if (plan->host_results) {              // the status words already sit in pinned host memory
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            const int32_t* st = (const int32_t*)plan->status.p;
            for (int64_t p = 0; p < plan->P; ++p) any |= st[p];
        } else {
            ScratchBuf d_or;
            int rc = dev_alloc(c, d_or, 64);
            if (rc) return rc;
            hipError_t e = hipMemsetAsync(d_or.p, 0, 4, c->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_status_or, dim3((unsigned)std::min<int64_t>(1024, (plan->P + kThreads - 1) / kThreads)), dim3(kThreads),
                                   0, c->stream, (const int32_t*)plan->status.p, plan->P, (int32_t*)d_or.p);
                e = hipGetLastError();
            }
            // (the word comes back through the planner's pinned report block: no copy into pageable memory, no stream synchronisation)
            if (e == hipSuccess) e = plan_report(c, ReportPiece{(const uint32_t*)d_or.p, 1, 0});
            if (e == hipSuccess) any = *(const int32_t*)c->plan_host;
            if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_plan_status: %s", hipGetErrorString(e));
        }
    }
    if (any & BI_ST_INTERNAL) internal_reported(c, plan);
    if (status_or) *status_or = any;
    return BI_OK;
}

int bi_eval(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* out,
            int32_t* status) {
    if (!c) return BI_ERR_INVALID;
    if (P > 0 && !out) return fail(c, BI_ERR_INVALID, "out is NULL");
    if (P == 1) {
        int rc1 = check_ready(c, true);
        if (rc1) return rc1;
        if (c->d > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
        HIP_TRY(c, hipSetDevice(c->device));
        if (status) *status = 0;
        return eval_single(c, z, rate_scale, dataset ? dataset[0] : 0, out, status);
    }
    if (multi_set(c)) {                // several event sets: one work item per point over its own set (bi_grad.h)
        int rc1 = check_ready(c, true);
        if (rc1) return rc1;
        if (P < 0) return fail(c, BI_ERR_INVALID, "bad P");
        if (c->d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
        return eval_grad_points(c, P, z, rate_scale, dataset, out, nullptr, status, true);
    }
    bi_plan* plan = nullptr;
    int rc = plan_points(c, P, z, rate_scale, dataset, &plan, /*transient=*/true);
    if (rc) return rc;
    rc = bi_run_plan(c, plan, nullptr);
    if (!rc && plan->host_results) {   // small batch: the finish kernel wrote out / status into pinned host memory
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, BI_ERR_HIP, "bi_eval: %s", hipGetErrorString(e));
        if (!rc && P) {
            memcpy(out, plan->out.p, (size_t)P * sizeof(double));
            if (status) memcpy(status, plan->status.p, (size_t)P * sizeof(int32_t));
            const int32_t* st = (const int32_t*)plan->status.p;
            for (int64_t p = 0; p < P; ++p)
                if (st[p] & BI_ST_INTERNAL) { reset_mail(c); break; }
        }
    } else if (!rc) {
        rc = bi_plan_read(c, plan, out, status);
    }
    bi_plan_destroy(c, plan);
    return rc;
}

// ---- one evaluation in two halves (value + analytic gradient, bi_eval_grad: bi_grad.h) ----------

// The two halves of bi_eval(P = 1), for callers that evaluate several contexts at once (a sum of likelihoods, one
// context per term): begin on every context, then end on every context -- the launches overlap.
int bi_eval_begin(bi_ctx* c, const double* z, const double* rate_scale, int64_t dataset) {
    if (!c) return BI_ERR_INVALID;
    if (c->pending) return fail(c, BI_ERR_STATE, "bi_eval_begin: the previous bi_eval_begin has not been collected with bi_eval_end");
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (c->d > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = eval_single(c, z, rate_scale, dataset, nullptr, nullptr, /*wait=*/false);
    if (rc) c->pending = 0;
    return rc;
}

int bi_eval_end(bi_ctx* c, double* out, int32_t* status) {
    if (!c || !out) return BI_ERR_INVALID;
    if (!c->pending) return fail(c, BI_ERR_STATE, "bi_eval_end without bi_eval_begin");
    const int kind = c->pending;
    c->pending = 0;
    if (kind == 2) {
        *out = c->pending_ll;
        if (status) *status = c->pending_status;
        return BI_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (status) *status = 0;
    return single_wait(c, c->pending_seq, out, status);
}

// ---- toy-MC form (bi_toys.h) ----------------------------------------------------------------

int bi_eval_datasets_points(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int64_t t0, int64_t t1, double* out,
                            int32_t* status) {
    if (!c) return BI_ERR_INVALID;
    return eval_datasets_points_impl(c, P, z, rate_scale, t0, t1, out, nullptr, status);
}

int bi_eval_datasets_points_device(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int64_t t0, int64_t t1,
                                   double* out_dev, int32_t* status) {
    if (!c) return BI_ERR_INVALID;
    if (P > 0 && t1 > t0 && !out_dev) return fail(c, BI_ERR_INVALID, "out_dev is NULL");
    return eval_datasets_points_impl(c, P, z, rate_scale, t0, t1, nullptr, out_dev, status);
}

int bi_eval_datasets(bi_ctx* c, const double* z, const double* rate_scale, int64_t t0, int64_t t1, double* out,
                     int32_t* status) {
    return eval_datasets_impl(c, z, rate_scale, t0, t1, out, nullptr, status);
}

int bi_eval_datasets_device(bi_ctx* c, const double* z, const double* rate_scale, int64_t t0, int64_t t1, double* out_dev,
                            int32_t* status) {
    if (t1 > t0 && !out_dev) return fail(c, BI_ERR_INVALID, "out_dev is NULL");
    return eval_datasets_impl(c, z, rate_scale, t0, t1, nullptr, out_dev, status);
}


// ---- toy-MC generation -------------------------------------------------------------------------

// a truth point of a generator call: its place on the anchor grid and its rates
struct ToyTruth {
    PointGeom g;
    std::vector<double> r;
};

// The generator: the non-empty-bin lists (nz_*, lgsum) of T = sum n_toys toys, n_toys[h] of them at truth h, truth-major; toy t
// of the call is toy toy_offset + t of the seed's ensemble.  Every truth picks its own method (meth: 1 = event by event, 0 = bin
// by bin, -1 = no toys), which splits the toys into at most two groups; from the draws onward each group is one set of launches
// and the scans and read-backs run once, whatever the number of truths.  The scratch is back in the recycle cache on return.
static int draw_toy_lists(bi_ctx* c, const std::vector<ToyTruth>& truths, const int64_t* n_toys, int64_t T, uint64_t seed,
                          std::vector<int32_t>& meth) {
    int rc;
    const int64_t H = (int64_t)truths.size(), B = c->B, Bp = c->Bp;
    std::vector<int64_t> rowoff, first_row((size_t)H + 1, 0), first_toy((size_t)H + 1, 0);
    std::vector<double> coef;
    for (int64_t h = 0; h < H; ++h) {
        const PointGeom& g = truths[(size_t)h].g;
        const size_t k0 = rowoff.size(), NS = g.w.size() * (size_t)c->S;
        rowoff.resize(k0 + NS);
        coef.resize(k0 + NS);
        point_streams(c, g, truths[(size_t)h].r.data(), rowoff.data() + k0, coef.data() + k0);
        first_row[(size_t)h + 1] = (int64_t)rowoff.size();
        first_toy[(size_t)h + 1] = first_toy[(size_t)h] + n_toys[h];
    }
    const int n_tiles = n_tiles_of(c);
    const int64_t slots = (int64_t)c->prop.multiProcessorCount * c->blocks_per_cu;
    const int nmu = (int)std::min<int64_t>(n_tiles, slots);
    const int nchunks = (int)((B + kNzChunk - 1) / kNzChunk);
    ScratchBuf d_row, d_coef, d_mu, d_p0;
    if ((rc = dev_upload(c, d_row, rowoff)) || (rc = dev_upload(c, d_coef, coef)) ||
        (rc = dev_alloc(c, d_mu, (size_t)H * Bp * sizeof(double))) ||
        (rc = dev_alloc(c, d_p0, (size_t)H * Bp * sizeof(double))) ||
        (rc = dev_alloc(c, c->scratch, (size_t)nmu * sizeof(double) + (size_t)nmu * sizeof(unsigned) + 64)) ||
        (rc = dev_alloc(c, c->lgsum, (size_t)T * sizeof(double)))) return rc;
    LaunchArgs a{};
    a.ps = (const double*)c->ps.p;
    a.partial = (double*)c->scratch.p;
    a.pflags = (unsigned*)((char*)c->scratch.p + (((size_t)nmu * sizeof(double) + 63) / 64) * 64);
    a.B = B; a.Bp = Bp; a.n_tiles = n_tiles;
    const double* mu = (const double*)d_mu.p;
    const double* p0 = (const double*)d_p0.p;
    for (int64_t h = 0; h < H; ++h) {
        a.rowoff = (const int64_t*)d_row.p + first_row[(size_t)h];
        a.coef = (const double*)d_coef.p + first_row[(size_t)h];
        a.n0 = (int)(first_row[(size_t)h + 1] - first_row[(size_t)h]);
        launch_morph_logmu(c, nmu, a, nullptr, (double*)d_mu.p + h * Bp, 1);
    }
    hipLaunchKernelGGL(k_exp_neg, dim3((unsigned)((H * Bp + 255) / 256)), dim3(256), 0, c->stream, mu, H * Bp, (double*)d_p0.p);
    // Sparse expectations (M = sum mu << B, templates and rates >= 0): event by event -- N ~ Poisson(M), the bins by bisection
    // in the cumulative sums, sorted and run-length encoded per toy (k_toy_events); else one draw per bin.  M, the sort
    // buffer npow2 and with them the choice are each truth's own.
    meth.assign((size_t)H, 0);
    for (int64_t h = 0; h < H; ++h) if (n_toys[h] == 0) meth[(size_t)h] = -1;
    std::vector<double> Mh((size_t)H, 0.0);
    std::vector<int> np2((size_t)H, 1024), ovf((size_t)H, 0);
    std::vector<ToyRef> refA, refB;
    int64_t n_events = 0;
    ScratchBuf d_cdf, d_tmp, d_M, d_np2, d_ovf, d_refA, d_refB, d_nev, d_room, d_nnz, d_tidx, d_tn, d_cnt, d_off, d_lgp;
    hipError_t e;
    if (c->toy_events && c->ps_nonneg && B >= 4096) {
        size_t sb1 = 0, sb2 = 0;
        (void)prim_inclusive_scan_sum(nullptr, sb1, (const double*)nullptr, (double*)nullptr, (size_t)B, c->stream);
        (void)prim_exclusive_scan_sum(nullptr, sb2, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(T + 1), c->stream);
        if ((rc = dev_alloc(c, d_cdf, (size_t)H * B * sizeof(double))) || (rc = dev_alloc(c, d_tmp, std::max<size_t>({sb1, sb2, 256})))) return rc;
        e = hipSuccess;
        for (int64_t h = 0; h < H && e == hipSuccess; ++h) {       // (one scan per row: its tree order is part of the stream)
            size_t tb = d_tmp.bytes;
            e = prim_inclusive_scan_sum(d_tmp.p, tb, mu + h * Bp, (double*)d_cdf.p + h * B, (size_t)B, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&Mh[(size_t)h], (const double*)d_cdf.p + h * B + (B - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "toy generation (cumulative sums): %s", hipGetErrorString(e));
        for (int64_t h = 0; h < H; ++h) {
            const double M = Mh[(size_t)h];
            const double bound = M + 12.0 * std::sqrt(std::max(M, 1.0)) + 32.0;
            int npow2 = 1024;
            while (npow2 < bound && npow2 < 65536) npow2 <<= 1;
            np2[(size_t)h] = npow2;
            if (n_toys[h] > 0 && M > 0.0 && M == M && M < (double)B / 8.0 && npow2 <= 32768) meth[(size_t)h] = 1;
        }
    }
    // (1) the two groups; events per toy of the event group -> room in the provisional lists.  A toy beyond its truth's sort
    // buffer (12 sigma) sends that truth to the bin-by-bin group and the round is made again without it (once at the most:
    // the truths that stay had no such toy).
    for (;;) {
        refA.clear();
        refB.clear();
        for (int64_t h = 0; h < H; ++h)
            for (int64_t j = 0; j < n_toys[h]; ++j)
                (meth[(size_t)h] == 1 ? refB : refA).push_back(ToyRef{(int32_t)(first_toy[(size_t)h] + j), (int32_t)h});
        if (refB.empty()) break;
        const int64_t nB = (int64_t)refB.size();
        if ((rc = dev_upload(c, d_refB, refB)) || (rc = dev_upload(c, d_M, Mh)) || (rc = dev_upload(c, d_np2, np2)) ||
            (rc = dev_alloc(c, d_ovf, (size_t)H * sizeof(int))) || (rc = dev_alloc(c, d_nev, (size_t)(nB + 1) * sizeof(int64_t))) ||
            (rc = dev_alloc(c, d_room, (size_t)(nB + 1) * sizeof(int64_t)))) return rc;
        e = hipMemsetAsync(d_ovf.p, 0, (size_t)H * sizeof(int), c->stream);
        hipLaunchKernelGGL(k_toy_event_counts, dim3((unsigned)((nB + 1 + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_M.p,
                           (const int*)d_np2.p, seed, c->toy_offset, (const ToyRef*)d_refB.p, nB, (int64_t*)d_nev.p, (int*)d_ovf.p);
        size_t tb = d_tmp.bytes;
        if (e == hipSuccess) e = prim_exclusive_scan_sum(d_tmp.p, tb, (const int64_t*)d_nev.p, (int64_t*)d_room.p, (int64_t)0, (size_t)(nB + 1), c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_events, (const int64_t*)d_room.p + nB, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ovf.data(), d_ovf.p, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "toy generation (events per toy): %s", hipGetErrorString(e));
        bool again = false;
        for (int64_t h = 0; h < H; ++h)
            if (ovf[(size_t)h]) { meth[(size_t)h] = 0; again = true; }
        if (!again) break;
    }
    const int64_t nA = (int64_t)refA.size(), nB = (int64_t)refB.size();
    // (2) event group: one block per toy: events -> sorted bins -> (bin, count) runs, written into the toy's room;
    //     bin-by-bin group: the non-empty bins per chunk of every toy
    const int64_t tchunk_ev = 65535, tchunk = 32768;
    std::vector<int64_t> h_nnz((size_t)nB, 0);
    std::vector<int32_t> h_cnt((size_t)nA * nchunks);
    e = hipSuccess;
    if (nB) {
        size_t lds = 0;
        for (int64_t h = 0; h < H; ++h) {
            if (meth[(size_t)h] != 1) continue;
            const int npow2 = np2[(size_t)h];
            lds = std::max(lds, (npow2 <= 16384 ? (size_t)2 * npow2 * sizeof(uint32_t) + 16 * kEvThreads * sizeof(uint16_t)
                                                : (size_t)npow2 * sizeof(uint32_t)) + kEvThreads * (sizeof(int) + sizeof(double)) + 64);
        }
        if ((e = hipFuncSetAttribute((const void*)k_toy_events, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return fail(c, BI_ERR_HIP, "toy generation (LDS size of the event kernel): %s", hipGetErrorString(e));
        if ((rc = dev_alloc(c, d_tidx, (size_t)std::max<int64_t>(n_events, 1) * sizeof(int32_t))) ||
            (rc = dev_alloc(c, d_tn, (size_t)std::max<int64_t>(n_events, 1) * sizeof(double))) ||
            (rc = dev_alloc(c, d_nnz, (size_t)nB * sizeof(int64_t)))) return rc;
        for (int64_t g0 = 0; g0 < nB; g0 += tchunk_ev) {
            const int64_t n = std::min(tchunk_ev, nB - g0);
            hipLaunchKernelGGL(k_toy_events, dim3((unsigned)n), dim3(kEvThreads), lds, c->stream, (const double*)d_cdf.p, B,
                               (const double*)d_M.p, (const int*)d_np2.p, seed, c->toy_offset, (const ToyRef*)d_refB.p + g0,
                               (const int64_t*)d_room.p + g0, (int32_t*)d_tidx.p, (double*)d_tn.p, (int64_t*)d_nnz.p + g0,
                               (double*)c->lgsum.p);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_nnz.data(), d_nnz.p, (size_t)nB * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    }
    if (nA && e == hipSuccess) {
        if ((rc = dev_upload(c, d_refA, refA)) || (rc = dev_alloc(c, d_cnt, (size_t)nA * nchunks * sizeof(int32_t))) ||
            (rc = dev_alloc(c, d_lgp, (size_t)nA * nchunks * sizeof(double)))) return rc;
        for (int64_t g0 = 0; g0 < nA; g0 += tchunk) {
            const int64_t n = std::min(tchunk, nA - g0);
            hipLaunchKernelGGL(k_toy_count, dim3((unsigned)nchunks, (unsigned)n), dim3(kThreads), 0, c->stream, mu, p0, Bp, B, seed,
                               c->toy_offset, (const ToyRef*)d_refA.p + g0, (int32_t*)d_cnt.p + g0 * nchunks, nchunks);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_cnt.data(), d_cnt.p, h_cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "toy generation (non-empty bins per toy): %s", hipGetErrorString(e));
    // (3) non-empty bins per toy -> the offsets of all T lists, in toy order; scatter and pack
    c->h_nz_off.assign((size_t)T + 1, 0);
    for (int64_t i = 0; i < nB; ++i) c->h_nz_off[(size_t)refB[(size_t)i].t + 1] = h_nnz[(size_t)i];
    for (int64_t i = 0; i < nA; ++i) {
        int64_t len = 0;
        for (int q = 0; q < nchunks; ++q) len += h_cnt[(size_t)i * nchunks + q];
        c->h_nz_off[(size_t)refA[(size_t)i].t + 1] = len;
    }
    for (int64_t t = 0; t < T; ++t) c->h_nz_off[(size_t)t + 1] += c->h_nz_off[(size_t)t];
    const int64_t run = c->h_nz_off[(size_t)T];
    std::vector<int64_t> h_off(h_cnt.size());
    for (int64_t i = 0; i < nA; ++i) {
        int64_t at = c->h_nz_off[(size_t)refA[(size_t)i].t];
        for (int q = 0; q < nchunks; ++q) { h_off[(size_t)i * nchunks + q] = at; at += h_cnt[(size_t)i * nchunks + q]; }
    }
    if ((rc = dev_alloc(c, c->nz_idx, (size_t)std::max<int64_t>(run, 1) * sizeof(int32_t))) ||
        (rc = dev_alloc(c, c->nz_n, (size_t)std::max<int64_t>(run, 1) * sizeof(double))) || (rc = dev_upload(c, c->nz_off, c->h_nz_off))) return rc;
    if (nA) {
        if ((rc = dev_upload(c, d_off, h_off))) return rc;
        for (int64_t g0 = 0; g0 < nA; g0 += tchunk) {
            const int64_t n = std::min(tchunk, nA - g0);
            hipLaunchKernelGGL(k_toy_scatter, dim3((unsigned)nchunks, (unsigned)n), dim3(kThreads), 0, c->stream, mu, p0, Bp, B, seed,
                               c->toy_offset, (const ToyRef*)d_refA.p + g0, (const int64_t*)d_off.p + g0 * nchunks, nchunks,
                               (int32_t*)c->nz_idx.p, (double*)c->nz_n.p, (double*)d_lgp.p + g0 * nchunks);
        }
        hipLaunchKernelGGL(k_toy_lgsum, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_lgp.p, nchunks,
                           (const ToyRef*)d_refA.p, nA, (double*)c->lgsum.p);
    }
    for (int64_t g0 = 0; g0 < nB; g0 += tchunk_ev) {
        const int64_t n = std::min(tchunk_ev, nB - g0);
        hipLaunchKernelGGL(k_toy_pack, dim3((unsigned)n), dim3(kThreads), 0, c->stream, (const ToyRef*)d_refB.p + g0,
                           (const int64_t*)d_room.p + g0, (const int64_t*)c->nz_off.p, (const int32_t*)d_tidx.p, (const double*)d_tn.p,
                           (int32_t*)c->nz_idx.p, (double*)c->nz_n.p);
    }
    c->h_lgsum.assign((size_t)T, 0.0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_lgsum.data(), c->lgsum.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "toy generation (lists): %s", hipGetErrorString(e));
    c->last_toy_method = nB > 0 && nA == 0;
    return BI_OK;
}

// the generator's entry: every truth is validated before the context changes; `one`: bi_generate_toys' messages
static int generate_toys_impl(bi_ctx* c, int64_t H, const double* z, const double* rate_scale, const int64_t* n_toys, uint64_t seed,
                              int32_t* method_out, bool one) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (H < 1 || !n_toys) return fail(c, BI_ERR_INVALID, "need H >= 1 truth points and their numbers of toys");
    int64_t T = 0;
    for (int64_t h = 0; h < H; ++h) {
        if (n_toys[h] < 0 && one) break;
        if (n_toys[h] < 0) return fail(c, BI_ERR_INVALID, "n_toys[%lld] = %lld is negative", (long long)h, (long long)n_toys[h]);
        if (n_toys[h] > INT32_MAX - T) return fail(c, BI_ERR_INVALID, "a call draws fewer than 2^31 toys");
        T += n_toys[h];
    }
    if (T < 1) return fail(c, BI_ERR_INVALID, "need T >= 1 toys");
    if (c->B < 1) return fail(c, BI_ERR_INVALID, "a binned likelihood needs at least one bin");
    if (c->d > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<ToyTruth> truths((size_t)H);
    for (int64_t h = 0; h < H; ++h) {
        char where[64] = "toy generation";
        if (!one) snprintf(where, sizeof where, "toy generation (truth %lld)", (long long)h);
        if ((rc = rates_at(c, c, z ? z + h * c->d : nullptr, rate_scale ? rate_scale + h * c->S : nullptr, where, where,
                           truths[(size_t)h].g, truths[(size_t)h].r))) return rc;
    }
    c->data_ready = false;
    c->dense_counts = false;
    c->csr_ready = c->compact_ready = false;
    ++c->epoch;
    dev_free(c->counts);  // the toys exist as non-empty-bin lists only
    c->cnt8_valid = false;  // ... and the narrow copy of the dense counts goes with them (bi_counts_to_dense rebuilds it)
    std::vector<int32_t> meth;
    if ((rc = draw_toy_lists(c, truths, n_toys, T, seed, meth))) return rc;
    if (method_out) std::copy(meth.begin(), meth.end(), method_out);
    c->T = T;
    c->csr_ready = true;
    if ((rc = build_compact_templates(c))) return rc;   // per-toy point evaluations, when the budget allows
    c->data_ready = true;
    return BI_OK;
}

int bi_generate_toys(bi_ctx* c, const double* z, const double* rate_scale, int64_t T, uint64_t seed) {
    if (!c) return BI_ERR_INVALID;
    return generate_toys_impl(c, 1, z, rate_scale, &T, seed, nullptr, true);
}

int bi_generate_toys_points(bi_ctx* c, int64_t H, const double* z, const double* rate_scale, const int64_t* n_toys, uint64_t seed,
                            int32_t* method_out) {
    if (!c) return BI_ERR_INVALID;
    return generate_toys_impl(c, H, z, rate_scale, n_toys, seed, method_out, false);
}

int bi_download_counts(bi_ctx* c, int64_t t, double* out) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (t < 0 || t >= c->T || !out) return fail(c, BI_ERR_INVALID, "dataset %lld outside [0,%lld) or out is NULL", (long long)t, (long long)c->T);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->dense_counts) {
        HIP_TRY(c, hipMemcpyAsync(out, (const double*)c->counts.p + t * c->Bp, (size_t)c->B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return BI_OK;
    }
    if (!c->csr_ready) return fail(c, BI_ERR_STATE, "no counts resident");
    if ((rc = dev_alloc(c, c->logmu, (size_t)c->Bp * sizeof(double)))) return rc;
    const int64_t lo = c->h_nz_off[(size_t)t], nnz = c->h_nz_off[(size_t)t + 1] - lo;
    HIP_TRY(c, hipMemsetAsync(c->logmu.p, 0, (size_t)c->B * sizeof(double), c->stream));
    if (nnz > 0)
        hipLaunchKernelGGL(k_csr_to_dense, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, c->stream,
                           (const int32_t*)c->nz_idx.p + lo, (const double*)c->nz_n.p + lo, nnz, (double*)c->logmu.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, c->logmu.p, (size_t)c->B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}


int bi_counts_to_dense(bi_ctx* c) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (c->dense_counts) return BI_OK;
    if (!c->csr_ready) return fail(c, BI_ERR_STATE, "no counts resident");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->T * c->Bp * sizeof(double);
    if ((rc = dev_alloc(c, c->counts, bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->counts.p, 0, bytes, c->stream));
    for (int64_t t = 0; t < c->T; ++t) {
        const int64_t lo = c->h_nz_off[(size_t)t], nnz = c->h_nz_off[(size_t)t + 1] - lo;
        if (nnz > 0)
            hipLaunchKernelGGL(k_csr_to_dense, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, c->stream,
                               (const int32_t*)c->nz_idx.p + lo, (const double*)c->nz_n.p + lo, nnz, (double*)c->counts.p + t * c->Bp);
    }
    HIP_TRY(c, hipGetLastError());
    build_narrow_counts(c, c->T);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->dense_counts = true;
    ++c->epoch;                                  // plans made over the lists alone are stale
    return BI_OK;
}


// ---- extended unbinned likelihood -----------------------------------------------------------------

int bi_set_unbinned(bi_ctx* c, double outlier_likelihood) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->bb_source >= 0) return fail(c, BI_ERR_INVALID, "Beeston-Barlow applies to binned likelihoods only");
    HIP_TRY(c, hipSetDevice(c->device));
    ++c->epoch;
    c->unbinned = true;
    c->cnt8_valid = false;
    drop_packed_rows(c, true);  // (the rows now hold pdf values at events, read by the unbinned kernels only)
    c->outlier = outlier_likelihood;
    c->csr_ready = c->compact_ready = false;
    // one pseudo dataset with zero lgamma sum; the counts row is never read in this mode
    if ((rc = dev_alloc(c, c->counts, (size_t)c->Bp * sizeof(double)))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->counts.p, 0, (size_t)c->Bp * sizeof(double), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->T = 1;
    c->h_lgsum.assign(1, 0.0);
    c->n_sets = 1;
    c->set_first.assign(1, 0);
    c->set_n.assign(1, c->B);
    c->dense_counts = true;
    c->data_ready = true;
    return BI_OK;
}

}  // extern "C"

// ---- compatibility mode --------------------------------------------------------------------

// bi_interpolate; set: the event set whose columns `which` = 0 hands back (an unbinned context with several sets: N_set columns
// from first_set; otherwise 0)
static int interpolate_set(bi_ctx* c, int which, const double* z, double* out, int64_t set) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!out) return fail(c, BI_ERR_INVALID, "out is NULL");
    if (c->d > 0 && !z) return fail(c, BI_ERR_INVALID, "z is NULL");
    if (which < 0 || which > 2) return fail(c, BI_ERR_INVALID, "which must be 0 (ps), 1 (mus) or 2 (n_model row)");
    if (which == 2 && c->bb_source < 0) return fail(c, BI_ERR_INVALID, "model has no n_model tensor");
    PointGeom g;
    if (!point_geometry(c, z, g))
        return fail(c, BI_ERR_INVALID, "One of the requested xi is out of bounds");  // scipy's ValueError text
    if (which == 1) { interp_mus(c, g, out); return BI_OK; }
    HIP_TRY(c, hipSetDevice(c->device));
    const int nc = (int)g.w.size();
    const int R = which == 0 ? c->S : 1;
    const bool of_set = which == 0 && multi_set(c);
    const int64_t col0 = of_set ? c->set_first[(size_t)set] : 0, nB = of_set ? c->set_n[(size_t)set] : c->B;
    if (of_set && nB == 0) return BI_OK;              // an empty set: nothing to hand back
    std::vector<int64_t> rowoff((size_t)R * nc);
    for (int r = 0; r < R; ++r)
        for (int corner = 0; corner < nc; ++corner) {
            const int64_t a = g.cell_anchor + corner_offset(c, corner);
            rowoff[(size_t)r * nc + corner] = which == 0 ? (a * c->S + r) * c->Bp + col0 : a * c->Bp;
        }
    ScratchBuf d_row, d_w, d_out;
    if ((rc = dev_upload(c, d_row, rowoff)) || (rc = dev_upload(c, d_w, g.w)) ||
        (rc = dev_alloc(c, d_out, (size_t)R * nB * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_morph_store, dim3((unsigned)((nB + kThreads - 1) / kThreads), (unsigned)R), dim3(kThreads), 0,
                       c->stream, which == 0 ? (const double*)c->ps.p : (const double*)c->nm.p,
                       (const int64_t*)d_row.p, (const double*)d_w.p, nc, nB, (double*)d_out.p,
                       // (an unbinned tensor scored on the device holds its events ordered by cell: back to the caller's order)
                       which == 0 && c->ev_sorted ? (const int32_t*)c->ev_perm.p : (const int32_t*)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out.p, (size_t)R * nB * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_interpolate: %s", hipGetErrorString(e));
    return BI_OK;
}

extern "C" {

int bi_interpolate(bi_ctx* c, int which, const double* z, double* out) { return interpolate_set(c, which, z, out, 0); }

int bi_eval_full(bi_ctx* c, const double* z, const double* rate_scale, int64_t dataset, double* ll, double* mus_out,
                 double* ps_out, int32_t* status) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!ll || !mus_out || !ps_out) return fail(c, BI_ERR_INVALID, "output pointers are NULL");
    if (c->bb_source >= 0 && !c->dense_counts) return fail(c, BI_ERR_STATE, "dataset counts are not resident in dense form");
    int32_t st = 0;
    rc = bi_eval(c, 1, z, rate_scale, &dataset, ll, &st);
    if (rc) return rc;
    if (status) *status = st;
    if (st & (BI_ST_OUT_OF_BOUNDS | BI_ST_UNPHYSICAL | BI_ST_BAD_DATASET)) return BI_OK;  // reference returns early
    PointGeom g;
    point_geometry(c, z, g);
    interp_mus(c, g, mus_out);
    if (rate_scale) for (int s = 0; s < c->S; ++s) mus_out[s] *= rate_scale[s];
    if ((rc = interpolate_set(c, 0, z, ps_out, dataset))) return rc;      // (several event sets: the N_dataset columns of that set)
    if (c->bb_source < 0) return BI_OK;
    // Beeston-Barlow adjusted (mus, pmfs) for full_output (likelihood.py:656-658), on the device.
    HIP_TRY(c, hipSetDevice(c->device));
    const int i = c->bb_source;
    const int64_t B = c->B;
    double Ntot = 0.0;
    for (size_t corner = 0; corner < g.w.size(); ++corner) {
        const double term = c->h_nm_tot[(size_t)(g.cell_anchor + corner_offset(c, (int)corner))] * g.w[corner];
        Ntot = Ntot + term;
    }
    if (c->bb_exact == 1 || (c->bb_exact == 2 && bb_zero_u_possible(c, g, mus_out))) {
        if ((rc = bb_exact_total(c, g, &Ntot))) return rc;     // as the evaluation above did
    }
    const double p_cal = mus_out[i] / Ntot;
    std::vector<double> a_row((size_t)B);
    if ((rc = bi_interpolate(c, 2, z, a_row.data()))) return rc;
    const int nblk = (int)std::min<int64_t>(1024, (B + kThreads - 1) / kThreads);
    ScratchBuf d_ps, d_a, d_mus, d_aw, d_part, d_tot;
    std::vector<double> mus_v(mus_out, mus_out + c->S);
    if ((rc = dev_alloc(c, d_ps, (size_t)c->S * B * sizeof(double))) || (rc = dev_upload(c, d_a, a_row)) ||
        (rc = dev_upload(c, d_mus, mus_v)) || (rc = dev_alloc(c, d_aw, (size_t)B * sizeof(double))) ||
        (rc = dev_alloc(c, d_part, (size_t)nblk * sizeof(double))) || (rc = dev_alloc(c, d_tot, sizeof(double)))) return rc;
    hipError_t e = hipMemcpyAsync(d_ps.p, ps_out, (size_t)c->S * B * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bb_full, dim3((unsigned)nblk), dim3(kThreads), 0, c->stream, (const double*)d_ps.p,
                           (const double*)d_a.p, (const double*)c->counts.p + dataset * c->Bp, (const double*)d_mus.p,
                           c->S, i, p_cal, Ntot, B, (double*)d_aw.p, (double*)d_part.p);
        hipLaunchKernelGGL(k_rows_sum, dim3(1), dim3(64), 0, c->stream, (const double*)d_part.p, nblk, (double*)d_tot.p,
                           (int64_t)1);
        hipLaunchKernelGGL(k_bb_normalise, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                           (const double*)d_aw.p, (const double*)d_tot.p, B, (double*)d_ps.p + (size_t)i * B);
        e = hipGetLastError();
    }
    double tot = 0.0;
    if (e == hipSuccess) e = hipMemcpyAsync(ps_out + (size_t)i * B, (double*)d_ps.p + (size_t)i * B, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&tot, d_tot.p, sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_eval_full: %s", hipGetErrorString(e));
    mus_out[i] = tot * p_cal;  // likelihood.py:658
    return BI_OK;
}

// ---- plain device buffers (gather staging for multi-GPU runs) -----------------------------------

int bi_device_alloc(bi_ctx* c, int64_t bytes, void** out) {
    if (!c || !out || bytes < 0) return BI_ERR_INVALID;
    *out = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(out, (size_t)std::max<int64_t>(bytes, 16));
    if (e != hipSuccess) {                       // the context's parked buffers (up to 4 GiB) go first
        drop_recycle_cache(c);
        e = hipMalloc(out, (size_t)std::max<int64_t>(bytes, 16));
    }
    if (e != hipSuccess) return fail(c, BI_ERR_NOMEM, "hipMalloc(%lld bytes) failed: %s", (long long)bytes, hipGetErrorString(e));
    c->user_allocs.push_back(*out);           // whatever is still alive goes with the context (bi_destroy)
    return BI_OK;
}

int bi_device_free(bi_ctx* c, void* p) {
    if (!c) return BI_ERR_INVALID;
    if (!p) return BI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    auto it = std::find(c->user_allocs.begin(), c->user_allocs.end(), p);
    if (it == c->user_allocs.end()) return fail(c, BI_ERR_INVALID, "bi_device_free: %p was not allocated by bi_device_alloc on this context", p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->user_allocs.erase(it);
    HIP_TRY(c, hipFree(p));
    return BI_OK;
}

// Copies of up to 4 MB between a device buffer and pageable host memory go through a pinned bounce buffer of the context:
// the runtime's own handling of pageable memory costs 15 ... 110 us per small copy (it varies from call to call), the
// bounce a DMA plus a memcpy -- the per-call gather of 10^4 toy results (80 KB) is such a copy.
constexpr int64_t kBounceBytes = (int64_t)4 << 20;

static int bounce_of(bi_ctx* c) {
    if (!c->bounce_host) HIP_TRY(c, hipHostMalloc(&c->bounce_host, (size_t)kBounceBytes, hipHostMallocDefault));
    return BI_OK;
}

int bi_memcpy_to_host(bi_ctx* c, void* dst, const void* src, int64_t bytes) {
    if (!c || bytes < 0 || (bytes > 0 && (!dst || !src))) return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (bytes > 0 && bytes <= kBounceBytes) {
        int rc = bounce_of(c);
        if (rc) return rc;
        if (bytes % 4 == 0 && ((uintptr_t)src & 3) == 0) {      // a kernel writing through the host mapping (see k_copy_words)
            const int64_t n_words = bytes / 4;
            hipLaunchKernelGGL(k_copy_words, dim3((unsigned)std::min<int64_t>(1024, (n_words + 255) / 256)), dim3(256), 0, c->stream,
                               (const uint32_t*)src, (uint32_t*)c->bounce_host, n_words);
            HIP_TRY(c, hipGetLastError());
        } else {
            HIP_TRY(c, hipMemcpyAsync(c->bounce_host, src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        memcpy(dst, c->bounce_host, (size_t)bytes);
        return BI_OK;
    }
    if (bytes) HIP_TRY(c, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

int bi_memcpy_to_device(bi_ctx* c, void* dst, const void* src, int64_t bytes) {
    if (!c || bytes < 0 || (bytes > 0 && (!dst || !src))) return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (bytes > 0 && bytes <= kBounceBytes) {
        int rc = bounce_of(c);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // an earlier copy out of the bounce buffer is complete
        memcpy(c->bounce_host, src, (size_t)bytes);
        HIP_TRY(c, hipMemcpyAsync(dst, c->bounce_host, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return BI_OK;
    }
    if (bytes) HIP_TRY(c, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

// ---- self-tests of device math ---------------------------------------------------------------

int bi_selftest_log(bi_ctx* c, int64_t n, const double* x, double* out) {
    if (!c || n < 0 || (n > 0 && (!x || !out))) return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    ScratchBuf dx, dy;
    int rc;
    if ((rc = dev_alloc(c, dx, (size_t)std::max<int64_t>(n, 1) * sizeof(double))) ||
        (rc = dev_alloc(c, dy, (size_t)std::max<int64_t>(n, 1) * sizeof(double)))) return rc;
    hipError_t e = n ? hipMemcpyAsync(dx.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(k_selftest_log, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double*)dx.p, n, (double*)dy.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n) e = hipMemcpyAsync(out, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_selftest_log: %s", hipGetErrorString(e));
    return BI_OK;
}

// the packed shadow of the template rows expanded back to doubles on the device: out_dev [anchors x sources][padded bins]
int bi_unpack_rows(bi_ctx* c, double* out_dev) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!out_dev) return fail(c, BI_ERR_INVALID, "bi_unpack_rows: out_dev is NULL");
    if (!c->pk_valid || !c->pk.p) return fail(c, BI_ERR_STATE, "bi_unpack_rows: the model has no packed rows (packed_rows_valid = 0)");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t n_chunks = c->A * c->S * (c->Bp / kTile), per_launch = (int64_t)1 << 30;
    for (int64_t q0 = 0; q0 < n_chunks; q0 += per_launch)
        hipLaunchKernelGGL(k_unpack_rows, dim3((unsigned)std::min(per_launch, n_chunks - q0)), dim3(kThreads), 0, c->stream,
                           (const uint8_t*)c->pk.p, (const uint32_t*)c->pk_base.p, q0, out_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BI_OK;
}

// the library's own device-wide primitives (tu_prim.hip) on caller data: kind of sort 0 (uint64 keys, int64 values), 1 (int64, int32),
// 2 (double, int32), 3 (the counting sort: uint64 keys below `end_bit` <= 1024, int64 values); kind of scan 0 inclusive max int64, 1 inclusive sum int64, 2 inclusive sum double, 3 exclusive sum int64 (+ init)
int bi_selftest_sort(bi_ctx* c, int kind, int64_t n, const void* keys, const void* vals, int begin_bit, int end_bit, void* keys_out, void* vals_out) {
    if (!c || n < 0 || kind < 0 || kind > 3 || begin_bit < 0 || end_bit > (kind == 3 ? 1024 : 64) || begin_bit > end_bit || (kind == 3 && end_bit < 1) ||
        (n > 0 && (!keys || !vals || !keys_out || !vals_out)))
        return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t vb = (kind == 0 || kind == 3) ? 8 : 4, nn = (size_t)std::max<int64_t>(n, 1);
    ScratchBuf dk, dv, dk2, dv2, dt;
    size_t tb = 0;
    if (kind == 0) (void)prim_sort_pairs(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n, 0u, 64u, c->stream);
    else if (kind == 3) (void)prim_count_sort_pairs(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n, (uint64_t)end_bit, c->stream);
    else if (kind == 1) (void)prim_sort_pairs(nullptr, tb, (const int64_t*)nullptr, (int64_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0u, 64u, c->stream);
    else (void)prim_sort_pairs(nullptr, tb, (const double*)nullptr, (double*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0u, 64u, c->stream);
    int rc;
    if ((rc = dev_alloc(c, dk, nn * 8)) || (rc = dev_alloc(c, dv, nn * vb)) || (rc = dev_alloc(c, dk2, nn * 8)) || (rc = dev_alloc(c, dv2, nn * vb)) ||
        (rc = dev_alloc(c, dt, std::max<size_t>(tb, 256)))) return rc;
    hipError_t e = n ? hipMemcpyAsync(dk.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess && n) e = hipMemcpyAsync(dv.p, vals, (size_t)n * vb, hipMemcpyHostToDevice, c->stream);
    size_t t2 = dt.bytes;
    if (e == hipSuccess) {
        if (kind == 0) e = prim_sort_pairs(dt.p, t2, (const uint64_t*)dk.p, (uint64_t*)dk2.p, (const int64_t*)dv.p, (int64_t*)dv2.p, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit, c->stream);
        else if (kind == 3) e = prim_count_sort_pairs(dt.p, t2, (const uint64_t*)dk.p, (uint64_t*)dk2.p, (const int64_t*)dv.p, (int64_t*)dv2.p, (size_t)n, (uint64_t)end_bit, c->stream);
        else if (kind == 1) e = prim_sort_pairs(dt.p, t2, (const int64_t*)dk.p, (int64_t*)dk2.p, (const int32_t*)dv.p, (int32_t*)dv2.p, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit, c->stream);
        else e = prim_sort_pairs(dt.p, t2, (const double*)dk.p, (double*)dk2.p, (const int32_t*)dv.p, (int32_t*)dv2.p, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit, c->stream);
    }
    if (e == hipSuccess && n) e = hipMemcpyAsync(keys_out, dk2.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(vals_out, dv2.p, (size_t)n * vb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_selftest_sort: %s", hipGetErrorString(e));
    return BI_OK;
}

int bi_selftest_scan(bi_ctx* c, int kind, int64_t n, const void* in, int64_t init, void* out) {
    if (!c || n < 0 || kind < 0 || kind > 3 || (n > 0 && (!in || !out))) return BI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    ScratchBuf di, dout, dt;
    size_t tb = 0;
    (void)prim_exclusive_scan_sum(nullptr, tb, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)n, c->stream);   // (all kinds: 8-byte elements, the same size)
    int rc;
    if ((rc = dev_alloc(c, di, nn * 8)) || (rc = dev_alloc(c, dout, nn * 8)) || (rc = dev_alloc(c, dt, std::max<size_t>(tb, 256)))) return rc;
    hipError_t e = n ? hipMemcpyAsync(di.p, in, (size_t)n * 8, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    size_t t2 = dt.bytes;
    if (e == hipSuccess) {
        if (kind == 0) e = prim_inclusive_scan_max(dt.p, t2, (const int64_t*)di.p, (int64_t*)dout.p, (size_t)n, c->stream);
        else if (kind == 1) e = prim_inclusive_scan_sum(dt.p, t2, (const int64_t*)di.p, (int64_t*)dout.p, (size_t)n, c->stream);
        else if (kind == 2) e = prim_inclusive_scan_sum(dt.p, t2, (const double*)di.p, (double*)dout.p, (size_t)n, c->stream);
        else e = prim_exclusive_scan_sum(dt.p, t2, (const int64_t*)di.p, (int64_t*)dout.p, init, (size_t)n, c->stream);
    }
    if (e == hipSuccess && n) e = hipMemcpyAsync(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); else (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_selftest_scan: %s", hipGetErrorString(e));
    return BI_OK;
}

// ---- measurement ---------------------------------------------------------------------------

int bi_measure_read_bandwidth(bi_ctx* c, int nontemporal, int blocks_per_cu, int reps, double* gb_per_s) {
    if (!c || !gb_per_s || reps < 1 || blocks_per_cu < 1) return BI_ERR_INVALID;
    if (!c->model_ready || !c->ps.p) return fail(c, BI_ERR_STATE, "bi_measure_read_bandwidth: no model resident");
    HIP_TRY(c, hipSetDevice(c->device));
    ScratchBuf sink;
    int rc = dev_alloc(c, sink, 8);
    if (rc) return rc;
    const int64_t n2 = c->A * c->S * c->Bp / 2;       // the whole template tensor, in 16-byte elements
    const dim3 grid((unsigned)(c->prop.multiProcessorCount * blocks_per_cu));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = 0.0;
    for (int r = 0; e == hipSuccess && r <= reps; ++r) {      // the first pass is the warm-up
        e = hipEventRecord(e0, c->stream);
        if (nontemporal) hipLaunchKernelGGL(k_read_sum<true>, grid, dim3(kThreads), 0, c->stream, (const double*)c->ps.p, n2, (double*)sink.p);
        else hipLaunchKernelGGL(k_read_sum<false>, grid, dim3(kThreads), 0, c->stream, (const double*)c->ps.p, n2, (double*)sink.p);
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && r > 0 && ms > 0.f) best = std::max(best, (double)n2 * 16.0 / (ms * 1e6));
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_measure_read_bandwidth: %s", hipGetErrorString(e));
    *gb_per_s = best;
    return BI_OK;
}

int bi_measure_stream_bandwidth(bi_ctx* c, int items, int rows, int nontemporal, int blocks_per_cu, int reps, double* gb_per_s) {
    if (!c || !gb_per_s || reps < 1 || blocks_per_cu < 1 || items < 1 || rows < 1) return BI_ERR_INVALID;
    if (!c->model_ready || !c->ps.p) return fail(c, BI_ERR_STATE, "bi_measure_stream_bandwidth: no model resident");
    HIP_TRY(c, hipSetDevice(c->device));
    ScratchBuf sink;
    int rc = dev_alloc(c, sink, 8);
    if (rc) return rc;
    const int64_t total_rows = c->A * c->S;
    // same launch shape as a batched morph launch: blocks_per_cu resident blocks per CU over all items; both the morph
    // kernel's own 512-bin tiles and (where the padded row length allows) 1024-bin tiles
    const int64_t slots = (int64_t)c->prop.multiProcessorCount * blocks_per_cu;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = 0.0;
    for (int pieces = 1; pieces <= 2; ++pieces) {
        if (c->Bp % (kTile * pieces)) continue;
        const int n_tiles = (int)(c->Bp / (kTile * pieces));
        const int nbx = (int)std::min<int64_t>(n_tiles, std::max<int64_t>(1, slots / items));
        const dim3 grid((unsigned)nbx, (unsigned)items);
        for (int r = 0; e == hipSuccess && r <= reps; ++r) {      // the first pass is the warm-up; every pass starts elsewhere
            const int64_t first = ((int64_t)r * items * rows * 7) % total_rows;
            e = hipEventRecord(e0, c->stream);
#define BI_ROWS(NTv, Pv) hipLaunchKernelGGL((k_read_rows<NTv, Pv>), grid, dim3(kThreads), 0, c->stream, (const double*)c->ps.p, c->Bp, total_rows, first, rows, n_tiles, (int)c->tile_chunks, (double*)sink.p)
            if (nontemporal) { if (pieces == 1) BI_ROWS(true, 1); else BI_ROWS(true, 2); }
            else { if (pieces == 1) BI_ROWS(false, 1); else BI_ROWS(false, 2); }
#undef BI_ROWS
            if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e == hipSuccess && r > 0 && ms > 0.f)
                best = std::max(best, (double)items * rows * (double)c->Bp * 8.0 / (ms * 1e6));
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_measure_stream_bandwidth: %s", hipGetErrorString(e));
    *gb_per_s = best;
    return BI_OK;
}

int bi_measure_copy_bandwidth(bi_ctx* c, int64_t bytes, int reps, double* gb_per_s) {
    if (!c || !gb_per_s || reps < 1 || bytes < 1) return BI_ERR_INVALID;
    if (!c->model_ready || !c->ps.p) return fail(c, BI_ERR_STATE, "bi_measure_copy_bandwidth: no model resident");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)std::min<int64_t>(bytes, c->A * c->S * c->Bp * (int64_t)sizeof(double));
    void* dst = nullptr;
    hipError_t e = hipMalloc(&dst, n);
    if (e != hipSuccess) return fail(c, BI_ERR_NOMEM, "bi_measure_copy_bandwidth: %s", hipGetErrorString(e));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = 0.0;
    for (int r = 0; e == hipSuccess && r <= reps; ++r) {      // the first pass is the warm-up
        e = hipEventRecord(e0, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst, c->ps.p, n, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && r > 0 && ms > 0.f) best = std::max(best, 2.0 * (double)n / (ms * 1e6));   // bytes read + bytes written
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(dst);
    if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_measure_copy_bandwidth: %s", hipGetErrorString(e));
    *gb_per_s = best;
    return BI_OK;
}

int bi_profile_enable(bi_ctx* c, int on) {
    if (!c) return BI_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->profiling = on != 0;
    c->ev_used = 0;
    c->prof_launches = 0;
    c->prof_ms = 0.0;
    return BI_OK;
}

int bi_profile_read(bi_ctx* c, int64_t* n_launches, double* total_ms) {
    if (!c) return BI_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, c->ev_pool[i].first, c->ev_pool[i].second));
        ms += t;
    }
    if (n_launches) *n_launches = (int64_t)c->ev_used;
    if (total_ms) *total_ms = ms;
    c->ev_used = 0;
    return BI_OK;
}

}  // extern "C"

#include "bi_varmap.h"
#include "bi_fit.h"
#include "bi_hess.h"
#include "bi_gof.h"
#include "bi_real.h"
#include "bi_factored.h"
#include "bi_factored_curv.h"
#include "bi_sourcewise.h"
#include "bi_sourcewise_real.h"
#include "bi_fisher.h"
#include "bi_sampler.h"
#include "bi_sourcewise_plan.h"
#include "bi_sourcewise_nonempty.h"
#include "bi_sourcewise_events.h"
#include "bi_sourcewise_sim.h"
#include "bi_sourcewise_scan.h"
#include "bi_grid.h"
#include "bi_coarse.h"
#include "bi_sourcewise_coarse.h"
