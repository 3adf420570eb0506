// bi_sourcewise_coarse.h -- coarse views of a source-wise model (host half; the kernels are k_sourcewise_coarse,
// bi_k_sourcewise_coarse.h, and k_sourcewise_coarse_jac, bi_k_sourcewise_coarse_jac.h): bi_sourcewise_set_coarse_binning,
// bi_sourcewise_expected_coarse, bi_sourcewise_expected_coarse_jacobian, bi_sourcewise_coarse_counts.
//
// The binning is a second bi_ctx::Coarse (c->sw_coarse) over the B bins of the source-wise store, built by bi_coarse.h's
// coarse_build and released by bi_factored_begin; the grid model's binning and its entry points do not see it.  The launch
// geometry, the chunks of points and the finish kernels are bi_coarse.h's too.  The expectation's descriptors are FacBatch's of
// order 0 (bi_factored.h), as bi_sourcewise_expected_counts uploads them; the dense counts [T][Bp] of the store -- uploaded or
// drawn on the device -- go through k_morph_coarse itself with NS = 1, a_0 = 1 and the counts row as the "template".
//
// bi_sourcewise_expected_coarse_jacobian: mu_C and d mu_C / d theta, theta = (z, then rate scales) as bi_eval_factored's gradient.
// The descriptors are FacBatch's of order 1; k_sourcewise_coarse_jac (bi_k_sourcewise_coarse_jac.h) sums per cell mu_b, the basis
// columns tau_s,b -> T_s and ups_s,j,b -> Y_s,j, the K = 1 + S + sum_s e_s live ones as the groups of an R = K call; a chunk's
// [item][K][C] comes down as one run and the host contracts it per cell in long double with M_s, dM_s,j (FacBatch::hM / hdM):
//     x_s,d+s   = M_s T_s                                      d mu_C / d rs_s
//     x_s,i     = rs_s (M_s Y_s,j + dM_s,j T_s)                i = own_s[j]: the term of source s in d mu_C / d z_i
// each rounded to a double once.  per_source: mu_s,C = r_s T_s (r_s as FacBatch::rates holds it; r Sum, where
// bi_sourcewise_expected_coarse's per-source form is Sum r: equal to rounding, not to the bit) and the rows of source s are its
// own x_s,. -- every entry of another source's scale or of an axis s does not own is exactly 0.0.  The total rows are the x_s,.
// added over s in ascending order in long double from 0.0 and rounded once, so THE PER-SOURCE ROWS, SUMMED OVER s IN ASCENDING
// ORDER IN LONG DOUBLE, REPRODUCE THE TOTAL ROWS BIT FOR BIT; an axis nobody owns has a row of exactly 0.0.  The total mu_C is the
// kernel's slot 0, untouched: bi_sourcewise_expected_coarse's bits.  No column limit beyond the model's own (d <= 32, S <= 8,
// e_s <= 3): d enters the host contraction alone.
#pragma once

namespace {

int sw_coarse_check(bi_ctx* c, const char* who, bool need_counts) {
    int rc = fac_check(c, who, need_counts);
    if (rc) return rc;
    if (!c->sw_coarse.set)
        return fail(c, BI_ERR_STATE, "%s: no coarse binning is set (bi_sourcewise_set_coarse_binning first; a new model releases it)", who);
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_sourcewise_set_coarse_binning(bi_ctx* c, int k, const int32_t* n_fine, const int32_t* n_groups, const int32_t* bounds, int64_t* n_cells) {
    const char* who = "bi_sourcewise_set_coarse_binning";
    if (!c) return BI_ERR_INVALID;
    if (n_cells) *n_cells = 0;
    if (k == 0) {
        if (c->pending) return fail(c, BI_ERR_STATE, "a bi_eval_begin is outstanding on this context: call bi_eval_end first");
        HIP_TRY(c, hipSetDevice(c->device));
        release_coarse(c->sw_coarse);
        return BI_OK;
    }
    int rc = fac_check(c, who, false);
    if (rc) return rc;
    return coarse_build(c, c->sw_coarse, who, c->fac.B, k, n_fine, n_groups, bounds, n_cells);
}

int bi_sourcewise_expected_coarse(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int per_source, double* out, int32_t* status) {
    const char* who = "bi_sourcewise_expected_coarse";
    int rc = sw_coarse_check(c, who, false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !out)) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointer", who);
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (P == 0) return BI_OK;
    const bi_ctx::Coarse& q = c->sw_coarse;
    FacBatch b(c, 0, false);
    const int R = per_source ? b.S : 1;
    const int64_t per_item = (int64_t)R * q.C;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    // the screen of bi_sourcewise_expected_counts (no dataset test); here the bit is reported too
    b.screen(P, z, rate_scale, nullptr, status, [&](int64_t p) { std::fill(out + p * per_item, out + (p + 1) * per_item, qnan); });
    const int64_t n_items = b.n_items;
    if (n_items == 0) return BI_OK;
    b.fill(z, rate_scale, nullptr);
    if ((rc = b.upload({}, 0))) return rc;
    const int64_t chunk = coarse_chunk(c, q, n_items, R);
    const CoarseGeometry geo = coarse_geometry(c, q);
    ScratchBuf d_partial, d_out;
    if ((rc = dev_alloc(c, d_partial, (size_t)(chunk * R * q.CR * geo.nsplit * q.Lx) * sizeof(double))) ||
        (rc = dev_alloc(c, d_out, (size_t)(chunk * per_item) * sizeof(double)))) return rc;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        SourcewiseCoarseArgs a{};
        a.f = b.args();
        b.point_at(a.f, i0);
        a.g = coarse_args(c, q, nullptr, nullptr, nullptr, 0, b.S, R, ni, (double*)d_partial.p, (double*)d_out.p);
        if (launch_sourcewise_coarse(c, b.SC, b.EM, per_source != 0, a, ni)) {
            (void)hipStreamSynchronize(c->stream);
            return fail(c, BI_ERR_INVALID, "%s: no kernel variant for %d source slots with %d own axes", who, b.SC, b.EM);
        }
        ++c->last_point_pieces;
        // (d_partial and d_out are reused by the next chunk: the download synchronises)
        const hipError_t e = download_live_runs(c, &b.live[(size_t)i0], ni, (const double*)d_out.p, per_item, out, hipGetLastError());
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return BI_OK;
}

int bi_sourcewise_expected_coarse_jacobian(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, int per_source, double* mu,
                                           double* jac, int32_t* status) {
    const char* who = "bi_sourcewise_expected_coarse_jacobian";
    int rc = sw_coarse_check(c, who, false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!mu || !jac))) return fail(c, BI_ERR_INVALID, "%s: bad P / output pointer", who);
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "%s: z is NULL", who);
    if (P == 0) return BI_OK;
    const bi_ctx::Coarse& q = c->sw_coarse;
    FacBatch b(c, 1, false);
    const bi_ctx::Factored& m = b.m;
    const int d = b.d, S = b.S, SC = b.SC, EM = b.EM, F = d + S, R = per_source ? S : 1;
    const int64_t C = q.C;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    b.screen(P, z, rate_scale, nullptr, status, [&](int64_t p) {
        std::fill(mu + p * R * C, mu + (p + 1) * R * C, qnan);
        std::fill(jac + p * R * F * C, jac + (p + 1) * R * F * C, qnan);
    });
    const int64_t n_items = b.n_items;
    if (n_items == 0) return BI_OK;
    b.fill(z, rate_scale, nullptr);
    if ((rc = b.upload({}, 0))) return rc;

    // k_morph_factored's slots -> the K live groups: mu, T_s (s < S), then Y_s,j (s < S ascending, j < e_s ascending)
    SourcewiseCoarseJacArgs a{};
    std::fill(a.group, a.group + kCoarseJacSlots, (signed char)-1);
    int K = 0;
    a.group[0] = (signed char)K++;
    for (int s = 0; s < S; ++s) a.group[1 + s] = (signed char)K++;
    int gY[kFacMaxSources][kFacMaxOwn];
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < m.n_own[(size_t)s]; ++j) a.group[1 + SC + s * EM + j] = (signed char)(gY[s][j] = K++);

    const int64_t chunk = coarse_chunk(c, q, n_items, K);
    const CoarseGeometry geo = coarse_geometry(c, q);
    ScratchBuf d_partial, d_out;
    if ((rc = dev_alloc(c, d_partial, (size_t)(chunk * K * q.CR * geo.nsplit * q.Lx) * sizeof(double))) ||
        (rc = dev_alloc(c, d_out, (size_t)(chunk * K * C) * sizeof(double)))) return rc;
    // The device holds a chunk's cells as [item][K][C]; it comes down as one run and is contracted here.
    std::vector<double> stage((size_t)(chunk * K * C));
    std::vector<int64_t> run((size_t)chunk);
    for (int64_t i = 0; i < chunk; ++i) run[(size_t)i] = i;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t ni = std::min(chunk, n_items - i0);
        a.f = b.args();
        b.point_at(a.f, i0);
        a.g = coarse_args(c, q, nullptr, nullptr, nullptr, 0, S, K, ni, (double*)d_partial.p, (double*)d_out.p);
        if (launch_sourcewise_coarse_jac(c, SC, EM, a, ni)) {
            (void)hipStreamSynchronize(c->stream);
            return fail(c, BI_ERR_INVALID, "%s: no kernel variant for %d source slots with %d own axes", who, SC, EM);
        }
        ++c->last_point_pieces;
        // (d_partial and d_out are reused by the next chunk: the download synchronises)
        const hipError_t e = download_live_runs(c, run.data(), ni, (const double*)d_out.p, (int64_t)K * C, stage.data(), hipGetLastError());
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        // (a thread is worth starting for some 16 K entries of jac)
        parallel_for(ni, std::max<int64_t>(1, 16384 / ((int64_t)F * C)), [&](int64_t lo, int64_t hi) {
            std::vector<long double> acc((size_t)std::max<int64_t>(1, d * C));       // the total's rows over z, summed over the sources
            for (int64_t ii = lo; ii < hi; ++ii) {
                const int64_t i = i0 + ii, p = b.live[(size_t)i];
                const double* h = stage.data() + ii * K * C;
                double* mp = mu + p * R * C;
                double* jp = jac + p * R * F * C;
                std::fill(jp, jp + (int64_t)R * F * C, 0.0);
                std::fill(acc.begin(), acc.end(), 0.0L);
                if (!per_source) std::copy(h, h + C, mp);
                // sources ascending, own axes ascending within a source (FacBatch::gradient's order)
                for (int s = 0; s < S; ++s) {
                    const long double M = b.hM[(size_t)i * S + s];
                    const long double rs = rate_scale ? rate_scale[p * S + s] : 1.0;
                    const double r = b.rates[(size_t)i * SC + s];
                    const double* T = h + (int64_t)(1 + s) * C;
                    double* js = jp + (per_source ? (int64_t)s * F * C : 0);        // the block the rows of source s go to
                    if (per_source)
                        for (int64_t cc = 0; cc < C; ++cc) mp[s * C + cc] = r * T[cc];
                    // (one term per scale: 0.0 + x is the sum the header speaks of, -0.0 included)
                    for (int64_t cc = 0; cc < C; ++cc) js[(d + s) * C + cc] = 0.0 + (double)(M * (long double)T[cc]);
                    for (int j = 0; j < m.n_own[(size_t)s]; ++j) {
                        const int ax = m.own[(size_t)s * kFacMaxOwn + j];
                        const long double dM = b.hdM[((size_t)i * S + s) * kFacMaxOwn + j];
                        const double* Y = h + (int64_t)gY[s][j] * C;
                        for (int64_t cc = 0; cc < C; ++cc) {
                            const double x = (double)(rs * (M * (long double)Y[cc] + dM * (long double)T[cc]));
                            if (per_source) js[ax * C + cc] = x;
                            else acc[(size_t)(ax * C + cc)] += x;
                        }
                    }
                }
                if (!per_source)
                    for (int64_t t = 0; t < d * C; ++t) jp[t] = (double)acc[(size_t)t];
            }
        });
    }
    return BI_OK;
}

int bi_sourcewise_coarse_counts(bi_ctx* c, int64_t n, const int64_t* dataset, double* out) {
    const char* who = "bi_sourcewise_coarse_counts";
    int rc = sw_coarse_check(c, who, true);
    if (rc) return rc;
    const bi_ctx::Factored& m = c->fac;
    if (n < 0 || (n > 0 && !out)) return fail(c, BI_ERR_INVALID, "%s: bad n / output pointer", who);
    if (!dataset && n != m.T) return fail(c, BI_ERR_INVALID, "%s: without a dataset list n must be the %lld resident datasets (got %lld)", who, (long long)m.T, (long long)n);
    for (int64_t i = 0; dataset && i < n; ++i)
        if (dataset[i] < 0 || dataset[i] >= m.T)
            return fail(c, BI_ERR_INVALID, "%s: dataset %lld outside [0,%lld)", who, (long long)dataset[i], (long long)m.T);
    c->last_point_pieces = 0;
    if (n == 0) return BI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const bi_ctx::Coarse& q = c->sw_coarse;
    const int64_t chunk = coarse_chunk(c, q, n, 1);
    ScratchBuf d_partial, d_out;
    if ((rc = dev_alloc(c, d_out, (size_t)(chunk * q.C) * sizeof(double))) ||
        (rc = dev_alloc(c, d_partial, (size_t)(chunk * q.CR * coarse_geometry(c, q).nsplit * q.Lx) * sizeof(double)))) return rc;
    std::vector<int64_t> first((size_t)chunk);        // the element offset of the dataset's counts row
    const std::vector<double> ones((size_t)chunk, 1.0);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t ni = std::min(chunk, n - i0);
        for (int64_t i = 0; i < ni; ++i) first[(size_t)i] = (dataset ? dataset[i0 + i] : i0 + i) * m.Bp;
        PackedUpload pu;
        if ((rc = packed_upload(c, {{first.data(), (size_t)ni * sizeof(int64_t)}, {ones.data(), (size_t)ni * sizeof(double)}}, 0, pu))) return rc;
        coarse_launch(c, q, (const double*)m.counts.p, pu.dev<int64_t>(0), pu.dev<double>(1), 1, 1, 1, ni, (double*)d_partial.p, (double*)d_out.p);
        ++c->last_point_pieces;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + i0 * q.C, d_out.p, (size_t)(ni * q.C) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        else (void)hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return BI_OK;
}

}  // extern "C"
