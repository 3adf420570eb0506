// bi_sampler.h -- the host loop of the ensemble sampler (bi_sample_stretch): E independent ensembles of W walkers, the context's
// likelihood as the target density.  The points never leave the device: k_stretch_propose writes the proposals of the moving
// half into the layouts the resident planner reads, the planner and the evaluation kernels of bi_plan_points_resident /
// bi_run_plan take them where they lie, k_stretch_accept moves the walkers and appends to the chain in HBM, and chain, log
// likelihoods and counters are copied to the host once, at the end.  The variables' map, the proposals' rows and their
// evaluation are ResidentPoints' (bi_varmap.h), shared with bi_grid.h.  What a half-step still costs on the host is the
// planner's: it reads its counts back to size its launches (plan_report), the plan's status OR is a second read
// (bi_plan_status), the plan is made and destroyed (buffers from the context's recycle cache, one stream synchronisation)
// every half-step.  A plan reused across half-steps would remove most of that; its place is ResidentPoints::evaluate.  The
// source-wise model's loop (bi_sourcewise_plan.h) has none of it and shares the checks below (stretch_check_*).  (The
// reference's counterpart is emcee's loop of n_walkers x n_steps scalar likelihood calls, blueice/inference.py:254-321.)
#pragma once

namespace {

// what only the sampler keeps on the device
struct SamplerBuffers {
    ScratchBuf lo, hi, x, ll, nacc, chain, chain_ll, pmean, psigma, pconst;
};

// The argument checks of bi_sample_stretch_gauss and bi_sample_stretch_sourcewise (bi_sourcewise_plan.h), reported under `who`
// (`who_terms`: those about the constraint terms).  d, S: the sampled model's axes and sources (< 0: the grid model's, and the
// context's event sets are checked); T: its datasets.  A prior_sigma without a finite entry: the two arrays come back NULL.
int stretch_check_args(bi_ctx* c, const char* who, const char* who_terms, int d, int S, int64_t T, int64_t E, int W, int F, const int32_t* var_kind,
                       const int32_t* var_index, const double* z0, const double* scale0, const double* unit, const int64_t* dataset, const double* x0,
                       const double* lo, const double* hi, int64_t n_steps, double a, int64_t first_ensemble, const double*& prior_mean,
                       const double*& prior_sigma, const double* prior_const, const double* chain, const double* ll, const int64_t* n_accepted) {
    int rc;
    if (W < 2 || (W & 1)) return fail(c, BI_ERR_INVALID, "%s: the stretch move needs an even number of walkers >= 2 (got %d): the ensemble moves in two halves", who, W);
    if (F < 1) return fail(c, BI_ERR_INVALID, "%s: need F >= 1 variables (got %d)", who, F);
    if (!(a > 1.0) || !std::isfinite(a)) return fail(c, BI_ERR_INVALID, "%s: the stretch scale a must be > 1 (got %g)", who, a);
    if (E < 1 || n_steps < 0 || n_steps > (int64_t)1 << 31 || first_ensemble < 0 || first_ensemble + E > (int64_t)1 << 32 ||
        E * (int64_t)W > (int64_t)1 << 30)
        return fail(c, BI_ERR_INVALID, "%s: need E >= 1, E * W <= 2^30, 0 <= n_steps <= 2^31 and ensembles within [0, 2^32)", who);
    if (!var_kind || !var_index || !scale0 || !unit || ((d < 0 ? c->d : d) > 0 && !z0) || !x0 || !lo || !hi || !n_accepted ||
        (n_steps > 0 && (!chain || !ll)))
        return fail(c, BI_ERR_INVALID, "%s: NULL argument", who);
    if ((rc = check_var_map(c, who, F, var_kind, var_index, d, S)) || (d < 0 && (rc = check_single_set(c, who, "ensemble", E, dataset))) ||
        (rc = check_entry_datasets(c, who, "ensemble", E, dataset, T)))
        return rc;
    // the constraint terms: all three arrays NULL is bi_sample_stretch; otherwise mean and sigma are required
    if (prior_mean || prior_sigma || prior_const) {
        if (const char* why = gauss_terms_invalid(F, E, prior_mean, prior_sigma, prior_const)) return fail(c, BI_ERR_INVALID, "%s: %s", who_terms, why);
        // no finite sigma: no term on any variable, and the kernels are not handed the two arrays
        bool any = false;
        for (int j = 0; j < F; ++j) any |= std::isfinite(prior_sigma[j]);
        if (!any) prior_mean = prior_sigma = nullptr;
    }
    return BI_OK;
}

// the chain stays in HBM until the end: it has to fit there
int stretch_check_chain(bi_ctx* c, const char* who, int64_t n_steps, size_t nW, int F) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    const double need = (double)n_steps * (double)nW * (F + 1) * sizeof(double);
    if (need > (double)free_b + (double)c->cache_bytes)
        return fail(c, BI_ERR_NOMEM, "%s: the chain (%lld steps x %lld walkers x %d variables: %.3g bytes) is larger than the free "
                                     "device memory (%zu bytes): run fewer steps per call", who, (long long)n_steps, (long long)nW, F, need, free_b);
    return BI_OK;
}

// the start: every walker inside [lo, hi], its log density finite and its status word clean
int stretch_check_start(bi_ctx* c, const char* who, size_t nW, int W, int F, const std::vector<double>& h_x, const std::vector<double>& h_lo,
                        const std::vector<double>& h_hi, const std::vector<double>& h_ll, const std::vector<int32_t>& h_st, bool terms) {
    for (size_t w = 0; w < nW; ++w)
        for (int v = 0; v < F; ++v)
            if (!(h_x[w * F + v] >= h_lo[(size_t)v] && h_x[w * F + v] <= h_hi[(size_t)v]))
                return fail(c, BI_ERR_INVALID, "%s: start walker %lld of ensemble %lld lies outside [lo, hi] in variable %d (%g)", who,
                            (long long)(w % (size_t)W), (long long)(w / (size_t)W), v, h_x[w * F + v]);
    for (size_t w = 0; w < nW; ++w)
        if (!std::isfinite(h_ll[w]) || h_st[w] != 0)
            return fail(c, BI_ERR_INVALID, "%s: the log likelihood of start walker %lld of ensemble %lld is not finite "
                                           "(%g, status %d): every walker must start at a point of non-zero likelihood%s", who,
                        (long long)(w % (size_t)W), (long long)(w / (size_t)W), h_ll[w], (int)h_st[w],
                        terms ? " (constraint terms included)" : "");
    return BI_OK;
}

int sample_stretch(bi_ctx* c, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                   const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo, const double* hi,
                   int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble, const double* prior_mean, const double* prior_sigma,
                   const double* prior_const, double* chain, double* ll, int64_t* n_accepted, int64_t* counters) {
    const size_t nE = (size_t)E, nW = (size_t)E * W;
    SamplerBuffers b;
    ResidentPoints pts;
    StretchArgs s{};
    int rc;
    if ((rc = stretch_check_chain(c, "bi_sample_stretch", n_steps, nW, F))) return rc;
    // (host copies that live until the uploads have been waited for)
    const std::vector<double> h_lo = host_copy(lo, (size_t)F, 0.0), h_hi = host_copy(hi, (size_t)F, 0.0), h_x = host_copy(x0, nW * F, 0.0);
    if ((rc = pts.bind(c, s, E, (int64_t)nW, F, var_kind, var_index, z0, scale0, unit, dataset)) || (rc = dev_upload(c, b.lo, h_lo)) ||
        (rc = dev_upload(c, b.hi, h_hi)) || (rc = dev_upload(c, b.x, h_x)))
        return rc;
    // Gaussian constraint terms (prior_sigma NULL here: none on any variable)
    const std::vector<double> h_pmean = host_copy(prior_sigma ? prior_mean : nullptr, (size_t)F, 0.0),
                              h_psigma = host_copy(prior_sigma, (size_t)F, std::numeric_limits<double>::infinity()),
                              h_pconst = host_copy(prior_const, nE, 0.0);
    const bool terms = prior_sigma || prior_const;
    if (prior_sigma && ((rc = dev_upload(c, b.pmean, h_pmean)) || (rc = dev_upload(c, b.psigma, h_psigma)))) return rc;
    if (prior_const && (rc = dev_upload(c, b.pconst, h_pconst))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t steps = (size_t)n_steps;
    if ((rc = dev_alloc(c, b.ll, nW * sizeof(double))) || (rc = dev_alloc(c, b.nacc, nW * sizeof(int64_t))) ||
        (rc = dev_alloc(c, b.chain, std::max<size_t>(steps, 1) * nW * F * sizeof(double))) ||
        (rc = dev_alloc(c, b.chain_ll, std::max<size_t>(steps, 1) * nW * sizeof(double))))
        return rc;
    HIP_TRY(c, hipMemsetAsync(b.nacc.p, 0, nW * sizeof(int64_t), c->stream));
    s.E = E; s.W = W;
    s.first_ensemble = first_ensemble;
    s.k0 = (uint32_t)seed; s.k1 = (uint32_t)(seed >> 32);
    s.a = a;
    s.lo = (const double*)b.lo.p; s.hi = (const double*)b.hi.p;
    s.x = (double*)b.x.p; s.ll = (double*)b.ll.p; s.n_accepted = (int64_t*)b.nacc.p;
    s.ll_prop = (const double*)pts.llp.p;
    s.prior_mean = prior_sigma ? (const double*)b.pmean.p : nullptr;
    s.prior_sigma = prior_sigma ? (const double*)b.psigma.p : nullptr;
    s.prior_const = prior_const ? (const double*)b.pconst.p : nullptr;
    if (counters) counters[0] = counters[1] = counters[2] = counters[3] = 0;

    // the start: every walker's own log density (the log likelihood, plus the constraint terms if there are any), which must be finite
    bi_plan* plan = nullptr;
    s.h = -1;
    launch_stretch_propose(c, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = pts.evaluate(c, (int64_t)nW, "bi_sample_stretch", &plan, counters))) return rc;
    {
        std::vector<double> h_ll(nW);
        std::vector<int32_t> h_st(nW);
        hipError_t e = hipSuccess;
        if (terms) {
            launch_stretch_start_density(c, s);                 // b.ll = b.llp + p
            e = hipGetLastError();
        } else
            e = hipMemcpyAsync(b.ll.p, pts.llp.p, nW * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_ll.data(), b.ll.p, nW * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_st.data(), plan->status.p, nW * sizeof(int32_t), hipMemcpyDefault, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        bi_plan_destroy(c, plan);
        plan = nullptr;
        if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_sample_stretch (start): %s", hipGetErrorString(e));
        if ((rc = stretch_check_start(c, "bi_sample_stretch", nW, W, F, h_x, h_lo, h_hi, h_ll, h_st, terms))) return rc;
    }

    const int64_t n = E * (W / 2);
    for (int64_t t = 0; t < n_steps; ++t)
        for (int h = 0; h < 2; ++h) {
            s.t = t; s.h = h;
            s.chain = (double*)b.chain.p + (size_t)t * nW * F;
            s.chain_ll = (double*)b.chain_ll.p + (size_t)t * nW;
            launch_stretch_propose(c, s);
            HIP_TRY(c, hipGetLastError());                      // (nothing is launched after a failed launch)
            if ((rc = pts.evaluate(c, n, "bi_sample_stretch", &plan, counters))) return rc;
            s.st_prop = (const int32_t*)plan->status.p;
            launch_stretch_accept(c, s);
            const hipError_t e = hipGetLastError();
            bi_plan_destroy(c, plan);                           // (waits for the stream: the accept kernel reads the plan's status words)
            plan = nullptr;
            if (e != hipSuccess) return fail(c, BI_ERR_HIP, "bi_sample_stretch (accept): %s", hipGetErrorString(e));
            ++c->n_sampler_half_steps;
            if (counters) ++counters[0];
        }
    // one copy of chain, log likelihoods and acceptance counters at the end of the call
    if (n_steps > 0) {
        HIP_TRY(c, hipMemcpyAsync(chain, b.chain.p, steps * nW * F * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(ll, b.chain_ll.p, steps * nW * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(n_accepted, b.nacc.p, nW * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (counters)
        for (size_t w = 0; w < nW; ++w) counters[2] += n_accepted[w];
    return BI_OK;
}

}  // namespace

extern "C" {

int bi_sample_stretch_gauss(bi_ctx* c, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index,
                            const double* z0, const double* scale0, const double* unit, const int64_t* dataset, const double* x0,
                            const double* lo, const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble,
                            const double* prior_mean, const double* prior_sigma, const double* prior_const, double* chain,
                            double* ll, int64_t* n_accepted, int64_t* counters) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    c->plan_refused = 0;
    if ((rc = stretch_check_args(c, "bi_sample_stretch", "bi_sample_stretch_gauss", -1, -1, c->T, E, W, F, var_kind, var_index, z0, scale0, unit, dataset,
                                 x0, lo, hi, n_steps, a, first_ensemble, prior_mean, prior_sigma, prior_const, chain, ll, n_accepted)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    try {
        return sample_stretch(c, E, W, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a, seed, first_ensemble, prior_mean,
                              prior_sigma, prior_const, chain, ll, n_accepted, counters);
    } catch (const std::bad_alloc&) {
        return fail(c, BI_ERR_NOMEM, "bi_sample_stretch: out of host memory");
    }
}

int bi_sample_stretch(bi_ctx* c, int64_t E, int W, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
                      const double* scale0, const double* unit, const int64_t* dataset, const double* x0, const double* lo,
                      const double* hi, int64_t n_steps, double a, uint64_t seed, int64_t first_ensemble, double* chain, double* ll,
                      int64_t* n_accepted, int64_t* counters) {
    return bi_sample_stretch_gauss(c, E, W, F, var_kind, var_index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a, seed, first_ensemble, nullptr,
                                   nullptr, nullptr, chain, ll, n_accepted, counters);
}

}  // extern "C"
