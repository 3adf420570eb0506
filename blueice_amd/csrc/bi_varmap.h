// bi_varmap.h -- the host side of the free-variable map (VarMap and varmap_write_point, bi_dev_common.h) that the native fit
// (bi_fit.h, bi_real.h), sampler (bi_sampler.h) and grid (bi_grid.h) loops share: its argument checks, each reporting under
// the caller's name, and ResidentPoints, which keeps the map and the staged points on the device and has them evaluated
// where they lie.  A plan reused across the calls of ResidentPoints::evaluate would land here.
#pragma once

namespace {

template <class T>
std::vector<T> host_copy(const T* p, size_t n, T fill) {
    return p ? std::vector<T>(p, p + n) : std::vector<T>(n, fill);
}

// variable j is a shape parameter or a rate multiplier of this model (distinct: and none of the variables before it); d, S:
// the model's axes and sources (< 0: the grid model's; the source-wise model has its own, bi_factored.h)
int check_variable(bi_ctx* c, const char* who, int j, const int32_t* var_kind, const int32_t* var_index, bool distinct, int d = -1, int S = -1) {
    if (d < 0) d = c->d;
    if (S < 0) S = c->S;
    if ((var_kind[j] == 0 && (var_index[j] < 0 || var_index[j] >= d)) || (var_kind[j] == 1 && (var_index[j] < 0 || var_index[j] >= S)) ||
        (var_kind[j] != 0 && var_kind[j] != 1))
        return fail(c, BI_ERR_INVALID, "%s: variable %d is neither a shape parameter nor a rate multiplier of this model", who, j);
    for (int i = 0; distinct && i < j; ++i)
        if (var_kind[i] == var_kind[j] && var_index[i] == var_index[j])
            return fail(c, BI_ERR_INVALID, "%s: variables %d and %d are the same parameter", who, i, j);
    return BI_OK;
}

int check_var_map(bi_ctx* c, const char* who, int F, const int32_t* var_kind, const int32_t* var_index, int d = -1, int S = -1) {
    int rc = BI_OK;
    for (int j = 0; j < F && !rc; ++j) rc = check_variable(c, who, j, var_kind, var_index, false, d, S);
    return rc;
}

// a context with several event sets takes one entry, of set 0; entries: what the caller calls its entries
int check_single_set(bi_ctx* c, const char* who, const char* entries, int64_t E, const int64_t* dataset) {
    if (!(multi_set(c) && (E > 1 || (dataset && dataset[0] != 0)))) return BI_OK;
    char what[128];
    snprintf(what, sizeof what, "%s with more than one %s, or with another set than 0,", who, entries);
    return refuse_sets(c, what);
}

// every entry's dataset (NULL: 0) lies in [0, T); what: the caller's word for an entry, NULL: the real-valued store's sentence
int check_entry_datasets(bi_ctx* c, const char* who, const char* what, int64_t E, const int64_t* dataset, int64_t T) {
    for (int64_t e = 0; dataset && e < E; ++e)
        if (dataset[e] < 0 || dataset[e] >= T)
            return what ? fail(c, BI_ERR_INVALID, "%s: dataset %lld of %s %lld outside [0, %lld)", who, (long long)dataset[e], what, (long long)e, (long long)T)
                        : fail(c, BI_ERR_INVALID, "%s: dataset[%lld] = %lld outside the %lld real-valued sets", who, (long long)e, (long long)dataset[e], (long long)T);
    return BI_OK;
}

// The device side of a loop over staged points: the map of E entries and the rows of up to n_max points, freed with the scope.
struct ResidentPoints {
    ScratchBuf map, zp, rsp, dsp, llp;

    // the map in one copy (the caller waits for the stream before its arrays go), room for n_max points, m pointed at both;
    // model_d, model_S: the model's axes and sources as check_variable takes them (< 0: the grid model's)
    int bind(bi_ctx* c, VarMap& m, int64_t E, int64_t n_max, int F, const int32_t* var_kind, const int32_t* var_index, const double* z0,
             const double* scale0, const double* unit, const int64_t* dataset, int model_d = -1, int model_S = -1) {
        if (model_d < 0) model_d = c->d;
        if (model_S < 0) model_S = c->S;
        const size_t nE = (size_t)E, n = (size_t)n_max, d = (size_t)model_d, S = (size_t)model_S;
        PackedUpload pu;
        int rc;
        if ((rc = packed_upload(c, {{var_kind, (size_t)F * sizeof(int32_t)}, {var_index, (size_t)F * sizeof(int32_t)}, {z0, nE * d * sizeof(double)},
                                    {scale0, nE * S * sizeof(double)}, {unit, nE * S * sizeof(double)}, {dataset, dataset ? nE * sizeof(int64_t) : 0}},
                                0, pu, &map)) ||
            (rc = dev_alloc(c, zp, n * std::max<size_t>(d, 1) * sizeof(double))) || (rc = dev_alloc(c, rsp, n * S * sizeof(double))) ||
            (rc = dev_alloc(c, dsp, n * sizeof(int64_t))) || (rc = dev_alloc(c, llp, n * sizeof(double))))
            return rc;
        m.F = F; m.d = model_d; m.S = model_S;
        m.var_kind = pu.dev<int32_t>(0); m.var_index = pu.dev<int32_t>(1);
        m.z0 = pu.dev<double>(2); m.scale0 = pu.dev<double>(3); m.unit = pu.dev<double>(4);
        m.dataset = dataset ? pu.dev<int64_t>(5) : nullptr;
        m.z_dev = (double*)zp.p; m.rs_dev = (double*)rsp.p; m.ds_dev = (int64_t*)dsp.p;
        return BI_OK;
    }

    // plan and evaluate the first n staged points into llp; the plan is handed back for its status words (destroyed on failure)
    int evaluate(bi_ctx* c, int64_t n, const char* who, bi_plan** plan, int64_t* counters) {
        int rc = plan_points_resident_impl(c, n, c->d > 0 ? (const double*)zp.p : nullptr, (const double*)rsp.p, (const int64_t*)dsp.p, 0, 1, plan,
                                           false);
        if (rc) return rc;
        int32_t any = 0;
        if (!(rc = bi_run_plan(c, *plan, (double*)llp.p)) && !(rc = bi_plan_status(c, *plan, &any))) {
            if (counters) { counters[1] += n; counters[3] += bi_plan_launches(*plan); }
            if (!(any & BI_ST_INTERNAL)) return BI_OK;
        }
        bi_plan_destroy(c, *plan);
        *plan = nullptr;
        return rc ? rc : fail(c, BI_ERR_HIP, "%s: the device gave up waiting for a partial sum (in-launch reduction): GPU fault", who);
    }
};

}  // namespace
