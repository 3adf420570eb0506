// bi_factored_curv.h -- the second-order layers of a source-wise model (host half; the kernel is k_factored_curv,
// bi_k_factored_curv.h): bi_eval_sourcewise_hess (value, gradient and Hessian against the counts) and bi_eval_sourcewise_fisher
// (the expected information, no data).  Screen, descriptors, upload and the sub-batched launches are FacBatch's (bi_factored.h).
//
// theta = (z_0 .. z_{d-1}, rs_0 .. rs_{S-1}).  Source s is multilinear over its own axes, so d_q mu_b = sum_a C_qa u_a over the
// first-order basis u = (tau_s, ups_s,j) of the kernel, K = SC (1 + EM) columns, with the point's constants
//     C[rs_s, tau_s] = M_s          C[z_i, tau_s] += rs_s dM_s,j          C[z_i, ups_s,j] += rs_s M_s          (i = O_s[j])
// From the kernel's linear sums L (over f = n / mu - 1) and its Gram Q = sum_b (n / mu^2) u u^T
//     H = -C Q C^T   + (rs_s, z_i):   dM_s,j L_tau_s + M_s L_ups_s,j
//                    + (z_i, z_i):    2 rs_s dM_s,j L_ups_s,j
//                    + (z_i, z_k):    rs_s (d2M_s,jk L_tau_s + dM_s,j L_ups_s,k + dM_s,k L_ups_s,j + M_s L_chi_s,jk)      j < k
// each summed over the sources that own the axes, sources ascending, own axes ascending; and I = C Q' C^T with Q' = sum_{mu_b > 0}
// u u^T / mu_b.  The contractions run in long double on host threads (O(K^2 (d + S)) per point), one triangle, mirrored.
// An item's results: [linear slots of panel 0][the K (K + 1) / 2 Gram pairs, row-major lower triangle]; every panel is a
// launch of its own through FacBatch::run, which writes its rows' stretch of the triangle.
#pragma once

namespace {

// the launches of all Gram panels of one call; `lg0`: the slot constants of panel 0 (nullptr: zeros)
struct FacCurvPlan {
    int NL, NTRI, NTOT, panels, PS, W;
    std::vector<int> nsl, tri0;                 // per panel: result slots, first pair of the triangle
    std::vector<std::vector<int64_t>> perm;     // per panel [n][nsl]
    std::vector<double> lg0, zeros;

    FacCurvPlan(const FacBatch& b, bool fisher)
        : NL(factored_curv_linear(b.SC, b.EM, fisher)), NTRI(b.SC * b.W * (b.SC * b.W + 1) / 2), NTOT(NL + NTRI),
          panels(factored_curv_panels(b.SC, b.EM)), PS(factored_curv_panel_sources(b.SC, b.EM)), W(b.W) {
        const int64_t n = b.n_items;
        int most = 0;
        for (int p = 0; p < panels; ++p) {
            const int a0 = p * PS * W, a1 = (p + 1) * PS * W;
            tri0.push_back(a0 * (a0 + 1) / 2);
            nsl.push_back((p == 0 ? NL : 0) + a1 * (a1 + 1) / 2 - a0 * (a0 + 1) / 2);
            most = std::max(most, nsl.back());
            perm.emplace_back((size_t)(n * nsl.back()));
            for (int64_t i = 0; i < n; ++i)
                for (int q = 0; q < nsl.back(); ++q)
                    perm.back()[(size_t)(i * nsl.back() + q)] = i * NTOT + (p == 0 ? q : NL + tri0.back() + q);
        }
        lg0.assign((size_t)(n * nsl[0]), 0.0);
        zeros.assign((size_t)(n * most), 0.0);
    }

    int run(bi_ctx* c, FacBatch& b, bool fisher, const char* what) {
        std::vector<std::pair<const void*, size_t>> extra = {{lg0.data(), lg0.size() * sizeof(double)}, {zeros.data(), zeros.size() * sizeof(double)}};
        for (const auto& pm : perm) extra.push_back({pm.data(), pm.size() * sizeof(int64_t)});
        int rc = b.upload(extra, (size_t)b.n_items * NTOT);
        if (rc) return rc;
        for (int p = 0; p < panels; ++p) {
            if (b.events) {     // the event store (bi_eval_sourcewise_events_hess): the same panels over the items' event sets
                rc = b.run_events(nsl[(size_t)p], b.pu.dev<int64_t>(b.first_extra + 2 + p), b.pu.dev<double>(b.first_extra + (p == 0 ? 0 : 1)), what,
                                  [&](const SourcewiseEventsArgs& a, dim3 grid) {
                                      const int e = launch_sourcewise_events_curv(c, b.SC, b.EM, p, a, grid);
                                      return e ? fail(c, e, "%s: no kernel variant for %d source slots with %d own axes, panel %d", what, b.SC, b.EM, p)
                                               : BI_OK;
                                  });
                if (rc) return rc;
                continue;
            }
            rc = b.run(nsl[(size_t)p], b.pu.dev<int64_t>(b.first_extra + 2 + p), b.pu.dev<double>(b.first_extra + (p == 0 ? 0 : 1)), what,
                       [&](const FactoredArgs& a, dim3 grid) {
                           const int e = launch_factored_curv(c, b.SC, b.EM, fisher, p, a, grid);
                           return e ? fail(c, e, "%s: no kernel variant for %d source slots with %d own axes, panel %d", what, b.SC, b.EM, p) : BI_OK;
                       });
            if (rc) return rc;
        }
        return BI_OK;
    }
};

// C [F][K] of item i (zero rows for axes nobody owns)
void fac_curv_matrix(const FacBatch& b, int64_t i, const double* rate_scale, std::vector<long double>& C) {
    const int d = b.d, S = b.S, K = b.SC * b.W;
    const int64_t p = b.live[(size_t)i];
    std::fill(C.begin(), C.end(), 0.0L);
    for (int s = 0; s < S; ++s) {
        const double M = b.hM[(size_t)i * S + s], rs = rate_scale ? rate_scale[p * S + s] : 1.0;
        C[(size_t)(d + s) * K + s * b.W] = M;
        for (int j = 0; j < b.m.n_own[(size_t)s]; ++j) {
            const int ax = b.m.own[(size_t)s * kFacMaxOwn + j];
            C[(size_t)ax * K + s * b.W] += (long double)rs * b.hdM[((size_t)i * S + s) * kFacMaxOwn + j];
            C[(size_t)ax * K + s * b.W + 1 + j] += (long double)rs * M;
        }
    }
}

// out [F][F] = sign * C Q C^T for the lower triangle Q (row-major pairs a >= b), one triangle computed and mirrored; T [F][K] scratch
void fac_curv_contract(int F, int K, const std::vector<long double>& C, const double* tri, long double sign, std::vector<long double>& T,
                       std::vector<long double>& out) {
    for (int q = 0; q < F; ++q)
        for (int a = 0; a < K; ++a) {
            long double v = 0.0L;
            for (int b = 0; b < K; ++b) {
                const long double cq = C[(size_t)q * K + b];
                if (cq != 0.0L) v += cq * (long double)(a >= b ? tri[a * (a + 1) / 2 + b] : tri[b * (b + 1) / 2 + a]);
            }
            T[(size_t)q * K + a] = v;
        }
    for (int q = 0; q < F; ++q)
        for (int r = 0; r <= q; ++r) {
            long double v = 0.0L;
            for (int a = 0; a < K; ++a) {
                const long double cr = C[(size_t)r * K + a];
                if (cr != 0.0L) v += T[(size_t)q * K + a] * cr;
            }
            out[(size_t)q * F + r] = out[(size_t)r * F + q] = sign * v;
        }
}

// The observed Hessian of item i into hp [F][F]: H = -C Q C^T plus the (rs_s, z_i), (z_i, z_i) and (z_i, z_k) terms of the header,
// from the linear sums L (k_factored_curv's observed layout: L[1 + s] = L_tau_s, L[1 + SC + s EM + j] = L_ups_s,j,
// L[1 + K + s NX + x] = L_chi_s,x) and the Gram triangle tri.  What bi_eval_sourcewise_hess (L over f = n / mu - 1) and
// bi_eval_sourcewise_events_hess (L over g = 1 / lam, L_tau less 1) share; C, T [F][K] and H [F][F] are the caller's scratch.
void fac_curv_hessian(const FacBatch& b, int64_t i, const double* L, const double* tri, const double* rate_scale, std::vector<long double>& C,
                      std::vector<long double>& T, std::vector<long double>& H, double* hp) {
    const int d = b.d, S = b.S, F = d + S, K = b.SC * b.W, NXK = b.EM * (b.EM - 1) / 2;
    const int64_t p = b.live[(size_t)i];
    fac_curv_matrix(b, i, rate_scale, C);
    fac_curv_contract(F, K, C, tri, -1.0L, T, H);
    for (int s = 0; s < S; ++s) {
        const long double M = b.hM[(size_t)i * S + s], rs = rate_scale ? rate_scale[p * S + s] : 1.0, Lt = L[1 + s];
        const double* dM = &b.hdM[((size_t)i * S + s) * kFacMaxOwn];
        const double* d2M = &b.hd2M[((size_t)i * S + s) * kFacMaxOwn];
        const double* Lu = L + 1 + b.SC + s * b.EM;
        const double* Lx = L + 1 + K + s * NXK;
        const int* ax = &b.m.own[(size_t)s * kFacMaxOwn];
        for (int j = 0; j < b.m.n_own[(size_t)s]; ++j) {
            const long double v = (long double)dM[j] * Lt + M * (long double)Lu[j];
            H[(size_t)(d + s) * F + ax[j]] += v;
            H[(size_t)ax[j] * F + (d + s)] += v;
            H[(size_t)ax[j] * F + ax[j]] += 2.0L * rs * (long double)dM[j] * (long double)Lu[j];
            for (int k = j + 1; k < b.m.n_own[(size_t)s]; ++k) {
                const int x = k * (k - 1) / 2 + j;
                const long double w = rs * ((long double)d2M[x] * Lt + (long double)dM[j] * (long double)Lu[k] +
                                            (long double)dM[k] * (long double)Lu[j] + M * (long double)Lx[x]);
                H[(size_t)ax[j] * F + ax[k]] += w;
                H[(size_t)ax[k] * F + ax[j]] += w;
            }
        }
    }
    for (int q = 0; q < F; ++q)
        for (int r = 0; r <= q; ++r) hp[q * F + r] = hp[r * F + q] = (double)H[(size_t)q * F + r] + 0.0;
}

}  // namespace

extern "C" {

int bi_eval_sourcewise_hess(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, const int64_t* dataset, double* ll, double* grad,
                            double* hess, int32_t* status) {
    int rc = fac_check(c, "bi_eval_sourcewise_hess", true);
    if (rc) return rc;
    if (P < 0 || (P > 0 && (!ll || !grad || !hess))) return fail(c, BI_ERR_INVALID, "bi_eval_sourcewise_hess: bad P / output pointer");
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "bi_eval_sourcewise_hess: z is NULL");
    if (P == 0) return BI_OK;
    FacBatch b(c, 2);
    const int d = b.d, S = b.S, F = d + S, K = b.SC * b.W;
    const double inf = std::numeric_limits<double>::infinity();
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    b.screen(P, z, rate_scale, dataset, status, [&](int64_t p) {
        ll[p] = -inf;
        for (int j = 0; j < F; ++j) grad[p * F + j] = qnan;
        for (int j = 0; j < F * F; ++j) hess[p * F * F + j] = qnan;
    });
    if (b.n_items == 0) return BI_OK;
    b.fill(z, rate_scale, dataset);
    FacCurvPlan plan(b, false);
    for (int64_t i = 0; i < b.n_items; ++i) plan.lg0[(size_t)(i * plan.nsl[0])] = b.m.h_lgsum[(size_t)(dataset ? dataset[b.live[(size_t)i]] : 0)];
    if ((rc = plan.run(c, b, false, "bi_eval_sourcewise_hess"))) return rc;

    const double* out = b.out();
    parallel_for(b.n_items, 256, [&](int64_t lo, int64_t hi) {
        std::vector<double> gz((size_t)std::max(d, 1));
        std::vector<long double> C((size_t)F * K), T((size_t)F * K), H((size_t)F * F);
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = b.live[(size_t)i];
            const double* h = out + (size_t)i * plan.NTOT;
            ll[p] = h[0];
            if (!std::isfinite(h[0])) continue;             // gradient and Hessian stay nan
            b.gradient(i, h, rate_scale, grad + p * F, gz);
            fac_curv_hessian(b, i, h, h + plan.NL, rate_scale, C, T, H, hess + p * F * F);
        }
    });
    return BI_OK;
}

int bi_eval_sourcewise_fisher(bi_ctx* c, int64_t P, const double* z, const double* rate_scale, double* info, double* total, int64_t* unbounded,
                              int32_t* status) {
    int rc = fac_check(c, "bi_eval_sourcewise_fisher", false);
    if (rc) return rc;
    if (P < 0 || (P > 0 && !info)) return fail(c, BI_ERR_INVALID, "bi_eval_sourcewise_fisher: bad P / output pointer");
    if (c->fac.d > 0 && P > 0 && !z) return fail(c, BI_ERR_INVALID, "bi_eval_sourcewise_fisher: z is NULL");
    if (P == 0) return BI_OK;
    FacBatch b(c, 3);
    const int d = b.d, S = b.S, F = d + S, K = b.SC * b.W;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipSetDevice(c->device));
    b.screen(P, z, rate_scale, nullptr, status, [&](int64_t p) {
        for (int j = 0; j < F * F; ++j) info[p * F * F + j] = qnan;
        if (total) total[p] = qnan;
        for (int j = 0; unbounded && j < F; ++j) unbounded[p * F + j] = 0;
    });
    if (b.n_items == 0) return BI_OK;
    b.fill(z, rate_scale, nullptr);
    FacCurvPlan plan(b, true);
    if ((rc = plan.run(c, b, true, "bi_eval_sourcewise_fisher"))) return rc;

    // the slot that counts for axis i: the first slot (s, j) of that axis, as FacBatch::run marks it for the kernel
    std::vector<int> lead((size_t)std::max(d, 1), -1);
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < b.m.n_own[(size_t)s]; ++j) {
            const int ax = b.m.own[(size_t)s * kFacMaxOwn + j];
            if (lead[(size_t)ax] < 0) lead[(size_t)ax] = 1 + b.SC + s * b.EM + j;
        }
    const double* out = b.out();
    parallel_for(b.n_items, 256, [&](int64_t lo, int64_t hi) {
        std::vector<long double> C((size_t)F * K), T((size_t)F * K), I((size_t)F * F);
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = b.live[(size_t)i];
            const double* h = out + (size_t)i * plan.NTOT;
            if (total) total[p] = h[0];
            for (int q = 0; unbounded && q < F; ++q) {
                const int slot = q < d ? lead[(size_t)q] : 1 + (q - d);
                unbounded[p * F + q] = slot < 0 ? 0 : (int64_t)h[slot];
            }
            if (!(h[0] >= 0.0)) continue;        // a negative or nan expectation in some bin: the matrix stays nan
            fac_curv_matrix(b, i, rate_scale, C);
            fac_curv_contract(F, K, C, h + plan.NL, 1.0L, T, I);
            double* ip = info + p * F * F;
            for (int j = 0; j < F * F; ++j) ip[j] = (double)I[(size_t)j] + 0.0;
        }
    });
    return BI_OK;
}

}  // extern "C"
