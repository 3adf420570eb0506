// bi_k_gof_terms.h -- gof_terms: the per-bin half-deviance and Pearson forms that k_morph_gof (bi_k_gof.h) and k_sourcewise_gof
// (bi_k_sourcewise.h) add up; the forms and their edge values are stated at the head of bi_k_gof.h.  Device code only.
#pragma once

namespace {

__device__ __forceinline__ void gof_terms(double n, double mu, double& dev, double& chi) {
    double d = mu, x = mu;
    if (n > 0.0) {
        d = (mu - n) - n * bin_log(mu / n);      // mu = 0: +inf
        const double r = n - mu;
        x = r * r / mu;
    }
    if (!(mu >= 0.0) || n != n) d = x = __builtin_nan("");
    else if (n < 0.0 || n != floor(n)) d = x = __builtin_inf();
    dev += d;
    chi += x;
}

}  // namespace
