// Likelihood heads of the latent exact-GP models (gpmi_latent_gp_lp_grad): one row of F against the m replicate columns of Y.
// Included by small_kernels.hip (the one-workgroup kernel) and latent_kernels.hip (the chain's head kernel), so that both paths
// evaluate the same expression in the same order.  ocml's double exp / log1p; log sigma comes from the host (LatentHead).
#pragma once

// Row i: f0 = F[i, 0], f1 = F[i, 1] (NORMAL_LOGSD only); y: &Y[i, 0].  lik and dsig are the row's terms of out[0] and out[1],
// fb0 / fb1 its entries of Fbar.  The `~` constants are dropped.
//   NORMAL:          lik = -m log sigma - sum r^2 / (2 sigma^2), fb0 = sum r / sigma^2, dsig = -m / sigma + sum r^2 / sigma^3
//   BERNOULLI_LOGIT: lik = f sum y - m softplus(f), fb0 = sum y - m inv_logit(f), softplus(f) = max(f, 0) + log1p(exp(-|f|))
//   NORMAL_LOGSD:    lik = -m s - sum r^2 exp(-2 s) / 2, fb0 = sum r exp(-2 s), fb1 = sum r^2 exp(-2 s) - m   (mu = f0, s = f1)
__device__ __forceinline__ void latent_head_row(const LatentHead &h, double f0, double f1, const double *__restrict__ y, double &lik,
                                                double &dsig, double &fb0, double &fb1)
{
    const double md = (double)h.m;
    const bool bern = h.family == GPMI_LIK_BERNOULLI_LOGIT;
    const double off = bern ? 0.0 : f0;
    double s1 = 0.0, s2 = 0.0;   // sum of y - f0 (BERNOULLI: of y) and of its squares, columns in index order
    for (int c = 0; c < h.m; ++c) {
        const double r = y[(size_t)c * h.ldy] - off;
        s1 += r;
        s2 += r * r;
    }
    fb1 = 0.0;
    dsig = 0.0;
    if (h.family == GPMI_LIK_NORMAL) {
        const double is2 = 1.0 / (h.sigma * h.sigma);
        lik = -md * h.log_sigma - 0.5 * s2 * is2;
        fb0 = s1 * is2;
        dsig = -md / h.sigma + s2 * is2 / h.sigma;
        return;
    }
    const double e = exp(bern ? -fabs(f0) : -2.0 * f1);   // one exponential serves both heads
    if (bern) {
        const double sp = fmax(f0, 0.0) + log1p(e);
        const double pr = (f0 >= 0.0 ? 1.0 : e) / (1.0 + e);
        lik = s1 * f0 - md * sp;
        fb0 = s1 - md * pr;
    } else {
        lik = -md * f1 - 0.5 * s2 * e;
        fb0 = s1 * e;
        fb1 = s2 * e - md;
    }
}
