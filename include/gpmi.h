/*
 * gpmi.h -- C ABI of libgpmi: the MI355X (gfx950) implementation of the exact-GP
 * marginal-likelihood hot path of bbbales2/gp.
 *
 * This is the drop-in boundary: what an R `.Call()` shim (r/gpmi_shim.c), an
 * Rcpp replacement of covariance.cpp, or any FFI binds.  Plain pointers and
 * sizes only; no C++ / torch types.  Reference interfaces replaced are cited
 * per entry point (paths relative to the reference repository root).
 *
 * Conventions
 *  - All matrices column-major doubles (R's native layout) with explicit
 *    leading dimension.  X is n x D column-major, i.e. each input dimension is
 *    one contiguous stream.
 *  - Every function returns int: 0 ok; k > 0 = "leading minor of order k is not
 *    positive definite" (LAPACK dpotrf style; mirrors base-R chol()'s error and
 *    Stan's cholesky_decompose domain_error); < 0 = GPMI_E* (text through
 *    gpmi_last_error()).  Nothing throws or aborts across this boundary.
 *  - Host-buffer entry points (no suffix) take ordinary host memory, stage it
 *    through HBM and block until the result is back: this is what `.Call`
 *    binds.  `_dev` entry points take device pointers (e.g. torch tensors'
 *    data_ptr()), enqueue on the context's stream and do NOT synchronise.
 *  - A gpmi_ctx owns its device workspace and stream; it is bound to one GPU
 *    and to the creating process.  HIP state does not survive fork() and cannot
 *    be re-initialised in the child: once the library has touched the GPU in a
 *    process, EVERY call from a forked child of it -- e.g. parallel::mclapply
 *    at pendulum_fit.R:268 --, gpmi_create and gpmi_device_count included,
 *    returns GPMI_EFORK.  Workers must be fresh processes (or fork before the
 *    first gpmi call); prefer the grid API to fork-per-draw.
 *  - There is no CPU fallback anywhere in the library: without a HIP device
 *    gpmi_create fails with GPMI_ENODEV.
 */
#ifndef GPMI_H
#define GPMI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMI_VERSION 302

/* the ABI: the ONLY symbols libgpmi.so exports (it is built with -fvisibility=hidden) */
#define GPMI_API __attribute__((visibility("default")))

typedef struct gpmi_ctx gpmi_ctx;
typedef struct gpmi_seq gpmi_seq; /* sequential conditional sampler (gpmi_seq_*) */

enum {
    GPMI_OK = 0,
    GPMI_EARG = -1,   /* bad argument                              */
    GPMI_EHIP = -2,   /* HIP runtime error                         */
    GPMI_ENOMEM = -3, /* device allocation failed                  */
    GPMI_ENODEV = -4, /* no usable gfx950 device                   */
    GPMI_EFORK = -5   /* called from a forked child of a GPU process */
};

/* derivative-kernel selector: derivative_kernels.R:39-73 (Q value, R first,
 * T second derivative of the process; row argument first) */
enum {
    GPMI_QQ = 0, GPMI_QR = 1, GPMI_RQ = 2, GPMI_RR = 3, GPMI_QT = 4,
    GPMI_TQ = 5, GPMI_RT = 6, GPMI_TR = 7, GPMI_TT = 8
};

/* flags for gpmi_se_cov* */
enum {
    GPMI_FULL = 0,        /* write all n x m entries                              */
    GPMI_LOWER = 1,       /* square case only: write i >= j, leave the rest alone */
    GPMI_COMPAT_RR = 2    /* reproduce R/kernels.R:31's amplitude precedence bug  */
};

/* ---- library / context ------------------------------------------------ */
GPMI_API int gpmi_version(void);
GPMI_API const char *gpmi_last_error(void);
GPMI_API int gpmi_device_count(int *count);
GPMI_API int gpmi_create(gpmi_ctx **ctx, int device);
GPMI_API int gpmi_destroy(gpmi_ctx *ctx);
/* run on a caller-owned hipStream_t; NULL (handle 0) is HIP's legacy null stream -- what
 * torch's default stream is -- so `_dev` calls are ordered with the caller's other work there */
GPMI_API int gpmi_set_stream(gpmi_ctx *ctx, void *hip_stream);
/* back to the context's own (non-blocking) stream */
GPMI_API int gpmi_reset_stream(gpmi_ctx *ctx);
GPMI_API int gpmi_sync(gpmi_ctx *ctx);
/* pre-size the factorisation workspace for matrices of order <= n_max */
GPMI_API int gpmi_reserve(gpmi_ctx *ctx, int n_max);
/* algorithm switches of THIS context (never process-global): "nb_outer" (outer panel width, multiple
 * of 128, 0 = auto), "grid_lanes", "fuse_diag", "ksplit", "block_recursive", "stagger", "se_nt", "nb_adapt",
 * "nb_thr1024", "nb_thr512", "nb_thr256", "small_n", "small_n1", "small_m" (one-workgroup kernels for small
 * problems), "small_ng1", "small_ng" (value + gradient by one workgroup: one evaluation up to n <= small_ng1, several at once
 * up to n <= small_ng <= 256), "grad_aug_n", "grad_aug_ng" (value + gradient through ONE augmented partial factorisation up
 * to this n: one evaluation / several at once), "small_gc" (gpmi_gp_condition in one launch up to n + m + 1 <= small_gc rows), "small_pr" (gpmi_gp_predict[_dev] in
 * one launch up to n + m + 1 <= small_pr rows and D <= 8; 0 sends every size to the blocked chain), "small_pj" (the same for
 * gpmi_gp_predict_joint[_dev], 0 .. 1024), "small_jp" (gpmi_joint_predict[_dev] in one launch up to 2n + p m + 1 <= small_jp rows,
 * 0 .. 1024; 0 sends every size to the chain; default 220: the measured crossover at B = 1 and three orders), "predict_mb" (rows of Xs per chunk of the
 * chains of gpmi_gp_predict / gpmi_seq_marginals; 0 = auto, about n / 4), "small_vjp" (gpmi_exact_gp_f_vjp[_dev] by
 * one workgroup up to n <= small_vjp <= 256; 0 sends every size to the blocked chain), "small_cen" (gpmi_centered_gp_lp_grad[_dev] by one
 * workgroup up to n <= small_cen <= 256 (default 192: the measured crossover), D <= 8, k <= 8; 0 sends every size to the blocked chain), "small_sd", "small_sdb" (gpmi_sample_derivs[_batch]: one workgroup per draw up to
 * n + m + 1 <= small_sd rows for at least small_sdb ((n + m + 1) / 400)^2 draws), "small_n2", "small_g2" (grids of at least small_g2 (n / 1024)^2 + 2 points run one workgroup per point up
 * to n <= small_n2 <= 1024), "calibrate", "timing", "kernel_timing", "debug_ncu" (test hook like gpmi_debug_fill: the compute-unit
 * count the planner of the trailing update sees -- 0: the device's own, 4 .. the device's count: that many; any other value
 * returns GPMI_EARG and changes nothing; no kernel and no default changes, grid lanes copy it); unknown names return GPMI_EARG.  The switches of variants
 * that were measured and rejected ("lookahead", "lane_lookahead", "diag_waves", "gemm_variant", "rect_auto", "syrk_order" = 1)
 * were removed with the variants (DESIGN.md sections 4 and 5 keep the measurements): both builds reject them. */
GPMI_API int gpmi_set_option(gpmi_ctx *ctx, const char *name, int value);

/* ---- covariance builders ---------------------------------------------- */

/* K[i,j] = alpha^2 exp(-1/2 sum_d ((X[i,d]-Y[j,d])/ell[d])^2) (+ diag_add on
 * i == j when X and Y are the same n points).  n_ell = 1 (isotropic) or D (ARD).
 * Replaces QQard(X,Y,phi) R/kernels.R:11-19, QQ(x,y,phi) R/kernels.R:22-24
 * (D = 1), Stan cov_exp_quad models/fit_hyperparameters.stan:19 and the
 * diagonal update :21-24 / models/exact_gp.stan:20-22 (diag_add).
 * Y == NULL means Y = X (symmetric; enables GPMI_LOWER). */
GPMI_API int gpmi_se_cov(gpmi_ctx *ctx, const double *X, int n, int ldx, const double *Y, int m, int ldy,
                int D, double alpha, const double *ell, int n_ell, double diag_add, int flags,
                double *K, int ldk);
GPMI_API int gpmi_se_cov_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, const double *dY, int m,
                    int ldy, int D, double alpha, const double *ell, int n_ell, double diag_add,
                    int flags, double *dK, int ldk);

/* K[i,j] = alpha^2 * kind(x[i], y[j], l), 1-D inputs.  Replaces the matrix API
 * QQ/QR/RR(x,y,phi) of R/kernels.R:22-32 (GPMI_COMPAT_RR for :31 as written)
 * and a^2 * outer(ti, ti, FUN = kern) of pendulum_fit.R:237-240. */
GPMI_API int gpmi_deriv_cov(gpmi_ctx *ctx, int kind, const double *x, int n, const double *y, int m,
                   double alpha, double l, int flags, double *K, int ldk);
GPMI_API int gpmi_deriv_cov_dev(gpmi_ctx *ctx, int kind, const double *dx, int n, const double *dy, int m,
                       double alpha, double l, int flags, double *dK, int ldk);

/* out[i] = kind(tj[i], tk[i], l): the vectorised elementwise functions
 * QQ..TT(tj,tk,l) of derivative_kernels.R:39-73 (unit amplitude). */
GPMI_API int gpmi_deriv_elem(gpmi_ctx *ctx, int kind, const double *tj, const double *tk, size_t len,
                    double l, double *out);

/* Joint [values; derivatives] covariance of order 2n,
 * [[QQ + sigma^2 I, QR], [RQ, RR]] + jitter I   (R/ode_gp_library.R:29-30). */
GPMI_API int gpmi_joint_cov(gpmi_ctx *ctx, const double *t, int n, double alpha, double l, double sigma,
                   double jitter, int flags, double *K, int ldk);

/* ---- dense factorisation ---------------------------------------------- */

/* In-place lower Cholesky A = L L^T (strict upper triangle zeroed on return,
 * like Stan's cholesky_decompose: models/fit_hyperparameters.stan:25,
 * models/exact_gp.stan:23; base-R chol() returns t(L)). */
GPMI_API int gpmi_potrf(gpmi_ctx *ctx, double *A, int n, int lda);
GPMI_API int gpmi_potrf_dev(gpmi_ctx *ctx, double *dA, int n, int lda, int *d_info);

/* f = L z (models/exact_gp.stan:25) and z = L^-1 b (mdivide_left_tri_low inside
 * multi_normal_cholesky, models/fit_hyperparameters.stan:31). */
GPMI_API int gpmi_trmv_lower(gpmi_ctx *ctx, const double *L, int n, int ldl, const double *z, double *f);
GPMI_API int gpmi_trsv_lower(gpmi_ctx *ctx, const double *L, int n, int ldl, const double *b, double *z);
/* w = L^T u: the transpose of gpmi_trmv_lower (z-adjoint of f = L z). */
GPMI_API int gpmi_trmv_lower_t(gpmi_ctx *ctx, const double *L, int n, int ldl, const double *u, double *w);
/* The latent exact GP's transform in ONE call, models/exact_gp.stan:17-25 (test_interpolate.R:31-36 runs it at N = 100):
 * f = cholesky_decompose(cov_exp_quad(X, alpha, ell) + jitter I) z -- covariance, factor and product stay on the
 * device, only z goes in and f comes out (n <= 256: one launch of one workgroup).  Returns 0, or the order of the first
 * non-positive leading minor (f is NaN then). */
GPMI_API int gpmi_exact_gp_f(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                    double jitter, const double *z, double *f);
/* Vector-Jacobian product of that transform: what reverse-mode autodiff needs of models/exact_gp.stan:17-25 (z and l are
 * parameters) and of models/heteroscedastic.stan:23-32 (one factor applied to two vectors, sigmaf = alpha a parameter) at every
 * leapfrog step.  F = L Z for k columns (Z n x k, ldz), upstream adjoint Fbar (n x k, ldfb):
 *   Zbar = L^T Fbar  (n x k, ldzb);
 *   grad[0] = d/dalpha, grad[1 .. n_ell] = d/dell of sum(Fbar o F)  (1 + n_ell doubles);
 *   F (nullable, ldf) = L Z, each column bit-identical to gpmi_exact_gp_f.
 * With U = L^-T, B = Phi(Zbar Z^T) (lower triangle, halved diagonal): Sbar = sym(U B U^T), theta_bar = <Sbar, dK/dtheta>;
 * about 4/3 n^3 flops on top of the value whatever the number of hyper-parameters.  D <= 64, any k (n <= 256, D <= 8, k <= 8:
 * one launch of one workgroup), alpha > 0.  Returns 0, or the order of the first non-positive leading minor (every output NaN). */
GPMI_API int gpmi_exact_gp_f_vjp(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                        double jitter, const double *Z, int k, int ldz, const double *Fbar, int ldfb, double *F /* nullable */,
                        int ldf, double *Zbar, int ldzb, double *grad);
/* the same with device-resident X, Z, Fbar, F, Zbar, grad and d_info (1 int), enqueued on the context's stream (ell: host) */
GPMI_API int gpmi_exact_gp_f_vjp_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, double alpha, const double *ell,
                            int n_ell, double jitter, const double *dZ, int k, int ldz, const double *dFbar, int ldfb,
                            double *dF /* nullable */, int ldf, double *dZbar, int ldzb, double *d_grad, int *d_info);

/* The latent exact-GP models' likelihood part of lp__ and its gradient in one call with ONE factorisation: forward product
 * F = L Z, a likelihood head on F against the m replicate columns of Y (n x m, ldy), the head's adjoint Fbar = d lik / d F and the
 * reverse sweep of gpmi_exact_gp_f_vjp on that Fbar.  Heads (the constants `~` drops are dropped; sums over rows i and columns c):
 *   GPMI_LIK_NORMAL (k = 1; models/exact_gp.stan:27-33, fit_full_gp.stan): lik = sum(-log sigma - (y_ic - f_i)^2 / (2 sigma^2)),
 *     Fbar_i = sum_c (y_ic - f_i) / sigma^2, out[1] = d lik / d sigma = -n m / sigma + sum r^2 / sigma^3;
 *   GPMI_LIK_BERNOULLI_LOGIT (k = 1, y in {0, 1}; models/westbrook_exact.stan): lik = sum(y f - softplus(f)),
 *     Fbar_i = sum_c (y_ic - inv_logit(f_i)), softplus(f) = max(f, 0) + log1p(exp(-|f|)): Stan's bernoulli_logit, finite for |f|
 *     in the hundreds, where the model's bernoulli(inv_logit(f)) underflows;
 *   GPMI_LIK_NORMAL_LOGSD (k = 2, mu = F[:,0], s = F[:,1]; models/heteroscedastic.stan:23-36): lik = sum(-s_i - (y_ic - mu_i)^2
 *     exp(-2 s_i) / 2), Fbar[:,0] = sum_c (y - mu) exp(-2 s), Fbar[:,1] = sum_c ((y - mu)^2 exp(-2 s) - 1).
 * out[0] = lik, out[1] = d lik / d sigma (0 for the heads without sigma); F and Fbar (both nullable, n x k) as computed; Zbar,
 * grad, the return value and NaN on a non-positive leading minor (out[0] too) as gpmi_exact_gp_f_vjp.  Priors and Jacobians stay
 * with the caller.  All sums run in a fixed order: repeated calls give identical bits.  GPMI_EARG: k or m not as the family asks,
 * ldy < n, sigma <= 0 (NORMAL), unknown family, and on this host-buffer form y outside {0, 1} (BERNOULLI_LOGIT). */
enum { GPMI_LIK_NORMAL = 0, GPMI_LIK_BERNOULLI_LOGIT = 1, GPMI_LIK_NORMAL_LOGSD = 2 };
GPMI_API int gpmi_latent_gp_lp_grad(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                           double jitter, const double *Z, int k, int ldz, int family, const double *Y, int m, int ldy,
                           double sigma, double *out, double *F /* nullable */, int ldf, double *Fbar /* nullable */, int ldfb,
                           double *Zbar, int ldzb, double *grad);
/* the same with device-resident X, Z, Y, out (2), F, Fbar, Zbar, grad and d_info (1 int), enqueued on the context's stream */
GPMI_API int gpmi_latent_gp_lp_grad_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, double alpha, const double *ell,
                               int n_ell, double jitter, const double *dZ, int k, int ldz, int family, const double *dY, int m,
                               int ldy, double sigma, double *d_out, double *dF /* nullable */, int ldf,
                               double *dFbar /* nullable */, int ldfb, double *dZbar, int ldzb, double *d_grad, int *d_info);

/* The CENTRED latent GP (models/heteroscedastic_centered.stan:24-34): the latent columns F (n x k, ldf) are parameters
 * themselves and the GP is their prior, f_c ~ multi_normal_cholesky(0, L), Sigma = alpha^2 K0(X; ell) + jitter I = L L^T (the
 * matrix of gpmi_exact_gp_f), with a likelihood head evaluated directly on F.  One factorisation serves all k columns.  With
 * z_c = L^-1 f_c and a_c = Sigma^-1 f_c:
 *   out[2] = sum_i log L_ii, out[3] = sum_c z_c' z_c, prior = -1/2 out[3] - k out[2] (the -n k / 2 log(2 pi) that `~` drops is
 *   dropped); out[0] = prior + lik(F, Y), out[1] = d lik / d sigma, lik exactly as for gpmi_latent_gp_lp_grad (same heads, same k
 *   per head); family GPMI_LIK_NONE: no head (lik = 0; any k >= 1; Y, m, ldy, sigma ignored) -- accepted by these two entry
 *   points only;
 *   Fgrad (n x k, ldfg) = d out[0] / d F = Fbar_head - [a_1 .. a_k];
 *   grad[0] = d prior / d alpha, grad[1 .. n_ell] = d prior / d ell = 1/2 sum_ij (sum_c a_ic a_jc - k Sigma^-1_ij) dSigma_ij / dtheta
 *   (the head does not depend on the hyper-parameters in this parameterisation).
 * D <= 64, n_ell in {1, D}, alpha > 0, any k (n <= small_cen, default 192, at most 256, D <= 8, k <= 8: one launch of one workgroup).  Returns 0, or
 * the order of the first non-positive leading minor (every output NaN).  All sums run in a fixed order: repeated calls give
 * identical bits.  Priors on the hyper-parameters and Jacobians stay with the caller.  GPMI_EARG: n or k < 1; ldx, ldf, ldfg < n;
 * k not as the head asks; ldy < n or m < 1 with a head; sigma <= 0 (NORMAL); unknown family; a NULL pointer; and on this
 * host-buffer form y outside {0, 1} (BERNOULLI_LOGIT). */
enum { GPMI_LIK_NONE = 3 };
GPMI_API int gpmi_centered_gp_lp_grad(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, double alpha, const double *ell,
                             int n_ell, double jitter, const double *F, int k, int ldf, int family, const double *Y, int m,
                             int ldy, double sigma, double *out /* 4 */, double *Fgrad, int ldfg, double *grad /* 1 + n_ell */);
/* the same with device-resident X, F, Y, out (4), Fgrad, grad and d_info (1 int), enqueued on the context's stream without
 * synchronisation (ell: host) */
GPMI_API int gpmi_centered_gp_lp_grad_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, double alpha, const double *ell,
                                 int n_ell, double jitter, const double *dF, int k, int ldf, int family, const double *dY, int m,
                                 int ldy, double sigma, double *d_out, double *dFgrad, int ldfg, double *d_grad, int *d_info);

/* ---- marginal likelihood ---------------------------------------------- */

/* One evaluation of models/fit_hyperparameters.stan:18-32 with double inputs:
 * Sigma = cov_exp_quad(X, alpha, rho) + (sigma^2 + jitter) I; L = chol(Sigma);
 * out[0] = -1/2 z'z - sum log L_ii - n/2 log(2 pi), out[1] = sum log L_ii,
 * out[2] = z'z, z = L^-1 y.  ell/n_ell as in gpmi_se_cov (rho == ell[0]). */
GPMI_API int gpmi_logml(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
               double alpha, const double *ell, int n_ell, double sigma, double jitter,
               double *out3);
/* device-resident X, y; d_out3 (3 doubles) and d_info (1 int) in device memory */
GPMI_API int gpmi_logml_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                   double alpha, const double *ell, int n_ell, double sigma, double jitter,
                   double *d_out3, int *d_info);

/* Log marginal likelihood AND its gradient with respect to (alpha, ell[0..n_ell), sigma):
 * grad[0] = d/dalpha, grad[1 .. n_ell] = d/dell, grad[1 + n_ell] = d/dsigma.  This is what Stan's
 * autodiff computes per leapfrog step for models/fit_hyperparameters.stan:18-32 (the reference has
 * no function of its own for it); 1/2 tr((a a' - K^-1) dK/dtheta) with K^-1 formed on the device.
 * Any D the covariance builder takes (<= 64; QQard, R/kernels.R:11-19).  Same status codes as gpmi_logml
 * (k > 0: not positive definite, grad = NaN). */
GPMI_API int gpmi_logml_grad(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                    double alpha, const double *ell, int n_ell, double sigma, double jitter,
                    double *out3, double *grad);

/* Value AND gradient at G independent points (alpha[g], rho[g], sigma[g]), concurrently on the context's lanes: what
 * rstan's default four chains (pendulum_fit.R:140: chains = 4, cores = 4) ask for per leapfrog step.  out3: 3 G;
 * grad: 3 G, (d/dalpha, d/drho, d/dsigma) per point; info: G (non-PD: NaN, the grid continues).  D <= 64. */
GPMI_API int gpmi_logml_grad_grid(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                                  const double *alpha, const double *rho, const double *sigma, int G, double jitter,
                                  double *out3, double *grad, int *info);

/* gpmi_logml_grad with device-resident X, y, d_out3 (3), d_grad (2 + n_ell), d_info (1 int): enqueued on the context's stream,
 * no synchronisation; the device itself writes the gradient, NaN when the matrix is not positive definite (ell: host).
 * The return value says only whether the work was enqueued; the bits are those of gpmi_logml_grad. */
GPMI_API int gpmi_logml_grad_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                                 double alpha, const double *ell, int n_ell, double sigma, double jitter,
                                 double *d_out3, double *d_grad, int *d_info);

/* Exact leave-one-out cross-validation of the same model (Rasmussen and Williams, section 5.4.2): how well the fit predicts
 * each observation from all the others, in closed form from S^-1 and a = S^-1 y (d = diag S^-1), by ONE factorisation.
 *   out3       as gpmi_logml
 *   loo   (1)  sum_i lpd_i, the LOO log pseudo-likelihood
 *   mu    (n)  E[y_i | y_-i]   = y_i - a_i / d_i
 *   var   (n)  Var[y_i | y_-i] = 1 / d_i, of the OBSERVATION (noise and jitter included)
 *   lpd   (n)  log p(y_i | y_-i) = -1/2 log(2 pi) + 1/2 log d_i - a_i^2 / (2 d_i): the pointwise values loo::loo takes
 *   grad  (2 + n_ell)  d loo / d(alpha, ell.., sigma), in the order of gpmi_logml_grad
 * mu, var, lpd and grad may be NULL; without grad the call costs what gpmi_logml_grad costs, with it one more n^3-flop
 * symmetric product.  Status codes as gpmi_logml_grad: k > 0 (not positive definite) leaves out3 as gpmi_logml_grad does
 * and NaN in every LOO output.  GPMI_EARG: n < 1, D outside 1..64, ldx < n, alpha <= 0, a length-scale <= 0, sigma < 0, a
 * NULL pointer other than mu, var, lpd, grad.  Sums run in a fixed order: repeated calls give identical bits. */
GPMI_API int gpmi_logml_loo(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                            double alpha, const double *ell, int n_ell, double sigma, double jitter,
                            double *out3, double *loo, double *mu, double *var, double *lpd, double *grad);
/* ... with device-resident X, y and outputs (d_info: 1 int): enqueued on the context's stream, no synchronisation; the
 * device writes every output, NaN when the matrix is not positive definite (ell: host).  The bits of the host form. */
GPMI_API int gpmi_logml_loo_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                                double alpha, const double *ell, int n_ell, double sigma, double jitter,
                                double *d_out3, double *d_loo, double *d_mu, double *d_var, double *d_lpd, double *d_grad,
                                int *d_info);

/* Value, gradient AND exact Hessian of gpmi_logml in theta = (alpha, ell[0 .. n_ell), sigma), q = 2 + n_ell, by ONE
 * factorisation and one dense n x n x n product per length-scale: standard errors of fitted hyper-parameters (the inverse of
 * -hess at the maximum), their Laplace approximation, Newton and trust-region steps.
 *   out3  as gpmi_logml;  grad (q, nullable) as gpmi_logml_grad, with its bits wherever that call runs the chain
 *   hess  (q x q, column-major, ldh >= q): hess[i + j ldh] = d^2 out3[0] / dtheta_i dtheta_j, both triangles written,
 *         bit-for-bit symmetric; nothing outside the q rows of a column is written
 * The parameters are the natural ones, in the order of grad; for log-parameters H_log = diag(theta) H diag(theta) +
 * diag(theta o grad).  Status codes as gpmi_logml_grad: k > 0 (not positive definite) leaves out3 as gpmi_logml_grad does
 * and NaN in every entry of grad and hess.  n_ell is 1 (any D <= 64) or D (D <= 8).  GPMI_EARG: n < 1, ldx < n, ldh < q,
 * D outside 1..64, n_ell neither 1 nor D or above 8, alpha <= 0, a length-scale <= 0, sigma < 0, a NULL pointer other than
 * grad; nothing is launched then.  GPMI_ENOMEM: the 2 n_ell + 1 matrices of n x n doubles cannot be allocated.  Sums run in
 * a fixed order, without atomics: repeated calls give identical bits. */
GPMI_API int gpmi_logml_hess(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                             double alpha, const double *ell, int n_ell, double sigma, double jitter,
                             double *out3, double *grad /* nullable */, double *hess, int ldh);
/* ... with device-resident X, y and outputs (d_info: 1 int; ell: host): enqueued on the context's stream, no
 * synchronisation; the device writes every output, the NaNs and d_info = k included.  The bits of the host form. */
GPMI_API int gpmi_logml_hess_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                             double alpha, const double *ell, int n_ell, double sigma, double jitter,
                             double *d_out3, double *d_grad /* nullable */, double *d_hess, int ldh, int *d_info);

/* gpmi_logml_grad_grid on device-resident data: d_out3 3 G, d_grad 3 G, d_info G (alpha, rho, sigma: host arrays) */
GPMI_API int gpmi_logml_grad_grid_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                                      const double *alpha, const double *rho, const double *sigma, int G, double jitter,
                                      double *d_out3, double *d_grad, int *d_info);

/* Value AND gradient at G points with ONE LENGTH-SCALE PER DIMENSION and point: ell G x D point-major as in
 * gpmi_logml_grid_ard; grad G x (D + 2) point-major: grad[g (D + 2)] = d/dalpha, [.. + 1 + d] = d/dell_d,
 * [.. + D + 1] = d/dsigma.  The several optimiser starts of a fit of QQard's theta (R/kernels.R:11-19), whose likelihood is
 * multimodal in the length-scales.  Status codes, info and NaN as gpmi_logml_grad_grid; every point has the bits of
 * gpmi_logml_grad at that point, and the _dev form those of the host form.  D <= 64.  n <= 256 (128 for one point) and
 * D <= 8: one workgroup per point, any number of points; otherwise the context's lanes.  These three grids return GPMI_EARG
 * for n < 1, G < 0, D outside 1..64, ldx < n, a NULL pointer or a length-scale <= 0; G = 0 returns 0 and writes nothing. */
GPMI_API int gpmi_logml_grad_grid_ard(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                                      const double *alpha, const double *ell, const double *sigma, int G, double jitter,
                                      double *out3, double *grad, int *info);
GPMI_API int gpmi_logml_grad_grid_ard_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                                          const double *alpha, const double *ell, const double *sigma, int G, double jitter,
                                          double *d_out3, double *d_grad, int *d_info);

/* G independent hyper-parameter points (alpha[g], rho[g], sigma[g]) on the same
 * data: out3[3*g..], info[g].  Non-PD points get NaN and info[g] = k and the
 * grid continues.  Replaces the stan()-fit + arg-max of R/tests.R:13-27 when a
 * grid search is acceptable; sharding over GPUs is done by the host layer
 * (one context per device / process). */
GPMI_API int gpmi_logml_grid(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                    const double *alpha, const double *rho, const double *sigma, int G,
                    double jitter, double *out3, int *info);
GPMI_API int gpmi_logml_grid_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                        const double *alpha, const double *rho, const double *sigma, int G,
                        double jitter, double *d_out3, int *d_info);

/* The same grid with ONE LENGTH-SCALE PER DIMENSION and point (ARD): ell is G x D, point-major (ell[g * D + d]).
 * QQard(X, Y, phi) takes a vector phi[[2]] (R/kernels.R:11-19); a grid search or optimiser over ARD
 * length-scales evaluates exactly this.  Everything else as gpmi_logml_grid. */
GPMI_API int gpmi_logml_grid_ard(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                        const double *alpha, const double *ell, const double *sigma, int G,
                        double jitter, double *out3, int *info);
GPMI_API int gpmi_logml_grid_ard_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                            const double *alpha, const double *ell, const double *sigma, int G,
                            double jitter, double *d_out3, int *d_info);

/* Log marginal likelihood of stacked observations yy = [y; y'] (length 2n)
 * under gpmi_joint_cov's matrix (BASELINE config c5). */
GPMI_API int gpmi_joint_logml(gpmi_ctx *ctx, const double *t, int n, const double *yy, double alpha,
                     double l, double sigma, double jitter, double *out3);
GPMI_API int gpmi_joint_logml_dev(gpmi_ctx *ctx, const double *dt, int n, const double *dyy, double alpha,
                         double l, double sigma, double jitter, double *d_out3, int *d_info);
/* G independent (alpha[g], l[g], sigma[g]) points of the joint model on the same device-resident data, concurrently
 * on the context's lanes: d_out3[3 g ..], d_info[g] (non-PD points get NaN and the grid continues). */
GPMI_API int gpmi_joint_logml_grid_dev(gpmi_ctx *ctx, const double *dt, int n, const double *dyy, const double *alpha,
                                       const double *l, const double *sigma, int G, double jitter, double *d_out3,
                                       int *d_info);

/* Value AND gradient of gpmi_joint_logml through one factorisation of its order-2n matrix: out3 as there,
 * grad[0..2] = d out3[0] / d(alpha, l, sigma) = 1/2 tr((a a' - S^-1) dS/dtheta), a = S^-1 yy, with S^-1 formed on the device and
 * the four derivative blocks contracted from one exp per pair of time points.  Returns 0, or the order k of the first
 * non-positive leading minor (out3 as gpmi_joint_logml returns it, grad = NaN).  The options "grad_aug_n" / "grad_aug_ng" apply to
 * the order 2n.  All sums run in a fixed order: repeated calls give identical bits.  GPMI_EARG: n < 1, a NULL pointer, l <= 0 or
 * not finite, alpha <= 0. */
GPMI_API int gpmi_joint_logml_grad(gpmi_ctx *ctx, const double *t, int n, const double *yy, double alpha, double l, double sigma,
                          double jitter, double *out3, double *grad /* 3 */);
/* device-resident t, yy, d_out3 (3), d_grad (3), d_info (1 int): enqueued on the context's stream, no synchronisation; the
 * device itself writes the NaN gradient of a matrix that is not positive definite */
GPMI_API int gpmi_joint_logml_grad_dev(gpmi_ctx *ctx, const double *dt, int n, const double *dyy, double alpha, double l,
                              double sigma, double jitter, double *d_out3, double *d_grad, int *d_info);
/* G points (alpha[g], l[g], sigma[g]) on the same data, concurrently on the context's lanes: out3 3 G, grad 3 G, info G
 * (a point that is not positive definite: NaN gradient, info[g] = k, and the grid continues).  Every point is bit-identical to
 * the single call with its parameters wherever both take the same route (orders between grad_aug_ng and grad_aug_n do not, for
 * G > 1).  GPMI_EARG also for G < 0; G = 0 returns 0. */
GPMI_API int gpmi_joint_logml_grad_grid(gpmi_ctx *ctx, const double *t, int n, const double *yy, const double *alpha,
                               const double *l, const double *sigma, int G, double jitter, double *out3, double *grad,
                               int *info);

/* ---- Rcpp export ------------------------------------------------------ */

/* rbf_cov_chol(x1, l): Sigma_ij = exp(-(xi-xj)^2/(2 l^2)) + 1e-10 I, L = chol,
 * dLdl = dL/dl (forward-mode tangent).  covariance.cpp:9-47.  L, dLdl n x n. */
GPMI_API int gpmi_rbf_cov_chol(gpmi_ctx *ctx, const double *x, int n, double l, double *L, int ldl,
                      double *dLdl, int lddl);

/* ---- Cholesky-factor interpolation over the length-scale ---------------
 * Table of P factors L(lp[p]) and tangents dL/dl(lp[p]) kept in HBM (2 P n^2 doubles), then
 * piecewise cubic Hermite blends at any l.  Interval rule of the reference: the first p with
 * lp[p+1] >= l (clamped to the last interval, where the reference reads past the end).
 *   gpmi_interp_build : the table test_interpolate.R:9-19 builds with P calls of rbf_cov_chol
 *   gpmi_interp_load  : a caller-supplied table (P stacked n x n column-major matrices, leading
 *                       dimension ld, matrix p at Ls + p*ld*n) -- the `Ls`, `dLdls` data of
 *                       models/cubic_interpolated_gp.stan:11-12
 *   gpmi_approx_L     : covariance.cpp:49-96 (lower triangle blended, zeros above)
 *   gpmi_approx_Lz    : models/cubic_interpolated_gp.hpp:38-73, f = approx_L(l) z, fused (the
 *                       blended matrix is never stored: 4 n^2/2 doubles read per call)
 *   gpmi_approx_Lz_grad : the same value plus dfdl = (dv/dl) z, the partial Stan's reverse mode
 *                       attaches to every output of approx_Lz (`var` overload of build_output,
 *                       cubic_interpolated_gp.hpp:6-32, dvdl :67) -- what makes the external
 *                       function differentiable in l (cubic_interpolated_gp.stan:1-3); same pass,
 *                       same traffic.  (d f / d z is the blend itself: gpmi_approx_L.)
 * gpmi_interp_build factors the P table entries concurrently on the context's grid lanes.      */
GPMI_API int gpmi_interp_build(gpmi_ctx *ctx, const double *x, int n, const double *lp, int P);
GPMI_API int gpmi_interp_load(gpmi_ctx *ctx, const double *lp, int P, const double *Ls, const double *dLdls,
                     int n, int ld);
GPMI_API int gpmi_approx_L(gpmi_ctx *ctx, double l, double *out, int ldo);
GPMI_API int gpmi_approx_Lz(gpmi_ctx *ctx, double l, const double *z, double *f);
GPMI_API int gpmi_approx_Lz_dev(gpmi_ctx *ctx, double l, const double *dz, double *df);
GPMI_API int gpmi_approx_Lz_grad(gpmi_ctx *ctx, double l, const double *z, double *f, double *dfdl);
GPMI_API int gpmi_approx_Lz_grad_dev(gpmi_ctx *ctx, double l, const double *dz, double *df, double *ddfdl);
GPMI_API int gpmi_interp_free(gpmi_ctx *ctx);
/* cubic_interpolated_gp.hpp:6-32,38-73 under reverse mode: F = v(l) Z, Zbar = v(l)^T Fbar,
 * lbar = sum(Fbar o (dv/dl) Z); table from gpmi_interp_build / gpmi_interp_load.  Z, Fbar, F, Zbar: n x k, column-major.
 * One pass over the interval's four triangles (k <= 8 columns per pass; n <= 256, k <= 8: one launch); every column of F
 * is bit-identical to gpmi_approx_Lz.  Errors (GPMI_EARG): no table, k < 1, non-finite l. */
GPMI_API int gpmi_approx_Lz_vjp(gpmi_ctx *ctx, double l, const double *Z, int k, int ldz, const double *Fbar, int ldfb,
                       double *F /* nullable */, int ldf, double *Zbar, int ldzb, double *lbar);
/* the same on device pointers (d_lbar: 1 double), enqueued on the context's stream */
GPMI_API int gpmi_approx_Lz_vjp_dev(gpmi_ctx *ctx, double l, const double *dZ, int k, int ldz, const double *dFbar, int ldfb,
                           double *dF /* nullable */, int ldf, double *dZbar, int ldzb, double *d_lbar);
/* The GP-regression interpolation of models/interpolated_gp.stan:9-47 (rho = 1, jitter = 1e-10 in the reference):
 * transformed data lookup = (Sigma_P \ exact)^T with Sigma_P = cov_exp_quad(lp, 1, rho) + jitter I (partial-pivot LU, P <= 64)
 * and exact the P factors chol(cov_exp_quad(x, 1, lp[p]) + 1e-10 I), kept on the device as P lower triangles M_p beside
 * (not in place of) the Hermite table; L(l) = sum_p w_p M_p with w_p = exp(-(l - lp_p)^2 / (2 rho^2)).
 * gpmi_interp_gp_build factors x as gpmi_interp_build does and returns its status codes; gpmi_interp_gp_load takes the P
 * stacked n x n factors.  The Lz calls follow gpmi_approx_Lz_vjp (lbar from w'_p = -(l - lp_p) / rho^2 w_p); F of
 * gpmi_interp_gp_Lz and of gpmi_interp_gp_Lz_vjp are bit-identical.  Errors (GPMI_EARG): no table, P > 64, singular
 * Sigma_P, k < 1, non-finite l. */
GPMI_API int gpmi_interp_gp_build(gpmi_ctx *ctx, const double *x, int n, const double *lp, int P, double rho, double jitter);
GPMI_API int gpmi_interp_gp_load(gpmi_ctx *ctx, const double *lp, int P, double rho, double jitter,
                        const double *Ls /* P stacked n x n exact factors */, int n, int ld);
GPMI_API int gpmi_interp_gp_L(gpmi_ctx *ctx, double l, double *out, int ldo);
GPMI_API int gpmi_interp_gp_Lz(gpmi_ctx *ctx, double l, const double *Z, int k, int ldz, double *F, int ldf);
GPMI_API int gpmi_interp_gp_Lz_vjp(gpmi_ctx *ctx, double l, const double *Z, int k, int ldz, const double *Fbar, int ldfb,
                          double *F /* nullable */, int ldf, double *Zbar, int ldzb, double *lbar);
GPMI_API int gpmi_interp_gp_Lz_vjp_dev(gpmi_ctx *ctx, double l, const double *dZ, int k, int ldz, const double *dFbar, int ldfb,
                              double *dF /* nullable */, int ldf, double *dZbar, int ldzb, double *d_lbar);
GPMI_API int gpmi_interp_gp_free(gpmi_ctx *ctx);

/* ---- GP posterior (value / derivative) -------------------------------- */

/* mn = Ks (K + s2 I)^-1 y,  Kn = Kss - Ks (K + s2 I)^-1 Ks^T + jitter I with
 * K = alpha^2 kindK(t,t), Ks = alpha^2 kindS(ts,t), Kss = alpha^2 kindSS(ts,ts)
 * through ONE Cholesky of K + s2 I (the reference does two LU solves).
 *  p_Xn      R/ode_gp.R:1-14     : (QQ, QQ, QQ), ts = t
 *  p_dotXn   R/ode_gp.R:19-32    : (QQ, RQ, RR), ts = t
 *  sample_derivs moments pendulum_fit.R:242-251 : (QQ, RQ, RR), jitter 1e-8
 *  lorenz.Rmd:80-107 variant: separate prediction times ts.
 * mn: m doubles; Kn: m x m (symmetric, both triangles written). */
GPMI_API int gpmi_gp_condition(gpmi_ctx *ctx, const double *t, int n, const double *ts, int m,
                      const double *y, double alpha, double l, double s2, double jitter,
                      int kindK, int kindS, int kindSS, int flags, double *mn, double *Kn, int ldkn);

/* Pointwise posterior of the latent function at m new D-dimensional inputs Xs (m x D, column-major, ldxs) under the ARD
 * squared-exponential model of gpmi_logml: Sigma = K(X, X) + (sigma^2 + jitter) I = L L^T (exactly gpmi_logml's matrix, so fitted
 * hyper-parameters go in unchanged), k_j = K(X, xs_j),
 *   mean[j] = k_j^T Sigma^-1 y,   var[j] = alpha^2 - k_j^T Sigma^-1 k_j.
 * var is the LATENT function's variance (the caller adds sigma^2 for a new observation) and is returned AS COMPUTED, not
 * clamped: where the posterior is tight it is a difference of O(alpha^2) terms and may come out as a tiny negative number.
 * This is what create_p_dotXnS conditions on (QQard(X, X, theta) with D = ncol(X), R/ode_gp_library.R:43-93) and the D-dimensional
 * counterpart of the (QQ, QQ, QQ) case of gpmi_gp_condition without the m x m covariance: one factorisation of order n, Xs in
 * chunks (any m).  var == NULL: the mean alone through a = Sigma^-1 y and a fused kernel evaluation, no n^2 m solve.
 * n + m + 1 <= small_pr rows and D <= 8: one launch of one workgroup.  ell / n_ell as in gpmi_se_cov.  All sums run in a fixed
 * order: repeated calls give identical bits.  Returns 0, or the order k of the first non-positive leading minor of Sigma (mean and
 * var are all NaN then).  GPMI_EARG: n or m < 1, D outside 1..64, ldx < n, ldxs < m, alpha <= 0, a length-scale <= 0, sigma < 0, a
 * NULL pointer other than var. */
GPMI_API int gpmi_gp_predict(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                    double alpha, const double *ell, int n_ell, double sigma, double jitter,
                    const double *Xs, int m, int ldxs, double *mean /* m */, double *var /* m, nullable */);
/* the same with device-resident X, y, Xs, mean, var (nullable) and d_info (1 int), enqueued on the context's stream (ell: host) */
GPMI_API int gpmi_gp_predict_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                        double alpha, const double *ell, int n_ell, double sigma, double jitter,
                        const double *dXs, int m, int ldxs, double *d_mean, double *d_var /* nullable */, int *d_info);

/* JOINT posterior of the latent function at the m new inputs Xs under the same model (Sigma, ell / n_ell as in gpmi_gp_predict):
 *   mean = Ks Sigma^-1 y,   C = K(Xs, Xs) - Ks Sigma^-1 Ks^T + post_jitter I,   draws[:, b] = mean + chol(C) Z[:, b],   Ks = K(Xs, X)
 * -- the distribution create_p_dotXnS (R/ode_gp_library.R:43-93) samples from point by point, for all m points in one call.  C is
 * the LATENT function's covariance as computed, not clamped (the caller puts sigma^2 for new observations into post_jitter; any
 * finite value, negative included).  cov (m x m, ldc; nullable) receives C with both triangles written, bit-for-bit symmetric;
 * with cov == NULL the m x m matrix never leaves the device.  Z (m x B, ldz) holds the caller's standard-normal variates, draws
 * (m x B, ldd) the B draws; both may be NULL iff B == 0, and then C is not factored.  n + m + 1 <= small_pj rows and D <= 8: one
 * launch of one workgroup; otherwise one workspace of (n + m + 1)^2 doubles, two partial factorisations and one triangular
 * matrix-matrix product (GPMI_ENOMEM when the workspace cannot be allocated).  The route depends on (n, m, D) and the options,
 * never on B, and all sums run in a fixed order: repeated calls give identical bits, and column b of draws has the same bits
 * whatever B is and whatever the other columns of Z hold.  Status: 0; k in 1..n: Sigma is not positive definite at order k and
 * every output is NaN; n + k: C is not positive definite at order k, mean and cov are valid (the bits of the same call with
 * B = 0) and draws are all NaN.  GPMI_EARG: n or m < 1, B < 0, D outside 1..64, ldx < n, ldxs < m, ldc < m with cov, ldz < m or
 * ldd < m with B > 0, alpha <= 0, a length-scale <= 0, sigma < 0, a NULL pointer other than cov (and Z / draws when B == 0). */
GPMI_API int gpmi_gp_predict_joint(gpmi_ctx *ctx, const double *X, int n, int ldx, int D, const double *y,
                    double alpha, const double *ell, int n_ell, double sigma, double jitter,
                    const double *Xs, int m, int ldxs, double post_jitter,
                    double *mean /* m */, double *cov /* m x m, nullable */, int ldc,
                    const double *Z /* m x B */, int B, int ldz, double *draws /* m x B */, int ldd);
/* the same with device-resident X, y, Xs, mean, cov, Z, draws and d_info (1 int): enqueued on the context's stream, not
 * synchronised; the return value says only whether the work was enqueued, the device writes d_info and the NaNs.  Nothing
 * outside the m rows of a column is written */
GPMI_API int gpmi_gp_predict_joint_dev(gpmi_ctx *ctx, const double *dX, int n, int ldx, int D, const double *dy,
                    double alpha, const double *ell, int n_ell, double sigma, double jitter,
                    const double *dXs, int m, int ldxs, double post_jitter,
                    double *d_mean, double *d_cov /* nullable */, int ldc,
                    const double *dZ, int B, int ldz, double *d_draws, int ldd, int *d_info);

/* Prediction for the joint value-and-derivative model of gpmi_joint_logml (R/ode_gp_library.R:29-30): the posterior of f, f'
 * and f'' at the m new times ts given the stacked observations yy = [y; y'] at the n times t -- both series of
 * pendulum_fit3.R:31-46 conditioned on at once, where the reference differentiates each series on its own
 * (pendulum_fit.R:227-268).  `orders` is a bit mask of the p requested derivative orders a_1 < .. < a_p; every output is stacked
 * by order, m rows per block: [f(ts); f'(ts); f''(ts)] restricted to the requested orders.  S is exactly gpmi_joint_logml's
 * matrix (alpha, l, sigma, jitter as there: fitted hyper-parameters go in unchanged).  With the kind letters Q, R, T for the
 * orders 0, 1, 2, first argument first (derivative_kernels.R:39-73):
 *   Ks block a = alpha^2 [kind(a, Q)(ts, t), kind(a, R)(ts, t)]  (p m x 2n),   Kss block (a, b) = alpha^2 kind(a, b)(ts, ts),
 *   mean = Ks S^-1 yy,   C = Kss - Ks S^-1 Ks^T + diag(post_jitter[a] on block a),   draws[:, b] = mean + chol(C) Z[:, b].
 * post_jitter (host memory in both forms) holds one finite value per requested order, negative allowed -- per order because f,
 * f', f'' carry the units alpha^2, alpha^2 / l^2, alpha^2 / l^4; the caller's observation noise goes here.  cov (p m x p m, ldc;
 * nullable) receives C with both triangles written, bit-for-bit symmetric; with cov == NULL the matrix never leaves the device.
 * Z (p m x B, ldz) and draws (p m x B, ldd) may be NULL iff B == 0, and then C is not factored.  2n + p m + 1 <= small_jp rows:
 * one launch of one workgroup; otherwise one workspace of (2n + p m + 1)^2 doubles, a fused builder of the star blocks (one
 * exponential per pair of points, every entry with the bits gpmi_deriv_cov gives for its kind), two partial factorisations and
 * one triangular matrix-matrix product (GPMI_ENOMEM when the workspace cannot be allocated).  The route depends on (n, m, p)
 * and the options, never on B, and all sums run in a fixed order: repeated calls give identical bits, and column b of draws has
 * the same bits whatever B is and whatever the other columns of Z hold.  Status: 0; k in 1..2n: S is not positive definite at
 * order k and every output is NaN; 2n + k: C is not positive definite at order k, mean and cov are valid (the bits of the same
 * call with B = 0) and draws are all NaN.  GPMI_EARG: n or m < 1, B < 0, orders outside 1..7, ldc < p m with cov, ldz or
 * ldd < p m with B > 0, alpha <= 0, l <= 0 or not finite, sigma < 0, a non-finite post_jitter, a NULL pointer other than cov (and
 * Z / draws when B == 0). */
enum { GPMI_OUT_VALUE = 1, GPMI_OUT_DERIV = 2, GPMI_OUT_DERIV2 = 4 };   /* bit mask `orders` */
GPMI_API int gpmi_joint_predict(gpmi_ctx *ctx, const double *t, int n, const double *yy /* 2n */,
                    double alpha, double l, double sigma, double jitter,
                    const double *ts, int m, int orders, const double *post_jitter /* p */,
                    double *mean /* p m */, double *cov /* p m x p m, nullable */, int ldc,
                    const double *Z /* p m x B */, int B, int ldz, double *draws /* p m x B */, int ldd);
/* the same with device-resident t, yy, ts, mean, cov, Z, draws and d_info (1 int); post_jitter stays in host memory.  Enqueued on
 * the context's stream, not synchronised; the return value says only whether the work was enqueued, the device writes d_info
 * and the NaNs.  Nothing outside the p m rows of a column is written */
GPMI_API int gpmi_joint_predict_dev(gpmi_ctx *ctx, const double *dt, int n, const double *dyy,
                    double alpha, double l, double sigma, double jitter,
                    const double *dts, int m, int orders, const double *post_jitter /* p, host */,
                    double *d_mean, double *d_cov /* nullable */, int ldc,
                    const double *dZ, int B, int ldz, double *d_draws, int ldd, int *d_info);

/* One draw of the derivative process given noisy values: sample_derivs(params = (l, a, sy), ynoise, ti),
 * pendulum_fit.R:227-255 (separate prediction times ts: lorenz.Rmd:80-107, jitter 1e-6 there, 1e-8 here):
 * draw = mu + chol(cov) z with the (QQ, RQ, RR) moments of gpmi_gp_condition, fused on the device -- the
 * m x m covariance is factored in place in the workspace and never crosses PCIe.  The reference draws
 * with MASS::mvrnorm and R's unseeded RNG, so the standard-normal variate z (m doubles) is the caller's;
 * mu (nullable) receives the mean.  Status k in 1..n: K + sy^2 I is not positive definite at order k;
 * n + k: the posterior covariance is not (at order k). */
GPMI_API int gpmi_sample_derivs(gpmi_ctx *ctx, const double *t, int n, const double *ts, int m, const double *y,
                                double l, double a, double sy, double jitter, const double *z, double *draw, double *mu);
/* B independent draws -- the loop mclapply(s_list[1:100], sample_derivs_both_states, mc.cores = 2) of
 * pendulum_fit.R:261-268 (one posterior draw of (l, a, sy) and one noisy series per call) -- run as
 * concurrent conditionings on the context's lanes.  params: 3 x B (l, a, sy per draw); Y: n x B, Z: m x B,
 * draws: m x B, mus (nullable): m x B, column-major with the given leading dimensions; info[b] as the
 * status of gpmi_sample_derivs (a failed draw does not stop the others). */
GPMI_API int gpmi_sample_derivs_batch(gpmi_ctx *ctx, const double *t, int n, const double *ts, int m, const double *Y,
                                      int ldy, const double *params, int B, double jitter, const double *Z, int ldz,
                                      double *draws, int ldd, double *mus, int ldmu, int *info);

/* ---- sequential conditional sampler ------------------------------------ */

/* create_p_dotXnS(Xn_list, mn, Kn, theta), R/ode_gp_library.R:43-93 (R/tests.R:78-91): a stateful
 * sampler of the derivative at new states xs, one at a time, each conditioned on the draws
 * already made.  X = do.call(cbind, Xn_list) (n x D), theta = (alpha, ell) of QQard; mn, Kn the
 * derivative posterior at the data (p_dotXn); jitter = 1e-6 in the reference (:55 and :77).
 * With K~ = K_XX + jitter I the joint law of the star points is N(m, K),
 *   m = K_XsX K~^-1 mn,  K = K_XsXs - K_XsX (K~^-1 - K~^-1 Kn K~^-1) K_XXs + jitter I   (:74-77);
 * gpmi_seq_step returns out2 = (condMean, condVar) of the NEW point given the committed draws
 * (what condMVN returns at :80-81; the closure's `mu`, `sigma`), gpmi_seq_commit appends the
 * value drawn for it (the reference draws rnorm(1, condMean, condVar) at :83 with R's RNG, so
 * the draw itself belongs to the caller).  A step that is not committed is discarded by the next
 * step.  The O(n^3) work (one Cholesky, two n-row triangular solves) happens once in
 * gpmi_seq_create; a step reads 12 n^2 B (factor + one n x n matrix).  max_steps <= 2048.
 * Status k > 0: K~ (create) or the star covariance (step, k = its order) is not positive definite. */
GPMI_API int gpmi_seq_create(gpmi_ctx *ctx, gpmi_seq **out, const double *X, int n, int ldx, int D,
                    const double *mn, const double *Kn, int ldkn, double alpha, const double *ell,
                    int n_ell, double jitter, int max_steps);
GPMI_API int gpmi_seq_step(gpmi_seq *seq, const double *xs /* D */, double *out2);
GPMI_API int gpmi_seq_commit(gpmi_seq *seq, double dot_xs);
GPMI_API int gpmi_seq_count(const gpmi_seq *seq); /* committed draws */
GPMI_API int gpmi_seq_destroy(gpmi_seq *seq);
/* For each of the m rows of Xs (m x D, column-major, ldxs): what gpmi_seq_step would return as out2 on a sampler with NO
 * committed draws -- the sweep of R/tests.R:89-97, which builds a fresh sampler per state and takes only its first step, in one
 * call and without a factorisation.  With the stored factor L, B = I - L^-1 Kn L^-T, b = L^-1 mn and t_j = L^-1 k_j:
 *   mean[j] = t_j . b,   var[j] = k(xs, xs) + jitter - t_j^T B t_j   (as computed, not clamped).
 * The sampler is only read: committed draws, a pending step and gpmi_seq_count stay as they were.  Returns 0 (there is no joint
 * factor, hence no positive-definiteness status), or GPMI_EARG: m < 1, ldxs < m, a NULL pointer. */
GPMI_API int gpmi_seq_marginals(gpmi_seq *seq, const double *Xs, int m, int ldxs, double *mean, double *var);

/* ---- low-rank (Hermite-eigenfunction) GP -------------------------------- */

/* The Mercer expansion of the squared-exponential kernel in 1-D: with a = 1 / (4 scale^2), eps^2 = 1 / (2 l^2), alpha^2 = 2 a,
 * beta = (1 + 4 eps^2 / alpha^2)^(1/4), delta^2 = alpha^2 (beta^2 - 1) / 2 and Dn = alpha^2 + delta^2 + eps^2, for k = 1 .. M
 *   Phi[i, k] = amp sqrt(lambda_k) phi_k(x_i),  lambda_k = sqrt(alpha^2 / Dn) (eps^2 / Dn)^(k-1),
 *   phi_k(x) = sqrt(beta / (2^(k-1) (k-1)!)) exp(-delta^2 x^2) H_(k-1)(alpha beta x)   (physicists' Hermite polynomials),
 * and Phi Phi^T -> amp^2 exp(-(x_i - x_j)^2 / (2 l^2)) as M grows.  `amp` is the `sigma` argument of the models' approx_L
 * (renamed: sigma stays the noise), `scale` its `scale`.  The device evaluates the three-term recurrence of the columns and,
 * for dPhi_dl, its forward tangent in l; every entry point below generates Phi with the same statements, hence the same bits.
 * M <= GPMI_LR_MMAX.  GPMI_EARG for every function of this section: n < 1, M outside 1..GPMI_LR_MMAX, scale, amp or l not
 * positive and finite, sigma not positive and finite where a noise is used, a leading dimension below n, m < 1, a NULL pointer
 * not marked nullable; nothing is launched then.
 *
 * gpmi_hermite_basis: Phi (n x M, column-major, ldp) and optionally dPhi_dl (lddp); nothing outside the n rows of a column is
 * written.  Replaces approx_L of models/westbrook.stan:2-30 (and its copies in fit_approx_gp, density_gp, diffusion_gp,
 * diffusion_state_gp, fit_ko_approx, multiple_players) and bH of spectral_test.R:6-27. */
#define GPMI_LR_MMAX 128
GPMI_API int gpmi_hermite_basis(gpmi_ctx *ctx, const double *x, int n, int M, double scale, double amp, double l, double *Phi,
                       int ldp, double *dPhi_dl /* nullable */, int lddp);
/* the same with device-resident x, Phi, dPhi_dl, enqueued on the context's stream and not synchronised */
GPMI_API int gpmi_hermite_basis_dev(gpmi_ctx *ctx, const double *dx, int n, int M, double scale, double amp, double l, double *dPhi,
                           int ldp, double *d_dPhi_dl /* nullable */, int lddp);

/* The marginal form y ~ N(0, Phi Phi^T + sigma^2 I) (the model westbrook.stan:72 compares with cov_exp_quad, marginalised over
 * z) and its gradient.  With G = Phi^T Phi, A = sigma^2 I_M + G, b = Phi^T y, u = A^-1 b:
 *   log|Sigma| = (n - M) log sigma^2 + log|A|,  y^T Sigma^-1 y = (y^T y - b^T u) / sigma^2.
 *   out3[0] = log marginal likelihood (with -n/2 log 2 pi), out3[1] = 1/2 log|Sigma|, out3[2] = y^T Sigma^-1 y: the layout of
 *   gpmi_logml, comparable entry by entry with the exact call once M has converged;
 *   grad (3, nullable) = d out3[0] / d (amp, l, sigma).
 * No n x M or n x n matrix is stored: the Gram products [Phi y]^T [Phi y dPhi/dl] are reduced over chunks of rows on the f64
 * matrix cores with the basis generated on the fly, one partial per chunk (the number of chunks depends on n and M alone), and
 * one workgroup adds the partials in chunk order, factors A and finishes.  No atomics: repeated calls and the two forms give
 * identical bits.  Returns 0, or k in 1..M when A is not positive definite at order k (out3 and grad all NaN). */
GPMI_API int gpmi_lowrank_logml_grad(gpmi_ctx *ctx, const double *x, int n, const double *y, int M, double scale, double amp, double l,
                            double sigma, double *out3, double *grad /* 3, nullable */);
/* the same with device-resident x, y, out3, grad and d_info (1 int: the status; the device writes the NaNs), enqueued on the
 * context's stream and not synchronised */
GPMI_API int gpmi_lowrank_logml_grad_dev(gpmi_ctx *ctx, const double *dx, int n, const double *dy, int M, double scale, double amp,
                                double l, double sigma, double *d_out3, double *d_grad /* 3, nullable */, int *d_info);

/* The latent form the models evaluate per leapfrog step: q = Phi z (z: M), then a likelihood head of gpmi_latent_gp_lp_grad on
 * q against the m replicate columns of Y (n x m, ldy):
 *   GPMI_LIK_NORMAL (fit_approx_gp.stan:46-58), GPMI_LIK_BERNOULLI_LOGIT (westbrook.stan:51-61, multiple_players.stan); the
 *   other families return GPMI_EARG.
 *   out[0] = lik, out[1] = d lik / d sigma; q and qbar = d lik / d q (n each, both nullable); zbar (M) = Phi^T qbar;
 *   grad[0] = d lik / d amp = qbar^T q / amp, grad[1] = d lik / d l = qbar^T (dPhi/dl z).
 * Priors (z[1] ~ normal(0, 0.01) among them) and Jacobians stay with the caller.  Phi is regenerated for the second pass, not
 * stored.  There is no factorisation, hence no positive-definiteness status: returns 0 or an error.  On this host-buffer form y
 * outside {0, 1} is GPMI_EARG for the Bernoulli head.  Fixed-order sums: repeated calls and the two forms give identical bits. */
GPMI_API int gpmi_lowrank_latent_lp_grad(gpmi_ctx *ctx, const double *x, int n, int M, double scale, double amp, double l,
                                const double *z, int family, const double *Y, int m, int ldy, double sigma, double *out /* 2 */,
                                double *q /* nullable */, double *qbar /* nullable */, double *zbar, double *grad /* 2 */);
/* the same with device-resident x, z, Y, out, q, qbar, zbar, grad, enqueued on the context's stream and not synchronised */
GPMI_API int gpmi_lowrank_latent_lp_grad_dev(gpmi_ctx *ctx, const double *dx, int n, int M, double scale, double amp, double l,
                                    const double *dz, int family, const double *dY, int m, int ldy, double sigma,
                                    double *d_out /* 2 */, double *dq /* nullable */, double *dqbar /* nullable */,
                                    double *dzbar, double *d_grad /* 2 */);

/* ---- diagnostics (tests / bench) -------------------------------------- */

/* Elapsed ms of the most recent evaluation's stages, measured with HIP events
 * on the context's stream when timing is enabled via gpmi_set_option("timing",1):
 * ms[0] covariance build, ms[1] Cholesky, ms[2] finalize; n_launch[0..2]. */
GPMI_API int gpmi_last_timing(gpmi_ctx *ctx, double *ms3);

/* Per-kernel HIP-event timing, enabled with gpmi_set_option("kernel_timing", 1): event
 * pairs bracket every covariance-build launch (category 0; work = bytes written), every
 * trailing-update SYRK launch (1; work = algorithmic flops) on the context's stream.
 * out9[3*cat + 0..2] = launches, total ms, total work since the last reset. */
GPMI_API int gpmi_kernel_timing(gpmi_ctx *ctx, int reset, double *out9);
/* The same with out12[9..11] = launches, total ms, total flops of the trailing-update launches of more than one
 * round of tiles -- the throughput-bound subset of category 1 (a single-round launch carries the next diagonal
 * block's factorisation and is bounded by that latency chain). */
GPMI_API int gpmi_kernel_timing_ex(gpmi_ctx *ctx, int reset, double *out12);

/* Test hook for the invariant "no result depends on the contents of context-owned scratch at entry": synchronises the
 * context's streams, sets every byte of every buffer of the context and of its grid lanes that holds only floating-point
 * scratch -- the workspace W, the staging buffers, the device scratch, the packed-factor ring, the finalize sums, the result
 * doubles, the parameter records of the device-parameter grids, the partial sums of gpmi_approx_Lz and the payload of the
 * pinned buffer, each over its full allocation -- to `byte` (0..255; 0xFF makes every double a NaN, 0x7F 1.38e306), and
 * synchronises again.  Counters, info words, the completion flag of the pinned buffer, the interpolation tables and the
 * buffers of a gpmi_seq are state and are left alone; buffers not allocated yet are skipped.  Never called by the library
 * itself.  GPMI_EARG: byte outside 0..255. */
GPMI_API int gpmi_debug_fill(gpmi_ctx *ctx, int byte);
/* *nonzero = the number of non-zero words among the 512 device counters of the context plus those of each grid lane, after a
 * synchronisation: the counters the waiting kernels poll are zeroed at creation and left zero by every call, and this reads
 * them back with a copy, without launching a kernel that would wait on them. */
GPMI_API int gpmi_debug_counters(gpmi_ctx *ctx, int *nonzero);

/* ---- probes: tools/ only ------------------------------------------------
 * Built into libgpmi_probes.so (-DGPMI_PROBES: `python -m gp_amd._build --probes`), never into the
 * shipped libgpmi.so: micro-benchmarks and instruments of the product's kernels, and the
 * debug_topology option. */
#ifdef GPMI_PROBES
/* Stand-alone trailing-update (SYRK, lower) launch on synthetic data, C(m x m) -= P P^T with
 * P m x k: average ms per launch over `reps` back-to-back launches (HIP events). */
GPMI_API int gpmi_probe_syrk(gpmi_ctx *ctx, int m, int k, int reps, double *ms);

/* Shader-clock probe of the SYRK kernel: out3 = summed shader cycles, summed 100 MHz ticks and number of
 * workgroups of every trailing-update launch since the last reset. */
GPMI_API int gpmi_probe_clock(gpmi_ctx *ctx, int reset, double *out3);

/* Fused in-block launches since the last call, block 0: cycles in the sub-tile product, in the wait for the
 * other two sub-tiles, in the diagonal-block body; number of launches; sum of their K. */
GPMI_API int gpmi_probe_fused(gpmi_ctx *ctx, double *out5);
/* Diagonal-block bodies (128-pivot factorisations) since the last call: shader cycles in the block loads, the 8-step
 * loop and the stores of tile wave 0, inside factor16 and waiting for the next diagonal tile (factor wave); bodies. */
GPMI_API int gpmi_probe_body(gpmi_ctx *ctx, double *out6);
/* One-workgroup small-N kernels since the last call (block 0 of every launch): shader cycles in the covariance
 * build, the diagonal blocks, the rows below, number of launches, cycles in the trailing tiles, in the finalize. */
GPMI_API int gpmi_probe_small(gpmi_ctx *ctx, double *out6);

/* MFMA f64 fragment-layout probe: D = A(16x4) * B(4x16) on one wave with the
 * library's fragment conventions; out256 row-major D[i][j].  Host buffers. */
GPMI_API int gpmi_probe_mfma(gpmi_ctx *ctx, const double *A64, const double *B64, double *out256);
/* Back-to-back v_mfma_f64_16x16x4_f64 issue-rate microbenchmark: achieved TFLOP/s over
 * the whole chip and (nullable) the shader clock held meanwhile, from
 * d(s_memtime)/d(s_memrealtime). */
GPMI_API int gpmi_probe_mfma_peak(gpmi_ctx *ctx, int iters, double *tflops, double *clock_mhz);
/* The product of gpmi_gp_predict_joint's chain, draws = mean 1^T + L Z, on one m x m lower factor and B columns in device
 * memory: ms2[0] = milliseconds per call of the triangular matrix-matrix kernel, ms2[1] = of a loop of B one-column
 * products (what it replaced); HIP events around `reps` repetitions each. */
GPMI_API int gpmi_probe_tril_draws(gpmi_ctx *ctx, int m, int B, int reps, double *ms2);
/* The star blocks of gpmi_joint_predict's workspace for n training times, m new times and the order mask: ms2[0] = milliseconds
 * per call of the fused builder, ms2[1] = of the gpmi_deriv_cov launches it replaces (12 at p = 3), into the same places; HIP
 * events around `reps` repetitions each. */
GPMI_API int gpmi_probe_joint_star(gpmi_ctx *ctx, int n, int m, int orders, int reps, double *ms2);
#endif /* GPMI_PROBES */

#ifdef __cplusplus
}
#endif
#endif /* GPMI_H */
