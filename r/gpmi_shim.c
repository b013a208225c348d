/*
 * gpmi_shim.c -- R `.Call()` shim over the libgpmi C ABI (include/gpmi.h).
 *
 * Reference-side binding a maintainer adds to bbbales2/gp:
 *     R CMD SHLIB -o gpmi_shim.so gpmi_shim.c -I<repo>/include -L<repo>/gp_amd/csrc -lgpmi
 *     dyn.load("gpmi_shim.so"); source("r/gpmi.R")
 * R is absent from the build image (no Rinternals.h), so this file is NOT compiled by
 * __graft_entry__.build(); it is a thin translation layer whose every code path is one
 * C-ABI call that tests/ exercise through ctypes.  tests/test_abi.py runs `gcc -fsyntax-only` over it
 * against tests/r_api/ (declarations of the R API it uses: a syntax / type check, nothing more).
 * Rules it follows:
 *   - every vector's type and length is checked against n, m, D, G, B BEFORE the ABI call (need());
 *   - arguments of .Call are shared, never modified (copy-on-modify semantics);
 *   - outputs are allocated with Rf_allocMatrix / Rf_allocVector under PROTECT;
 *   - the ABI returns a status; all C resources are released BEFORE Rf_error (a longjmp);
 *   - one lazily created context per process.  HIP does not survive fork() and cannot be
 *     re-initialised in the child: parallel::mclapply children of an R session that already
 *     used the GPU get GPMI_EFORK from every call (gpmi_create included) and the shim reports
 *     it as an R error -- use mc.cores = 1, PSOCK workers, or the grid entry point.
 */
#include <string.h>
#include <R.h>
#include <Rinternals.h>
#include <unistd.h>

#include "gpmi.h"

static gpmi_ctx *g_ctx = NULL;

static gpmi_ctx *ctx(void)
{
    /* in a forked child the parent's handle answers GPMI_EFORK by itself; it is not replaced */
    if (!g_ctx) {
        int rc = gpmi_create(&g_ctx, 0);
        if (rc) Rf_error("libgpmi: %s", gpmi_last_error());
    }
    return g_ctx;
}

/* argument validation BEFORE any pointer reaches the C ABI: a length-1 R vector where the ABI reads G doubles is
 * an out-of-bounds heap read, not an error message (nothing is allocated yet, so Rf_error may longjmp freely) */
static void need(int ok, const char *what)
{
    if (!ok) Rf_error("libgpmi shim: %s", what);
}
static int is_real(SEXP x) { return TYPEOF(x) == REALSXP; }

static void check(int rc)
{
    if (rc > 0) Rf_error("the leading minor of order %d is not positive definite", rc); /* base-R chol() wording */
    if (rc < 0) Rf_error("libgpmi: %s", gpmi_last_error());
}

/* QQard(X, Y, phi): R/kernels.R:11-19.  X n x D, Y m x D, alpha scalar, ell length 1 or D */
SEXP gpmi_R_se_cov(SEXP X, SEXP Y, SEXP alpha, SEXP ell)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), m = Rf_nrows(Y);
    need(is_real(X) && is_real(Y) && is_real(ell), "X, Y and the length-scales must be double");
    need(Rf_ncols(Y) == D, "X and Y must have the same number of columns");
    need(Rf_length(ell) == 1 || Rf_length(ell) == D, "length-scale must have length 1 or ncol(X)");
    SEXP K = PROTECT(Rf_allocMatrix(REALSXP, n, m));
    int rc = gpmi_se_cov(ctx(), REAL(X), n, n, REAL(Y), m, m, D, Rf_asReal(alpha), REAL(ell), Rf_length(ell),
                         0.0, GPMI_FULL, REAL(K), n > 0 ? n : 1);
    UNPROTECT(1);
    check(rc);
    return K;
}

/* QQ / QR / RR (x, y, phi) of R/kernels.R:22-32 and a^2 * outer(x, y, kern) of pendulum_fit.R:237-240 */
SEXP gpmi_R_deriv_cov(SEXP kind, SEXP x, SEXP y, SEXP alpha, SEXP l, SEXP flags)
{
    int n = Rf_length(x), m = Rf_length(y);
    need(is_real(x) && is_real(y), "x and y must be double");
    SEXP K = PROTECT(Rf_allocMatrix(REALSXP, n, m));
    int rc = gpmi_deriv_cov(ctx(), Rf_asInteger(kind), REAL(x), n, REAL(y), m, Rf_asReal(alpha), Rf_asReal(l),
                            Rf_asInteger(flags), REAL(K), n > 0 ? n : 1);
    UNPROTECT(1);
    check(rc);
    return K;
}

/* QQ..TT(tj, tk, l) of derivative_kernels.R:39-73 (vectors already recycled to equal length by the R wrapper) */
SEXP gpmi_R_deriv_elem(SEXP kind, SEXP tj, SEXP tk, SEXP l)
{
    R_xlen_t len = Rf_xlength(tj);
    need(is_real(tj) && is_real(tk) && Rf_xlength(tk) == len, "tj and tk must be double vectors of equal length (recycle in R)");
    SEXP out = PROTECT(Rf_allocVector(REALSXP, len));
    int rc = gpmi_deriv_elem(ctx(), Rf_asInteger(kind), REAL(tj), REAL(tk), (size_t)len, Rf_asReal(l), REAL(out));
    UNPROTECT(1);
    check(rc);
    return out;
}

/* list(L=, dLdl=) = rbf_cov_chol(x1, l_): covariance.cpp:9-47 */
SEXP gpmi_R_rbf_cov_chol(SEXP x, SEXP l)
{
    int n = Rf_length(x);
    need(is_real(x), "x must be double");
    SEXP L = PROTECT(Rf_allocMatrix(REALSXP, n, n));
    SEXP dL = PROTECT(Rf_allocMatrix(REALSXP, n, n));
    int rc = gpmi_rbf_cov_chol(ctx(), REAL(x), n, Rf_asReal(l), REAL(L), n, REAL(dL), n);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2)), names = PROTECT(Rf_allocVector(STRSXP, 2));
    SET_VECTOR_ELT(out, 0, L); SET_VECTOR_ELT(out, 1, dL);
    SET_STRING_ELT(names, 0, Rf_mkChar("L")); SET_STRING_ELT(names, 1, Rf_mkChar("dLdl"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* interp_build(x, lp): the device-resident table of L(lp[p]), dL/dl(lp[p]) that
 * test_interpolate.R:9-19 builds with P calls of rbf_cov_chol */
SEXP gpmi_R_interp_build(SEXP x, SEXP lp)
{
    need(is_real(x) && is_real(lp), "x and lp must be double");
    check(gpmi_interp_build(ctx(), REAL(x), Rf_length(x), REAL(lp), Rf_length(lp)));
    return R_NilValue;
}

/* approx_L(l, lp, Ls, dLdls): covariance.cpp:49-96.  Ls, dLdls are R lists of n x n matrices; only
 * the two table entries around l travel to the device. */
static int interval(double l, const double *lp, int P)
{
    int k = 0;
    for (; k < P - 1; ++k)
        if (lp[k + 1] >= l) break;
    return k > P - 2 ? P - 2 : k;
}
static int load_pair(double l, SEXP lp, SEXP Ls, SEXP dLdls, int *n_out)
{
    int P = Rf_length(lp);
    need(is_real(lp) && P >= 2, "lp must be a double vector of at least two length-scales");
    need(TYPEOF(Ls) == VECSXP && TYPEOF(dLdls) == VECSXP && Rf_length(Ls) == P && Rf_length(dLdls) == P,
         "Ls and dLdls must be lists with one matrix per entry of lp");
    int k = interval(l, REAL(lp), P), n = Rf_nrows(VECTOR_ELT(Ls, k));
    for (int q = k; q <= k + 1; ++q) {   /* the two table entries that travel: n x n doubles each */
        SEXP a = VECTOR_ELT(Ls, q), b = VECTOR_ELT(dLdls, q);
        need(is_real(a) && is_real(b) && Rf_nrows(a) == n && Rf_ncols(a) == n && Rf_nrows(b) == n && Rf_ncols(b) == n,
             "the entries of Ls and dLdls must be square double matrices of one order");
    }
    double *buf = (double *)R_alloc((size_t)4 * n * n, sizeof(double));  /* freed by R, also on error */
    size_t m = (size_t)n * n;
    memcpy(buf, REAL(VECTOR_ELT(Ls, k)), m * sizeof(double));
    memcpy(buf + m, REAL(VECTOR_ELT(Ls, k + 1)), m * sizeof(double));
    memcpy(buf + 2 * m, REAL(VECTOR_ELT(dLdls, k)), m * sizeof(double));
    memcpy(buf + 3 * m, REAL(VECTOR_ELT(dLdls, k + 1)), m * sizeof(double));
    double lp2[2] = {REAL(lp)[k], REAL(lp)[k + 1]};
    *n_out = n;
    return gpmi_interp_load(ctx(), lp2, 2, buf, buf + 2 * m, n, n);
}
SEXP gpmi_R_approx_L(SEXP l, SEXP lp, SEXP Ls, SEXP dLdls)
{
    int n = 0;
    check(load_pair(Rf_asReal(l), lp, Ls, dLdls, &n));
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, n));
    int rc = gpmi_approx_L(ctx(), Rf_asReal(l), REAL(out), n);
    UNPROTECT(1);
    check(rc);
    return out;
}

/* approx_Lz(l, lp, Ls, dLdls, z): models/cubic_interpolated_gp.hpp:38-73; with Ls = NULL the table of
 * gpmi_R_interp_build is used (one call per leapfrog step, nothing but z crosses PCIe) */
SEXP gpmi_R_approx_Lz(SEXP l, SEXP lp, SEXP Ls, SEXP dLdls, SEXP z)
{
    int n = Rf_length(z), nz = n;
    need(is_real(z), "z must be double");
    if (!Rf_isNull(Ls)) check(load_pair(Rf_asReal(l), lp, Ls, dLdls, &n));
    need(n == nz, "z must have the order of the table's matrices");   /* (a device-resident table checks z in gpmi.R) */
    SEXP f = PROTECT(Rf_allocVector(REALSXP, n));
    int rc = gpmi_approx_Lz(ctx(), Rf_asReal(l), REAL(z), REAL(f));
    UNPROTECT(1);
    check(rc);
    return f;
}

/* list(f = approx_L(l) z, dfdl = (dv/dl) z): value and the reverse-mode partial of the Stan external function
 * (`var` overload of build_output, models/cubic_interpolated_gp.hpp:6-32, dvdl :67) */
SEXP gpmi_R_approx_Lz_grad(SEXP l, SEXP lp, SEXP Ls, SEXP dLdls, SEXP z)
{
    int n = Rf_length(z), nz = n;
    need(is_real(z), "z must be double");
    if (!Rf_isNull(Ls)) check(load_pair(Rf_asReal(l), lp, Ls, dLdls, &n));
    need(n == nz, "z must have the order of the table's matrices");
    SEXP f = PROTECT(Rf_allocVector(REALSXP, n)), g = PROTECT(Rf_allocVector(REALSXP, n));
    int rc = gpmi_approx_Lz_grad(ctx(), Rf_asReal(l), REAL(z), REAL(f), REAL(g));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2)), names = PROTECT(Rf_allocVector(STRSXP, 2));
    SET_VECTOR_ELT(out, 0, f); SET_VECTOR_ELT(out, 1, g);
    SET_STRING_ELT(names, 0, Rf_mkChar("f")); SET_STRING_ELT(names, 1, Rf_mkChar("dfdl"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* list(f, zbar, lbar) of F = A(l) Z with upstream adjoint Fbar (z, fbar: n-vectors or n x k matrices; f and zbar come
 * back with z's shape) for the Hermite table (model 0) or the GP-regression table (model 1) */
static SEXP tri_vjp(int model, double l, SEXP z, SEXP fbar, int n)
{
    need(is_real(z) && is_real(fbar) && Rf_length(fbar) == Rf_length(z), "z and fbar must be double and of one shape");
    need(n > 0 && Rf_length(z) % n == 0 && Rf_length(z) > 0, "length(z) must be a multiple of the table's order");
    int k = Rf_length(z) / n;
    SEXP f = PROTECT(Rf_duplicate(z)), zb = PROTECT(Rf_duplicate(z)), lb = PROTECT(Rf_allocVector(REALSXP, 1));
    int rc = (model ? gpmi_interp_gp_Lz_vjp : gpmi_approx_Lz_vjp)(ctx(), l, REAL(z), k, n, REAL(fbar), n, REAL(f), n, REAL(zb),
                                                                  n, REAL(lb));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3)), names = PROTECT(Rf_allocVector(STRSXP, 3));
    SET_VECTOR_ELT(out, 0, f); SET_VECTOR_ELT(out, 1, zb); SET_VECTOR_ELT(out, 2, lb);
    SET_STRING_ELT(names, 0, Rf_mkChar("f")); SET_STRING_ELT(names, 1, Rf_mkChar("zbar")); SET_STRING_ELT(names, 2, Rf_mkChar("lbar"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(5);
    check(rc);
    return out;
}

/* list(f, zbar = t(approx_L(l)) fbar, lbar = sum(fbar * (dv/dl) z)): models/cubic_interpolated_gp.hpp:6-32,38-73 under
 * reverse mode; with Ls = NULL the table of gpmi_R_interp_build is used (n: its order) */
SEXP gpmi_R_approx_Lz_vjp(SEXP l, SEXP lp, SEXP Ls, SEXP dLdls, SEXP z, SEXP fbar, SEXP n_table)
{
    int n = Rf_asInteger(n_table);
    if (!Rf_isNull(Ls)) check(load_pair(Rf_asReal(l), lp, Ls, dLdls, &n));
    return tri_vjp(0, Rf_asReal(l), z, fbar, n);
}

/* the GP-regression table of models/interpolated_gp.stan:9-27: lookup = (Sigma_P \ exact)^T on the device */
SEXP gpmi_R_interp_gp_build(SEXP x, SEXP lp, SEXP rho, SEXP jitter)
{
    need(is_real(x) && is_real(lp), "x and lp must be double");
    check(gpmi_interp_gp_build(ctx(), REAL(x), Rf_length(x), REAL(lp), Rf_length(lp), Rf_asReal(rho), Rf_asReal(jitter)));
    return R_NilValue;
}

/* f = L(l) z, L(l) = to_matrix(lookup * Kp(l), N, N) (models/interpolated_gp.stan:39-44) */
SEXP gpmi_R_interp_gp_Lz(SEXP l, SEXP z, SEXP n_table)
{
    int n = Rf_asInteger(n_table);
    need(is_real(z) && n > 0 && Rf_length(z) % n == 0 && Rf_length(z) > 0, "z must be double with a multiple of n entries");
    SEXP f = PROTECT(Rf_duplicate(z));
    int rc = gpmi_interp_gp_Lz(ctx(), Rf_asReal(l), REAL(z), Rf_length(z) / n, n, REAL(f), n);
    UNPROTECT(1);
    check(rc);
    return f;
}

/* list(f, zbar = t(L(l)) fbar, lbar = sum(fbar * (dL/dl) z)) of the same */
SEXP gpmi_R_interp_gp_Lz_vjp(SEXP l, SEXP z, SEXP fbar, SEXP n_table)
{
    return tri_vjp(1, Rf_asReal(l), z, fbar, Rf_asInteger(n_table));
}

/* c(logml, sum log L_ii, z'z): one evaluation of models/fit_hyperparameters.stan:18-32 */
SEXP gpmi_R_logml(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X);
    need(is_real(X) && is_real(y) && is_real(ell), "X, y and the length-scales must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_length(ell) == 1 || Rf_length(ell) == D, "length-scale must have length 1 or ncol(X)");
    SEXP out = PROTECT(Rf_allocVector(REALSXP, 3));
    int rc = gpmi_logml(ctx(), REAL(X), n, n, D, REAL(y), Rf_asReal(alpha), REAL(ell), Rf_length(ell),
                        Rf_asReal(sigma), Rf_asReal(jitter), REAL(out));
    UNPROTECT(1);
    check(rc);
    return out;
}

/* f = cholesky_decompose(cov_exp_quad(X, alpha, ell) + jitter I) z: the transform of models/exact_gp.stan:17-25 */
SEXP gpmi_R_exact_gp_f(SEXP X, SEXP alpha, SEXP ell, SEXP jitter, SEXP z)
{
    int n = Rf_nrows(X), D = Rf_ncols(X);
    need(is_real(X) && is_real(z) && is_real(ell), "X, z and the length-scales must be double");
    need(Rf_length(z) == n, "length(z) must equal nrow(X)");
    need(Rf_length(ell) == 1 || Rf_length(ell) == D, "length-scale must have length 1 or ncol(X)");
    SEXP out = PROTECT(Rf_allocVector(REALSXP, n));
    int rc = gpmi_exact_gp_f(ctx(), REAL(X), n, n, D, Rf_asReal(alpha), REAL(ell), Rf_length(ell), Rf_asReal(jitter), REAL(z),
                             REAL(out));
    UNPROTECT(1);
    check(rc);
    return out;
}

/* list(f, zbar, grad): the vector-Jacobian product of that transform -- what reverse-mode autodiff needs of
 * models/exact_gp.stan:17-25 and models/heteroscedastic.stan:23-32 per leapfrog step.  z, fbar: n-vectors or n x k
 * matrices (f, zbar come back with z's shape); grad = c(d/dalpha, d/dell...) of sum(fbar * f). */
SEXP gpmi_R_exact_gp_f_vjp(SEXP X, SEXP alpha, SEXP ell, SEXP jitter, SEXP z, SEXP fbar)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), ne = Rf_length(ell);
    need(is_real(X) && is_real(z) && is_real(fbar) && is_real(ell), "X, z, fbar and the length-scales must be double");
    need(n > 0 && Rf_length(z) % n == 0 && Rf_length(z) > 0, "length(z) must be a multiple of nrow(X)");
    need(Rf_length(fbar) == Rf_length(z), "fbar must have the shape of z");
    need(ne == 1 || ne == D, "length-scale must have length 1 or ncol(X)");
    int k = Rf_length(z) / n;
    SEXP f = PROTECT(Rf_duplicate(z)), zb = PROTECT(Rf_duplicate(z)), g = PROTECT(Rf_allocVector(REALSXP, 1 + ne));
    int rc = gpmi_exact_gp_f_vjp(ctx(), REAL(X), n, n, D, Rf_asReal(alpha), REAL(ell), ne, Rf_asReal(jitter), REAL(z), k, n,
                                 REAL(fbar), n, REAL(f), n, REAL(zb), n, REAL(g));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3)), names = PROTECT(Rf_allocVector(STRSXP, 3));
    SET_VECTOR_ELT(out, 0, f); SET_VECTOR_ELT(out, 1, zb); SET_VECTOR_ELT(out, 2, g);
    SET_STRING_ELT(names, 0, Rf_mkChar("f")); SET_STRING_ELT(names, 1, Rf_mkChar("zbar")); SET_STRING_ELT(names, 2, Rf_mkChar("grad"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(5);
    check(rc);
    return out;
}

/* list(lik, dlik_dsigma, f, fbar, zbar, grad): the likelihood part of a latent exact-GP model's lp__ and its gradient in one
 * call with one factorisation (gpmi_latent_gp_lp_grad).  family: 0 normal, 1 bernoulli_logit, 2 normal_logsd (z n x 2);
 * y: n-vector or n x m matrix of replicates. */
SEXP gpmi_R_latent_gp_lp_grad(SEXP X, SEXP alpha, SEXP ell, SEXP jitter, SEXP z, SEXP family, SEXP y, SEXP sigma)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), ne = Rf_length(ell);
    need(is_real(X) && is_real(z) && is_real(y) && is_real(ell), "X, z, y and the length-scales must be double");
    need(n > 0 && Rf_length(z) % n == 0 && Rf_length(z) > 0, "length(z) must be a multiple of nrow(X)");
    need(Rf_length(y) % n == 0 && Rf_length(y) > 0, "length(y) must be a multiple of nrow(X)");
    need(ne == 1 || ne == D, "length-scale must have length 1 or ncol(X)");
    int k = Rf_length(z) / n, m = Rf_length(y) / n;
    SEXP f = PROTECT(Rf_duplicate(z)), fb = PROTECT(Rf_duplicate(z)), zb = PROTECT(Rf_duplicate(z));
    SEXP g = PROTECT(Rf_allocVector(REALSXP, 1 + ne)), lik = PROTECT(Rf_allocVector(REALSXP, 1)), ds = PROTECT(Rf_allocVector(REALSXP, 1));
    double o2[2] = {0.0, 0.0};
    int rc = gpmi_latent_gp_lp_grad(ctx(), REAL(X), n, n, D, Rf_asReal(alpha), REAL(ell), ne, Rf_asReal(jitter), REAL(z), k, n,
                                    Rf_asInteger(family), REAL(y), m, n, Rf_asReal(sigma), o2, REAL(f), n, REAL(fb), n, REAL(zb), n,
                                    REAL(g));
    static const char *nm[6] = {"lik", "dlik_dsigma", "f", "fbar", "zbar", "grad"};
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 6)), names = PROTECT(Rf_allocVector(STRSXP, 6));
    REAL(lik)[0] = o2[0]; REAL(ds)[0] = o2[1];
    SET_VECTOR_ELT(out, 0, lik); SET_VECTOR_ELT(out, 1, ds);
    SET_VECTOR_ELT(out, 2, f); SET_VECTOR_ELT(out, 3, fb); SET_VECTOR_ELT(out, 4, zb); SET_VECTOR_ELT(out, 5, g);
    for (int i = 0; i < 6; ++i) SET_STRING_ELT(names, i, Rf_mkChar(nm[i]));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(8);
    check(rc);
    return out;
}

/* list(lp, dlik_dsigma, sum_log_diag, quad, fgrad, grad): the centred latent GP's log-density and gradient in one call with one
 * factorisation (gpmi_centered_gp_lp_grad; models/heteroscedastic_centered.stan:24-34).  f: the latent columns (n-vector or
 * n x k); family: 0 normal, 1 bernoulli_logit, 2 normal_logsd (f n x 2), 3 none (the prior alone: y is not read). */
SEXP gpmi_R_centered_gp_lp_grad(SEXP X, SEXP alpha, SEXP ell, SEXP jitter, SEXP f, SEXP family, SEXP y, SEXP sigma)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), ne = Rf_length(ell), fam = Rf_asInteger(family);
    need(is_real(X) && is_real(f) && is_real(ell), "X, f and the length-scales must be double");
    need(n > 0 && Rf_length(f) % n == 0 && Rf_length(f) > 0, "length(f) must be a multiple of nrow(X)");
    need(fam == GPMI_LIK_NONE || (is_real(y) && Rf_length(y) % n == 0 && Rf_length(y) > 0),
         "y must be double and length(y) a multiple of nrow(X)");
    need(ne == 1 || ne == D, "length-scale must have length 1 or ncol(X)");
    int k = Rf_length(f) / n, m = fam == GPMI_LIK_NONE ? 0 : Rf_length(y) / n;
    SEXP fg = PROTECT(Rf_duplicate(f)), g = PROTECT(Rf_allocVector(REALSXP, 1 + ne));
    double o4[4] = {0.0, 0.0, 0.0, 0.0};
    int rc = gpmi_centered_gp_lp_grad(ctx(), REAL(X), n, n, D, Rf_asReal(alpha), REAL(ell), ne, Rf_asReal(jitter), REAL(f), k, n, fam,
                                      fam == GPMI_LIK_NONE ? NULL : REAL(y), m, n, Rf_asReal(sigma), o4, REAL(fg), n, REAL(g));
    static const char *nm[6] = {"lp", "dlik_dsigma", "sum_log_diag", "quad", "fgrad", "grad"};
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 6)), names = PROTECT(Rf_allocVector(STRSXP, 6));
    for (int i = 0; i < 4; ++i) {
        SEXP v = PROTECT(Rf_allocVector(REALSXP, 1));
        REAL(v)[0] = o4[i];
        SET_VECTOR_ELT(out, i, v);
        UNPROTECT(1);
    }
    SET_VECTOR_ELT(out, 4, fg); SET_VECTOR_ELT(out, 5, g);
    for (int i = 0; i < 6; ++i) SET_STRING_ELT(names, i, Rf_mkChar(nm[i]));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* list(value = c(logml, sum log L_ii, z'z), grad = c(d/dalpha, d/dell..., d/dsigma)): what Stan's
 * autodiff computes per leapfrog step for models/fit_hyperparameters.stan:18-32 */
SEXP gpmi_R_logml_grad(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), ne = Rf_length(ell);
    need(is_real(X) && is_real(y) && is_real(ell), "X, y and the length-scales must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(ne == 1 || ne == D, "length-scale must have length 1 or ncol(X)");
    SEXP val = PROTECT(Rf_allocVector(REALSXP, 3)), g = PROTECT(Rf_allocVector(REALSXP, 2 + ne));
    int rc = gpmi_logml_grad(ctx(), REAL(X), n, n, D, REAL(y), Rf_asReal(alpha), REAL(ell), ne,
                             Rf_asReal(sigma), Rf_asReal(jitter), REAL(val), REAL(g));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2)), names = PROTECT(Rf_allocVector(STRSXP, 2));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g);
    SET_STRING_ELT(names, 0, Rf_mkChar("value")); SET_STRING_ELT(names, 1, Rf_mkChar("grad"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* approx_L(M, scale, x, sigma, l) of models/westbrook.stan:2-30 (and bH of spectral_test.R:6-27): the n x M Hermite-eigenfunction
 * basis with Phi Phi' -> sigma^2 exp(-(x_i - x_j)^2 / (2 l^2)); `sigma` is the models' amplitude argument (gpmi.h: amp) */
SEXP gpmi_R_hermite_basis(SEXP M, SEXP scale, SEXP x, SEXP amp, SEXP l)
{
    int n = Rf_length(x), m = Rf_asInteger(M);
    need(is_real(x), "x must be double");
    need(n >= 1 && m >= 1 && m <= GPMI_LR_MMAX, "need length(x) >= 1 and M in 1..128");
    SEXP Phi = PROTECT(Rf_allocMatrix(REALSXP, n, m));
    int rc = gpmi_hermite_basis(ctx(), REAL(x), n, m, Rf_asReal(scale), Rf_asReal(amp), Rf_asReal(l), REAL(Phi), n, NULL, 0);
    UNPROTECT(1);
    check(rc);
    return Phi;
}

/* list(value = c(logml, 1/2 log|Sigma|, y' Sigma^-1 y), grad = c(d/damp, d/dl, d/dsigma)) of y ~ N(0, Phi Phi' + sigma^2 I) with
 * Phi the basis above (gpmi_lowrank_logml_grad) */
SEXP gpmi_R_lowrank_logml_grad(SEXP x, SEXP y, SEXP M, SEXP scale, SEXP amp, SEXP l, SEXP sigma)
{
    int n = Rf_length(x), m = Rf_asInteger(M);
    need(is_real(x) && is_real(y), "x and y must be double");
    need(Rf_length(y) == n, "length(y) must equal length(x)");
    SEXP val = PROTECT(Rf_allocVector(REALSXP, 3)), g = PROTECT(Rf_allocVector(REALSXP, 3));
    int rc = gpmi_lowrank_logml_grad(ctx(), REAL(x), n, REAL(y), m, Rf_asReal(scale), Rf_asReal(amp), Rf_asReal(l), Rf_asReal(sigma),
                                     REAL(val), REAL(g));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2)), names = PROTECT(Rf_allocVector(STRSXP, 2));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g);
    SET_STRING_ELT(names, 0, Rf_mkChar("value")); SET_STRING_ELT(names, 1, Rf_mkChar("grad"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* exact leave-one-out cross-validation (gpmi_logml_loo): list(value = c(logml, sum log L_ii, z'z), loo = sum(lpd), mu, var, lpd
 * (length n: mean, variance of the observation and log density of y_i given the others), grad = d loo / d(alpha, ell.., sigma)
 * or NULL when want_grad is 0) */
SEXP gpmi_R_logml_loo(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter, SEXP want_grad)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), ne = Rf_length(ell), wg = Rf_asInteger(want_grad) != 0;
    need(is_real(X) && is_real(y) && is_real(ell), "X, y and the length-scales must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(ne == 1 || ne == D, "length-scale must have length 1 or ncol(X)");
    SEXP val = PROTECT(Rf_allocVector(REALSXP, 3)), loo = PROTECT(Rf_allocVector(REALSXP, 1));
    SEXP mu = PROTECT(Rf_allocVector(REALSXP, n)), var = PROTECT(Rf_allocVector(REALSXP, n)), lpd = PROTECT(Rf_allocVector(REALSXP, n));
    SEXP g = PROTECT(wg ? Rf_allocVector(REALSXP, 2 + ne) : R_NilValue);
    int rc = gpmi_logml_loo(ctx(), REAL(X), n, n, D, REAL(y), Rf_asReal(alpha), REAL(ell), ne, Rf_asReal(sigma), Rf_asReal(jitter),
                            REAL(val), REAL(loo), REAL(mu), REAL(var), REAL(lpd), wg ? REAL(g) : NULL);
    static const char *nm[6] = {"value", "loo", "mu", "var", "lpd", "grad"};
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 6)), names = PROTECT(Rf_allocVector(STRSXP, 6));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, loo); SET_VECTOR_ELT(out, 2, mu); SET_VECTOR_ELT(out, 3, var);
    SET_VECTOR_ELT(out, 4, lpd); SET_VECTOR_ELT(out, 5, g);
    for (int i = 0; i < 6; ++i) SET_STRING_ELT(names, i, Rf_mkChar(nm[i]));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(8);
    check(rc);
    return out;
}

/* value, gradient and exact Hessian in (alpha, ell.., sigma) (gpmi_logml_hess): list(value = c(logml, sum log L_ii, z'z), grad,
 * hess = the q x q matrix of second derivatives, q = 2 + length(ell)) */
SEXP gpmi_R_logml_hess(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), ne = Rf_length(ell), q = 2 + ne;
    need(is_real(X) && is_real(y) && is_real(ell), "X, y and the length-scales must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(ne == 1 || ne == D, "length-scale must have length 1 or ncol(X)");
    SEXP val = PROTECT(Rf_allocVector(REALSXP, 3)), g = PROTECT(Rf_allocVector(REALSXP, q)), H = PROTECT(Rf_allocMatrix(REALSXP, q, q));
    int rc = gpmi_logml_hess(ctx(), REAL(X), n, n, D, REAL(y), Rf_asReal(alpha), REAL(ell), ne, Rf_asReal(sigma), Rf_asReal(jitter),
                             REAL(val), REAL(g), REAL(H), q);
    static const char *nm[3] = {"value", "grad", "hess"};
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3)), names = PROTECT(Rf_allocVector(STRSXP, 3));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g); SET_VECTOR_ELT(out, 2, H);
    for (int i = 0; i < 3; ++i) SET_STRING_ELT(names, i, Rf_mkChar(nm[i]));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(5);
    check(rc);
    return out;
}

/* value + gradient at G points (one per chain): list(value = 3 x G, grad = 3 x G (d/dalpha, d/drho, d/dsigma), info) */
SEXP gpmi_R_logml_grad_grid(SEXP X, SEXP y, SEXP alpha, SEXP rho, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), G = Rf_length(rho);
    need(is_real(X) && is_real(y) && is_real(alpha) && is_real(rho) && is_real(sigma), "X, y, alpha, rho, sigma must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_length(alpha) == G && Rf_length(sigma) == G, "alpha, rho and sigma must have one entry per grid point (recycle in R)");
    SEXP val = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), g = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), info = PROTECT(Rf_allocVector(INTSXP, G));
    int rc = gpmi_logml_grad_grid(ctx(), REAL(X), n, n, D, REAL(y), REAL(alpha), REAL(rho), REAL(sigma), G, Rf_asReal(jitter),
                                  REAL(val), REAL(g), INTEGER(info));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g); SET_VECTOR_ELT(out, 2, info);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* ... at G points with one length-scale per dimension each (ell: D x G, column g = the length-scales of point g): an unnamed
 * list of value (3 x G), grad ((D + 2) x G: d/dalpha, d/dell_1 .. d/dell_D, d/dsigma per column) and info (G) */
SEXP gpmi_R_logml_grad_grid_ard(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), G = Rf_ncols(ell);
    need(is_real(X) && is_real(y) && is_real(alpha) && is_real(ell) && is_real(sigma), "X, y, alpha, ell, sigma must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_nrows(ell) == D, "ell must be ncol(X) x (grid points)");
    need(Rf_length(alpha) == G && Rf_length(sigma) == G, "alpha and sigma must have one entry per grid point (recycle in R)");
    SEXP val = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), g = PROTECT(Rf_allocMatrix(REALSXP, D + 2, G)), info = PROTECT(Rf_allocVector(INTSXP, G));
    int rc = gpmi_logml_grad_grid_ard(ctx(), REAL(X), n, n, D, REAL(y), REAL(alpha), REAL(ell), REAL(sigma), G, Rf_asReal(jitter),
                                      REAL(val), REAL(g), INTEGER(info));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g); SET_VECTOR_ELT(out, 2, info);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* the joint [y; y'] model (R/ode_gp_library.R:29-30): list(value = c(logml, sum log L_ii, z'z), grad = c(d/dalpha, d/dl,
 * d/dsigma) of logml) through one factorisation of the order-2n matrix; yy = c(y, y') */
SEXP gpmi_R_joint_logml_grad(SEXP t, SEXP yy, SEXP alpha, SEXP l, SEXP sigma, SEXP jitter)
{
    int n = Rf_length(t);
    need(is_real(t) && is_real(yy), "t and yy must be double");
    need(Rf_length(yy) == 2 * n, "yy must stack c(y, y'): length 2 * length(t)");
    SEXP val = PROTECT(Rf_allocVector(REALSXP, 3)), g = PROTECT(Rf_allocVector(REALSXP, 3));
    int rc = gpmi_joint_logml_grad(ctx(), REAL(t), n, REAL(yy), Rf_asReal(alpha), Rf_asReal(l), Rf_asReal(sigma), Rf_asReal(jitter),
                                   REAL(val), REAL(g));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2)), names = PROTECT(Rf_allocVector(STRSXP, 2));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g);
    SET_STRING_ELT(names, 0, Rf_mkChar("value")); SET_STRING_ELT(names, 1, Rf_mkChar("grad"));
    Rf_setAttrib(out, R_NamesSymbol, names);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* ... at G points (one per chain): an unnamed list of value (3 x G), grad (3 x G) and info (G), as gpmi_R_logml_grad_grid */
SEXP gpmi_R_joint_logml_grad_grid(SEXP t, SEXP yy, SEXP alpha, SEXP l, SEXP sigma, SEXP jitter)
{
    int n = Rf_length(t), G = Rf_length(l);
    need(is_real(t) && is_real(yy) && is_real(alpha) && is_real(l) && is_real(sigma), "t, yy, alpha, l, sigma must be double");
    need(Rf_length(yy) == 2 * n, "yy must stack c(y, y'): length 2 * length(t)");
    need(Rf_length(alpha) == G && Rf_length(sigma) == G, "alpha, l and sigma must have one entry per grid point (recycle in R)");
    SEXP val = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), g = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), info = PROTECT(Rf_allocVector(INTSXP, G));
    int rc = gpmi_joint_logml_grad_grid(ctx(), REAL(t), n, REAL(yy), REAL(alpha), REAL(l), REAL(sigma), G, Rf_asReal(jitter),
                                        REAL(val), REAL(g), INTEGER(info));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, val); SET_VECTOR_ELT(out, 1, g); SET_VECTOR_ELT(out, 2, info);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* G x 3 matrix + info for a hyper-parameter grid (non-PD points NaN, grid continues) */
SEXP gpmi_R_logml_grid(SEXP X, SEXP y, SEXP alpha, SEXP rho, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), G = Rf_length(rho);
    need(is_real(X) && is_real(y) && is_real(alpha) && is_real(rho) && is_real(sigma), "X, y, alpha, rho, sigma must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_length(alpha) == G && Rf_length(sigma) == G, "alpha, rho and sigma must have one entry per grid point (recycle in R)");
    SEXP res = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), info = PROTECT(Rf_allocVector(INTSXP, G));
    int rc = gpmi_logml_grid(ctx(), REAL(X), n, n, D, REAL(y), REAL(alpha), REAL(rho), REAL(sigma), G,
                             Rf_asReal(jitter), REAL(res), INTEGER(info));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, res); SET_VECTOR_ELT(out, 1, info);
    UNPROTECT(3);
    check(rc);
    return out;
}

/* the same grid with a length-scale per dimension and point: ell is a D x G matrix (column g = point g), QQard's vector
 * phi[[2]] (R/kernels.R:11-19) */
SEXP gpmi_R_logml_grid_ard(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), G = Rf_ncols(ell);
    need(is_real(X) && is_real(y) && is_real(alpha) && is_real(ell) && is_real(sigma), "X, y, alpha, ell, sigma must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_nrows(ell) == D, "ell must be ncol(X) x (grid points)");
    need(Rf_length(alpha) == G && Rf_length(sigma) == G, "alpha and sigma must have one entry per grid point (recycle in R)");
    SEXP res = PROTECT(Rf_allocMatrix(REALSXP, 3, G)), info = PROTECT(Rf_allocVector(INTSXP, G));
    int rc = gpmi_logml_grid_ard(ctx(), REAL(X), n, n, D, REAL(y), REAL(alpha), REAL(ell), REAL(sigma), G, Rf_asReal(jitter),
                                 REAL(res), INTEGER(info));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, res); SET_VECTOR_ELT(out, 1, info);
    UNPROTECT(3);
    check(rc);
    return out;
}

/* list(mn, Kn): p_Xn / p_dotXn (R/ode_gp.R:1-32, R/ode_gp_library.R:4-33), sample_derivs moments
 * (pendulum_fit.R:242-251) */
SEXP gpmi_R_gp_condition(SEXP t, SEXP ts, SEXP y, SEXP alpha, SEXP l, SEXP s2, SEXP jitter, SEXP kinds, SEXP flags)
{
    int n = Rf_length(t), m = Rf_length(ts);
    need(is_real(t) && is_real(ts) && is_real(y), "t, ts and y must be double");
    need(Rf_length(y) == n, "length(y) must equal length(t)");
    need(TYPEOF(kinds) == INTSXP && Rf_length(kinds) == 3, "kinds must be three integers (K, Ks, Kss)");
    int *k = INTEGER(kinds);
    SEXP mn = PROTECT(Rf_allocMatrix(REALSXP, m, 1)), Kn = PROTECT(Rf_allocMatrix(REALSXP, m, m));
    int rc = gpmi_gp_condition(ctx(), REAL(t), n, REAL(ts), m, REAL(y), Rf_asReal(alpha), Rf_asReal(l), Rf_asReal(s2),
                               Rf_asReal(jitter), k[0], k[1], k[2], Rf_asInteger(flags), REAL(mn), REAL(Kn), m);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, mn); SET_VECTOR_ELT(out, 1, Kn);
    UNPROTECT(3);
    check(rc);
    return out;
}

/* list(mean, var): pointwise posterior of the latent function at the rows of Xs under QQard(X, X, theta) + (sigma^2 + jitter) I
 * (what create_p_dotXnS conditions on, R/ode_gp_library.R:43-93); var is alpha^2 - k' Sigma^-1 k as computed */
SEXP gpmi_R_gp_predict(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter, SEXP Xs)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), m = Rf_nrows(Xs);
    need(is_real(X) && is_real(y) && is_real(ell) && is_real(Xs), "X, y, the length-scales and Xs must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_ncols(Xs) == D, "Xs must have ncol(X) columns");
    need(Rf_length(ell) == 1 || Rf_length(ell) == D, "length-scale must have length 1 or ncol(X)");
    SEXP mean = PROTECT(Rf_allocVector(REALSXP, m)), var = PROTECT(Rf_allocVector(REALSXP, m));
    int rc = gpmi_gp_predict(ctx(), REAL(X), n, n, D, REAL(y), Rf_asReal(alpha), REAL(ell), Rf_length(ell), Rf_asReal(sigma),
                             Rf_asReal(jitter), REAL(Xs), m, m, REAL(mean), REAL(var));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, mean); SET_VECTOR_ELT(out, 1, var);
    UNPROTECT(3);
    check(rc);
    return out;
}

/* list(mean, cov, draws): the JOINT posterior of the latent function at the rows of Xs under the same model -- cov = K(Xs, Xs) -
 * Ks Sigma^-1 Ks' + post_jitter I (m x m) and draws = mean + chol(cov) Z for the caller's Z = matrix(rnorm(m * B), m, B) (R's own
 * RNG stream); Z with zero columns: no draws, cov is not factored */
SEXP gpmi_R_gp_predict_joint(SEXP X, SEXP y, SEXP alpha, SEXP ell, SEXP sigma, SEXP jitter, SEXP Xs, SEXP post_jitter, SEXP Z)
{
    int n = Rf_nrows(X), D = Rf_ncols(X), m = Rf_nrows(Xs), B = Rf_ncols(Z);
    need(is_real(X) && is_real(y) && is_real(ell) && is_real(Xs) && is_real(Z), "X, y, the length-scales, Xs and Z must be double");
    need(Rf_length(y) == n, "length(y) must equal nrow(X)");
    need(Rf_ncols(Xs) == D, "Xs must have ncol(X) columns");
    need(Rf_length(ell) == 1 || Rf_length(ell) == D, "length-scale must have length 1 or ncol(X)");
    need(Rf_nrows(Z) == m, "Z must have nrow(Xs) rows");
    SEXP mean = PROTECT(Rf_allocVector(REALSXP, m)), cov = PROTECT(Rf_allocMatrix(REALSXP, m, m)),
         draws = PROTECT(Rf_allocMatrix(REALSXP, m, B));
    int rc = gpmi_gp_predict_joint(ctx(), REAL(X), n, n, D, REAL(y), Rf_asReal(alpha), REAL(ell), Rf_length(ell), Rf_asReal(sigma),
                                   Rf_asReal(jitter), REAL(Xs), m, m, Rf_asReal(post_jitter), REAL(mean), REAL(cov), m,
                                   B > 0 ? REAL(Z) : NULL, B, m, B > 0 ? REAL(draws) : NULL, m);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, mean); SET_VECTOR_ELT(out, 1, cov); SET_VECTOR_ELT(out, 2, draws);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* list(mean, cov, draws): the posterior of f, f', f'' at the times ts given yy = c(y, yp) at the times t under the joint model
 * of gpmi_R_joint_logml -- orders: bit mask (1 f, 2 f', 4 f''), every result stacked by order; post_jitter: one value per
 * requested order; Z = matrix(rnorm(p m B), p m, B) (R's own RNG stream); Z with zero columns: no draws, cov is not factored */
SEXP gpmi_R_joint_predict(SEXP t, SEXP yy, SEXP alpha, SEXP l, SEXP sigma, SEXP jitter, SEXP ts, SEXP orders, SEXP post_jitter, SEXP Z)
{
    int n = Rf_length(t), m = Rf_length(ts), ord = Rf_asInteger(orders), B = Rf_ncols(Z);
    need(is_real(t) && is_real(yy) && is_real(ts) && is_real(post_jitter) && is_real(Z), "t, yy, ts, post_jitter and Z must be double");
    need(ord >= 1 && ord <= 7, "orders must be a bit mask in 1..7");
    int p = (ord & 1) + ((ord >> 1) & 1) + ((ord >> 2) & 1), pm = p * m;
    need(Rf_length(yy) == 2 * n, "length(yy) must equal 2 * length(t)");
    need(Rf_length(post_jitter) == p, "post_jitter must hold one value per requested order");
    need(Rf_nrows(Z) == pm, "Z must have one row per requested order and time");
    SEXP mean = PROTECT(Rf_allocVector(REALSXP, pm)), cov = PROTECT(Rf_allocMatrix(REALSXP, pm, pm)),
         draws = PROTECT(Rf_allocMatrix(REALSXP, pm, B));
    int rc = gpmi_joint_predict(ctx(), REAL(t), n, REAL(yy), Rf_asReal(alpha), Rf_asReal(l), Rf_asReal(sigma), Rf_asReal(jitter),
                                REAL(ts), m, ord, REAL(post_jitter), REAL(mean), REAL(cov), pm, B > 0 ? REAL(Z) : NULL, B, pm,
                                B > 0 ? REAL(draws) : NULL, pm);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, mean); SET_VECTOR_ELT(out, 1, cov); SET_VECTOR_ELT(out, 2, draws);
    UNPROTECT(4);
    check(rc);
    return out;
}

/* sample_derivs(params, ynoise, ti): pendulum_fit.R:227-255, one draw mu + chol(cov) z fused on the device; z = rnorm(m)
 * comes from R's own RNG (the reference's MASS::mvrnorm stream cannot be reproduced: eigen-decomposition draw) */
SEXP gpmi_R_sample_derivs(SEXP t, SEXP ts, SEXP y, SEXP params, SEXP jitter, SEXP z)
{
    int n = Rf_length(t), m = Rf_length(ts);
    need(is_real(t) && is_real(ts) && is_real(y) && is_real(params) && is_real(z), "t, ts, y, params and z must be double");
    need(Rf_length(y) == n, "length(ynoise) must equal length(ti)");
    need(Rf_length(z) == m, "length(z) must equal the number of prediction times");
    need(Rf_length(params) >= 3, "params must hold (l, a, sy)");
    double *p = REAL(params);
    SEXP draw = PROTECT(Rf_allocVector(REALSXP, m));
    int rc = gpmi_sample_derivs(ctx(), REAL(t), n, REAL(ts), m, REAL(y), p[0], p[1], p[2], Rf_asReal(jitter), REAL(z),
                                REAL(draw), NULL);
    UNPROTECT(1);
    check(rc);
    return draw;
}

/* the loop mclapply(s_list[1:100], sample_derivs_both_states, mc.cores = 2) of pendulum_fit.R:261-268 as ONE call:
 * params 3 x B, Y n x B, Z m x B -> draws m x B (independent conditionings on the GPU's lanes) */
SEXP gpmi_R_sample_derivs_batch(SEXP t, SEXP ts, SEXP Y, SEXP params, SEXP jitter, SEXP Z)
{
    int n = Rf_length(t), m = Rf_length(ts), B = Rf_ncols(Y);
    need(is_real(t) && is_real(ts) && is_real(Y) && is_real(params) && is_real(Z), "t, ts, Y, params and Z must be double");
    need(Rf_nrows(Y) == n, "nrow(Y) must equal length(ti)");
    need(Rf_nrows(Z) == m && Rf_ncols(Z) == B, "Z must be (prediction times) x (draws)");
    need(Rf_nrows(params) == 3 && Rf_ncols(params) == B, "params must be 3 x (draws): rows l, a, sy");
    SEXP draws = PROTECT(Rf_allocMatrix(REALSXP, m, B));
    int *info = (int *)R_alloc(B > 0 ? B : 1, sizeof(int));
    int rc = gpmi_sample_derivs_batch(ctx(), REAL(t), n, REAL(ts), m, REAL(Y), n, REAL(params), B, Rf_asReal(jitter), REAL(Z),
                                      m, REAL(draws), m, NULL, 0, info);
    UNPROTECT(1);
    check(rc);
    for (int b = 0; b < B; ++b) check(info[b]);
    return draws;
}

/* t(chol(A)) replacement: lower factor, upper zeroed (Stan convention); base-R chol() is t() of this */
SEXP gpmi_R_potrf(SEXP A)
{
    int n = Rf_nrows(A);
    need(is_real(A) && Rf_ncols(A) == n, "A must be a square double matrix");
    SEXP L = PROTECT(Rf_duplicate(A)); /* never modify a .Call argument */
    int rc = gpmi_potrf(ctx(), REAL(L), n, n > 0 ? n : 1);
    UNPROTECT(1);
    check(rc);
    return L;
}

/* create_p_dotXnS(Xn_list, mn, Kn, theta): R/ode_gp_library.R:43-93.  The sampler lives behind an
 * external pointer whose finalizer releases the device memory; step/commit are the two halves of
 * one closure call (the draw in between is R's own rnorm, so R's RNG stream is the reference's). */
static void seq_finalizer(SEXP ptr)
{
    gpmi_seq *q = (gpmi_seq *)R_ExternalPtrAddr(ptr);
    if (q) gpmi_seq_destroy(q);
    R_ClearExternalPtr(ptr);
}

SEXP gpmi_R_seq_create(SEXP X, SEXP mn, SEXP Kn, SEXP alpha, SEXP ell, SEXP jitter, SEXP max_steps)
{
    int n = Rf_nrows(X), D = Rf_ncols(X);
    need(is_real(X) && is_real(mn) && is_real(Kn) && is_real(ell), "X, mn, Kn and the length-scales must be double");
    need(Rf_length(mn) == n && Rf_nrows(Kn) == n && Rf_ncols(Kn) == n, "mn must have nrow(X) entries and Kn be nrow(X) x nrow(X)");
    need(Rf_length(ell) == 1 || Rf_length(ell) == D, "length-scale must have length 1 or ncol(X)");
    gpmi_seq *q = NULL;
    int rc = gpmi_seq_create(ctx(), &q, REAL(X), n, n, D, REAL(mn), REAL(Kn), n, Rf_asReal(alpha), REAL(ell),
                             Rf_length(ell), Rf_asReal(jitter), Rf_asInteger(max_steps));
    check(rc); /* nothing to release on failure: gpmi_seq_create frees what it allocated */
    SEXP ptr = PROTECT(R_MakeExternalPtr(q, R_NilValue, R_NilValue));
    R_RegisterCFinalizerEx(ptr, seq_finalizer, TRUE);
    UNPROTECT(1);
    return ptr;
}

SEXP gpmi_R_seq_step(SEXP ptr, SEXP xs, SEXP D)
{
    gpmi_seq *q = (gpmi_seq *)R_ExternalPtrAddr(ptr);
    need(q != NULL, "the sampler has been released");
    need(is_real(xs) && Rf_length(xs) == Rf_asInteger(D), "xs must be a double vector with one entry per input dimension");
    SEXP out = PROTECT(Rf_allocVector(REALSXP, 2)); /* condMean, condVar */
    int rc = gpmi_seq_step(q, REAL(xs), REAL(out));
    UNPROTECT(1);
    check(rc);
    return out;
}

/* list(mean, var): for every row of Xs the first step of a fresh sampler -- the sweep of R/tests.R:89-97 in one call; the
 * sampler is left as it was */
SEXP gpmi_R_seq_marginals(SEXP ptr, SEXP Xs, SEXP D)
{
    gpmi_seq *q = (gpmi_seq *)R_ExternalPtrAddr(ptr);
    need(q != NULL, "the sampler has been released");
    int m = Rf_nrows(Xs);
    need(is_real(Xs) && Rf_ncols(Xs) == Rf_asInteger(D), "Xs must be a double matrix with one column per input dimension");
    SEXP mean = PROTECT(Rf_allocVector(REALSXP, m)), var = PROTECT(Rf_allocVector(REALSXP, m));
    int rc = gpmi_seq_marginals(q, REAL(Xs), m, m, REAL(mean), REAL(var));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, mean); SET_VECTOR_ELT(out, 1, var);
    UNPROTECT(3);
    check(rc);
    return out;
}

SEXP gpmi_R_seq_commit(SEXP ptr, SEXP dot_xs)
{
    need(R_ExternalPtrAddr(ptr) != NULL, "the sampler has been released");
    check(gpmi_seq_commit((gpmi_seq *)R_ExternalPtrAddr(ptr), Rf_asReal(dot_xs)));
    return R_NilValue;
}
