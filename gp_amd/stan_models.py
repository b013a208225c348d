"""Double-precision evaluations of the reference's Stan model blocks on the GPU.

models/fit_hyperparameters.stan:18-32 (== stan/fit_hyperparameters.stan):
    Sigma = cov_exp_quad(t, alpha, rho) + sigma^2 I;  L = cholesky_decompose(Sigma)
    y ~ multi_normal_cholesky(0, L)
models/exact_gp.stan:16-26:  f = cholesky_decompose(cov_exp_quad(x, 1, l) + 1e-10 I) * z
models/westbrook_exact.stan, models/heteroscedastic.stan, models/fit_full_gp.stan: the same latent transform under a Bernoulli,
    a log-sd normal and a normal likelihood (gpmi_latent_gp_lp_grad: one factorisation per value/gradient pair)
models/heteroscedastic_centered.stan: the CENTRED parameterisation -- mu and sigma_log are parameters themselves with the GP as
    their prior (gpmi_centered_gp_lp_grad: one factorisation for both columns)
"""
import math

import numpy as np

from ._lib import NotPositiveDefinite, default_context


def gp_log_marginal(X, y, alpha, rho, sigma, jitter=0.0, ctx=None):
    """log p(y | X, alpha, rho, sigma) = -1/2 z'z - sum log L_ii - N/2 log(2 pi)."""
    return (ctx or default_context()).logml(X, y, alpha, rho, sigma, jitter)[0]


def stan_lp(sum_log_diag, quad, alpha, rho, sigma):
    """lp__ of fit_hyperparameters.stan: likelihood without the
    -N/2 log 2pi constant (`~` drops it, :31), gamma(4,4) / half-normal(0,1) priors without
    constants (:27-29), plus the log-Jacobian of the <lower=0> transforms (:13-15)."""
    return (-sum_log_diag - 0.5 * quad + (3.0 * math.log(rho) - 4.0 * rho) - 0.5 * alpha * alpha
            - 0.5 * sigma * sigma + (math.log(rho) + math.log(alpha) + math.log(sigma)))


def fit_hyperparameters_log_prob(t, y, rho, alpha, sigma, ctx=None):
    """Stan's lp__ for one (rho, alpha, sigma); -inf when Sigma is not positive definite
    (Stan rejects the proposal on cholesky_decompose's domain_error)."""
    try:
        _, sld, q = (ctx or default_context()).logml(t, y, alpha, rho, sigma, 0.0)
    except NotPositiveDefinite:
        return -math.inf
    return stan_lp(sld, q, alpha, rho, sigma)


def fit_hyperparameters_log_prob_grad(t, y, rho, alpha, sigma, ctx=None):
    """(lp__, d lp__/d(rho, alpha, sigma)) on the constrained scale -- the value/gradient pair Stan's
    autodiff produces per leapfrog step for fit_hyperparameters.stan; feeds an optimiser or HMC outside
    Stan.  Prior and Jacobian terms of stan_lp() differentiate to 4/rho - 4, 1/alpha - alpha,
    1/sigma - sigma."""
    try:
        out, g = (ctx or default_context()).logml_grad(t, y, alpha, [rho], sigma, 0.0)
    except NotPositiveDefinite:
        return -math.inf, np.full(3, math.nan)
    lp = stan_lp(out[1], out[2], alpha, rho, sigma)
    return lp, np.array([g[1] + 4.0 / rho - 4.0, g[0] + 1.0 / alpha - alpha, g[2] + 1.0 / sigma - sigma])


def fit_hyperparameters_log_prob_grad_chains(t, y, rho, alpha, sigma, ctx=None):
    """The same for several chains at once -- rstan runs `chains = 4` (pendulum_fit.R:140), each asking for one
    value + gradient per leapfrog step: (lp (C,), grad (C, 3) in (rho, alpha, sigma) order), evaluated
    concurrently on the GPU's lanes; rejected (non-PD) proposals get -inf / NaN."""
    rho = np.atleast_1d(np.asarray(rho, float)); alpha = np.atleast_1d(np.asarray(alpha, float))
    sigma = np.atleast_1d(np.asarray(sigma, float))
    out, g, info = (ctx or default_context()).logml_grad_grid(t, y, alpha, rho, sigma, 0.0)
    lp = np.array([stan_lp(o[1], o[2], a, r, s) if i == 0 else -math.inf for o, a, r, s, i in zip(out, alpha, rho, sigma, info)])
    grad = np.column_stack([g[:, 1] + 4.0 / rho - 4.0, g[:, 0] + 1.0 / alpha - alpha, g[:, 2] + 1.0 / sigma - sigma])
    grad[info != 0] = math.nan
    return lp, grad


def gp_log_marginal_grid(X, y, alpha, rho_vec, sigma_vec, jitter=0.0, lp=False, ctx=None):
    """|rho| x |sigma| matrix of log marginal likelihoods (lp=True: Stan lp__ instead);
    non-PD points are NaN (-inf for lp) and the grid continues."""
    rho_vec = np.atleast_1d(np.asarray(rho_vec, float)); sigma_vec = np.atleast_1d(np.asarray(sigma_vec, float))
    R, S = np.meshgrid(rho_vec, sigma_vec, indexing="ij")
    out, info = (ctx or default_context()).logml_grid(X, y, np.full(R.size, float(alpha)), R.ravel(), S.ravel(), jitter)
    if lp:
        vals = np.array([stan_lp(o[1], o[2], float(alpha), r, s) if i == 0 else -math.inf
                         for o, r, s, i in zip(out, R.ravel(), S.ravel(), info)])
    else:
        vals = out[:, 0]
    return vals.reshape(R.shape)


def get_ml_from_grid(values, alpha, rho_vec, sigma_vec):
    """arg-max over the grid -> list(alpha=, rho=, sigma=): mirror of
    get_ml_from_stan_samples (R/tests.R:21-27) with grid points in place of posterior draws."""
    v = np.where(np.isfinite(values), values, -np.inf)
    i, j = np.unravel_index(int(np.argmax(v)), v.shape)
    return {"alpha": float(alpha), "rho": float(np.atleast_1d(rho_vec)[i]), "sigma": float(np.atleast_1d(sigma_vec)[j])}


def exact_gp_f(x, l, z, ctx=None):
    """f = L z with L = chol(cov_exp_quad(x, 1, l) + 1e-10 I) -- models/exact_gp.stan:17-25."""
    c = ctx or default_context()
    x = np.asarray(x, float).reshape(len(z), -1)
    return c.exact_gp_f(x, 1.0, [l], z, 1e-10)   # covariance, factor and product stay on the device (gpmi_exact_gp_f)


def exact_gp_log_prob_grad(x, y, l, sigma, z, ctx=None, fused=False):
    """(lp__, d lp__/d(l, sigma, z)) of models/exact_gp.stan -- the value/gradient pair NUTS asks for at every leapfrog step
    of test_interpolate.R:31-36.  Conventions of fit_hyperparameters_log_prob_grad: `~` drops constants, the <lower=0>
    Jacobians log l + log sigma are included:
        lp = -z'z / 2 + 3 log l - 4 l - N log sigma - |y - f|^2 / (2 sigma^2) + log l + log sigma.
    With ubar = (y - f) / sigma^2 the gradient is (ubar' (dL/dl) z + 4/l - 4, -N/sigma + |y - f|^2 / sigma^3 + 1/sigma,
    L' ubar - z); ubar' (dL/dl) z and L' ubar come from the vector-Jacobian product of the transform
    (gpmi_exact_gp_f_vjp).  A non-positive-definite proposal returns (-inf, NaN).  fused=True takes
    gpmi_latent_gp_lp_grad instead: product, likelihood, its adjoint and the sweep in one call with one factorisation."""
    c = ctx or default_context()
    z = np.asarray(z, float).ravel()
    y = np.asarray(y, float).ravel()
    n = z.size
    x = np.asarray(x, float).reshape(n, -1)
    if fused:
        try:
            r = c.latent_gp_lp_grad(x, 1.0, [l], z, "normal", y, sigma, 1e-10, want_f=False)
        except NotPositiveDefinite:
            return -math.inf, np.full(2 + n, math.nan)
        lp = -0.5 * float(z @ z) + 3.0 * math.log(l) - 4.0 * l + r["lik"] + math.log(l) + math.log(sigma)
        grad = np.empty(2 + n)
        grad[0] = r["grad"][1] + 4.0 / l - 4.0
        grad[1] = r["dlik_dsigma"] + 1.0 / sigma
        grad[2:] = r["Zbar"] - z
        return lp, grad
    try:
        f = c.exact_gp_f(x, 1.0, [l], z, 1e-10)
        r = y - f
        ubar = r / (sigma * sigma)
        _, zbar, g = c.exact_gp_f_vjp(x, 1.0, [l], z, ubar, 1e-10)
    except NotPositiveDefinite:
        return -math.inf, np.full(2 + n, math.nan)
    rr = float(r @ r)
    lp = (-0.5 * float(z @ z) + 3.0 * math.log(l) - 4.0 * l - n * math.log(sigma) - 0.5 * rr / (sigma * sigma)
          + math.log(l) + math.log(sigma))
    grad = np.empty(2 + n)
    grad[0] = g[1] + 4.0 / l - 4.0
    grad[1] = -n / sigma + rr / sigma ** 3 + 1.0 / sigma
    grad[2:] = zbar - z
    return lp, grad


def westbrook_exact_log_prob_grad(x, y, z, sigma, l, ctx=None, jitter=1e-12):
    """(lp__, d lp__/d(z, sigma, l)) of models/westbrook_exact.stan (sigma is the GP's amplitude; y in {0, 1}):
        lp = -z'z / 2 + 3 log l - 4 l - sigma^2 / 2 + sum(y f - softplus(f)) + log sigma + log l,  f = chol(K(sigma, l) + 1e-12 I) z.
    The model writes y ~ bernoulli(inv_logit(f)); the likelihood here is the equal, stable bernoulli_logit form.  One call of
    gpmi_latent_gp_lp_grad; conventions of exact_gp_log_prob_grad.  jitter: the model's 1e-12 unless overridden."""
    c = ctx or default_context()
    z = np.asarray(z, float).ravel()
    n = z.size
    x = np.asarray(x, float).reshape(n, -1)
    try:
        r = c.latent_gp_lp_grad(x, sigma, [l], z, "bernoulli_logit", np.asarray(y, float).ravel(), None, jitter, want_f=False)
    except NotPositiveDefinite:
        return -math.inf, np.full(2 + n, math.nan)
    lp = -0.5 * float(z @ z) + 3.0 * math.log(l) - 4.0 * l - 0.5 * sigma * sigma + r["lik"] + math.log(sigma) + math.log(l)
    grad = np.empty(2 + n)
    grad[:n] = r["Zbar"] - z
    grad[n] = r["grad"][0] - sigma + 1.0 / sigma
    grad[n + 1] = r["grad"][1] + 4.0 / l - 4.0
    return lp, grad


def heteroscedastic_log_prob_grad(x, Y, l, sigmaf, z1, z2, ctx=None):
    """(lp__, d lp__/d(l, sigmaf, z1, z2)) of models/heteroscedastic.stan (Y: N x M replicates; mu = L z1, sigma = exp(L z2),
    L = chol(K(sigmaf, l) + 1e-9 I)):
        lp = 3 log l - 4 l - sigmaf^2 / 2 - z1'z1 / 2 - z2'z2 / 2 + sum_im(-s_i - (y_im - mu_i)^2 exp(-2 s_i) / 2) + log l + log sigmaf.
    One call of gpmi_latent_gp_lp_grad with two latent columns; conventions of exact_gp_log_prob_grad."""
    c = ctx or default_context()
    z1 = np.asarray(z1, float).ravel(); z2 = np.asarray(z2, float).ravel()
    n = z1.size
    x = np.asarray(x, float).reshape(n, -1)
    Y = np.asarray(Y, float).reshape(n, -1)
    try:
        r = c.latent_gp_lp_grad(x, sigmaf, [l], np.column_stack([z1, z2]), "normal_logsd", Y, None, 1e-9, want_f=False)
    except NotPositiveDefinite:
        return -math.inf, np.full(2 + 2 * n, math.nan)
    lp = (3.0 * math.log(l) - 4.0 * l - 0.5 * sigmaf * sigmaf - 0.5 * float(z1 @ z1) - 0.5 * float(z2 @ z2) + r["lik"]
          + math.log(l) + math.log(sigmaf))
    grad = np.empty(2 + 2 * n)
    grad[0] = r["grad"][1] + 4.0 / l - 4.0
    grad[1] = r["grad"][0] - sigmaf + 1.0 / sigmaf
    grad[2:2 + n] = r["Zbar"][:, 0] - z1
    grad[2 + n:] = r["Zbar"][:, 1] - z2
    return lp, grad


def heteroscedastic_centered_log_prob_grad(x, Y, l, sigmaf, mu, sigma_log, ctx=None, jitter=1e-9):
    """(lp__, d lp__/d(l, sigmaf, mu, sigma_log)) of models/heteroscedastic_centered.stan (Y: N x M replicates; mu and sigma_log
    ~ multi_normal_cholesky(0, L), L = chol(K(sigmaf, l) + 1e-9 I), y[:, m] ~ normal(mu, exp(sigma_log)), :24-41):
        lp = sum_c(-f_c' Sigma^-1 f_c / 2 - sum log L_ii) + sum_im(-s_i - (y_im - mu_i)^2 exp(-2 s_i) / 2) + 3 log l - 4 l
             - sigmaf^2 / 2 + log l + log sigmaf + sum_i log sigma_log_i,   f = (mu, sigma_log), s = sigma_log;
    the last term is the Jacobian of vector<lower=0>[N] sigma_log (:16), so d/dsigma_log_i gains 1 / sigma_log_i.  One call of
    gpmi_centered_gp_lp_grad with two latent columns; conventions of exact_gp_log_prob_grad (`~` constants dropped, gradient in
    the constrained values).  A non-positive-definite proposal returns (-inf, NaN).  jitter: the model's 1e-9 unless overridden."""
    c = ctx or default_context()
    mu = np.asarray(mu, float).ravel(); sigma_log = np.asarray(sigma_log, float).ravel()
    n = mu.size
    x = np.asarray(x, float).reshape(n, -1)
    Y = np.asarray(Y, float).reshape(n, -1)
    try:
        r = c.centered_gp_lp_grad(x, sigmaf, [l], np.column_stack([mu, sigma_log]), "normal_logsd", Y, None, jitter)
    except NotPositiveDefinite:
        return -math.inf, np.full(2 + 2 * n, math.nan)
    lp = (r["lp"] + 3.0 * math.log(l) - 4.0 * l - 0.5 * sigmaf * sigmaf + math.log(l) + math.log(sigmaf)
          + float(np.sum(np.log(sigma_log))))
    grad = np.empty(2 + 2 * n)
    grad[0] = r["grad"][1] + 4.0 / l - 4.0
    grad[1] = r["grad"][0] - sigmaf + 1.0 / sigmaf
    grad[2:2 + n] = r["Fgrad"][:, 0]
    grad[2 + n:] = r["Fgrad"][:, 1] + 1.0 / sigma_log
    return lp, grad


def fit_full_gp_log_prob_grad(x, y, l, alpha, sigma, zn, ctx=None):
    """(lp__, d lp__/d(l, alpha, sigma, zn)) of models/fit_full_gp.stan (z = alpha chol(K(1, l) + 1e-12 I) zn, y ~ normal(z, sigma),
    no prior on sigma):
        lp = 3 log l - 4 l - alpha^2 / 2 - zn'zn / 2 - N log sigma - |y - z|^2 / (2 sigma^2) + log l + log alpha + log sigma.
    The call with amplitude 1 and Z = alpha zn: zn_bar = alpha Zbar - zn, alpha_bar = Zbar . zn - alpha + 1 / alpha."""
    c = ctx or default_context()
    zn = np.asarray(zn, float).ravel()
    n = zn.size
    x = np.asarray(x, float).reshape(n, -1)
    try:
        r = c.latent_gp_lp_grad(x, 1.0, [l], alpha * zn, "normal", np.asarray(y, float).ravel(), sigma, 1e-12, want_f=False)
    except NotPositiveDefinite:
        return -math.inf, np.full(3 + n, math.nan)
    lp = (3.0 * math.log(l) - 4.0 * l - 0.5 * alpha * alpha - 0.5 * float(zn @ zn) + r["lik"] + math.log(l) + math.log(alpha)
          + math.log(sigma))
    grad = np.empty(3 + n)
    grad[0] = r["grad"][1] + 4.0 / l - 4.0
    grad[1] = float(r["Zbar"] @ zn) - alpha + 1.0 / alpha
    grad[2] = r["dlik_dsigma"] + 1.0 / sigma
    grad[3:] = alpha * r["Zbar"] - zn
    return lp, grad


def _interpolated_log_prob_grad(value, vjp, lo, hi, y, l, sigma, z):
    """lp__ and its gradient in (l, sigma, z) for a latent f = L(l) z with l <lower=lo, upper=hi>: the conventions of
    exact_gp_log_prob_grad with the Jacobian of the bounded transform, log(l - lo) + log(hi - l) - log(hi - lo)."""
    z = np.asarray(z, float).ravel()
    y = np.asarray(y, float).ravel()
    n = z.size
    if not (lo < l < hi) or not sigma > 0:
        return -math.inf, np.full(2 + n, math.nan)
    f = value(l, z)
    r = y - f
    ubar = r / (sigma * sigma)
    _, zbar, lbar = vjp(l, z, ubar, False)
    rr = float(r @ r)
    lp = (-0.5 * float(z @ z) + 3.0 * math.log(l) - 4.0 * l - n * math.log(sigma) - 0.5 * rr / (sigma * sigma)
          + math.log(l - lo) + math.log(hi - l) - math.log(hi - lo) + math.log(sigma))
    grad = np.empty(2 + n)
    grad[0] = lbar + 3.0 / l - 4.0 + 1.0 / (l - lo) - 1.0 / (hi - l)
    grad[1] = -n / sigma + rr / sigma ** 3 + 1.0 / sigma
    grad[2:] = zbar - z
    return lp, grad


def cubic_interpolated_gp_log_prob_grad(interp, y, l, sigma, z):
    """(lp__, d lp__/d(l, sigma, z)) of models/cubic_interpolated_gp.stan (f = approx_Lz(l, lp, Ls, dLdls, z), l in
    [min(lp), max(lp)], :17) for a FactorInterpolator `interp`:
        lp = -z'z/2 + 3 log l - 4 l - N log sigma - |y - f|^2 / (2 sigma^2) + log(l - lo) + log(hi - l) - log(hi - lo) + log sigma.
    With ubar = (y - f) / sigma^2 the gradient is (lbar(ubar) + 3/l - 4 + 1/(l - lo) - 1/(hi - l),
    -N/sigma + |y - f|^2/sigma^3 + 1/sigma, Zbar(ubar) - z), lbar and Zbar from gpmi_approx_Lz_vjp.  l outside the open
    interval returns (-inf, NaN)."""
    lp_ = np.asarray(interp.lp, float)
    return _interpolated_log_prob_grad(interp.ctx.approx_Lz, interp.ctx.approx_Lz_vjp, float(lp_.min()), float(lp_.max()), y, l, sigma, z)


def interpolated_gp_log_prob_grad(interp, y, l, sigma, z):
    """The same for models/interpolated_gp.stan (f = L(l) z with L(l) = to_matrix(lookup * Kp(l)), l in
    [min(lp), max(lp)], :32) for a GPFactorInterpolator `interp`; lbar and Zbar from gpmi_interp_gp_Lz_vjp."""
    lp_ = np.asarray(interp.lp, float)
    return _interpolated_log_prob_grad(interp.ctx.interp_gp_Lz, interp.ctx.interp_gp_Lz_vjp, float(lp_.min()), float(lp_.max()), y, l, sigma, z)


def fit_approx_gp_log_prob_grad(x, y, l, alpha, sigma, zm, M=None, scale=1.0, ctx=None):
    """(lp__, d lp__/d(l, alpha, sigma, zm)) of models/fit_approx_gp.stan (zh = approx_L(M, scale, x, alpha, l) zm, the
    Hermite-eigenfunction low-rank GP; no prior on sigma):
        lp = 3 log l - 4 l - alpha^2 / 2 - zm'zm / 2 - N log sigma - |y - zh|^2 / (2 sigma^2) + log l + log alpha + log sigma.
    One call of gpmi_lowrank_latent_lp_grad; conventions of exact_gp_log_prob_grad (`~` drops constants, the <lower=0> Jacobians
    are included)."""
    c = ctx or default_context()
    zm = np.asarray(zm, float).ravel()
    M = zm.size if M is None else int(M)
    r = c.lowrank_latent_lp_grad(x, M, scale, alpha, l, zm, "normal", np.asarray(y, float).ravel(), sigma, want_q=False)
    lp = (3.0 * math.log(l) - 4.0 * l - 0.5 * alpha * alpha - 0.5 * float(zm @ zm) + r["lik"] + math.log(l) + math.log(alpha)
          + math.log(sigma))
    grad = np.empty(3 + M)
    grad[0] = r["grad"][1] + 4.0 / l - 4.0
    grad[1] = r["grad"][0] - alpha + 1.0 / alpha
    grad[2] = r["dlik_dsigma"] + 1.0 / sigma
    grad[3:] = r["zbar"] - zm
    return lp, grad


def westbrook_log_prob_grad(x, y, z, sigma, l, M=None, scale=0.25, ctx=None):
    """(lp__, d lp__/d(z, sigma, l)) of models/westbrook.stan (q = approx_L(M, scale, x, sigma, l) z; sigma is the basis'
    amplitude; y in {0, 1}):
        lp = 3 log l - 4 l - z_1^2 / (2 0.01^2) - sum_{k > 1} z_k^2 / 2 - sigma^2 / 2 + sum(y q - softplus(q)) + log sigma + log l.
    One call of gpmi_lowrank_latent_lp_grad; conventions of westbrook_exact_log_prob_grad."""
    c = ctx or default_context()
    z = np.asarray(z, float).ravel()
    M = z.size if M is None else int(M)
    r = c.lowrank_latent_lp_grad(x, M, scale, sigma, l, z, "bernoulli_logit", np.asarray(y, float).ravel(), None, want_q=False)
    w = np.ones(M)
    w[0] = 1.0 / (0.01 * 0.01)
    lp = 3.0 * math.log(l) - 4.0 * l - 0.5 * float(z @ (w * z)) - 0.5 * sigma * sigma + r["lik"] + math.log(sigma) + math.log(l)
    grad = np.empty(M + 2)
    grad[:M] = r["zbar"] - w * z
    grad[M] = r["grad"][0] - sigma + 1.0 / sigma
    grad[M + 1] = r["grad"][1] + 4.0 / l - 4.0
    return lp, grad
