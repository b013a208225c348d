"""CPU references for gpmi_centered_gp_lp_grad: the centred latent GP of models/heteroscedastic_centered.stan:24-34, where the
k latent columns F are parameters and the GP is their prior.  Built on tests/vjp_reference.py (covariance, its derivatives,
long-double factorisation) and tests/latent_lik_reference.py (the heads).  Helper of tests/test_centered_gp_reference.py and
tests/test_gpu_centered_gp.py (not collected: no test_ prefix).

With Sigma = alpha^2 K0(X; ell) + jitter I = L L^T, Z = L^-1 F, A = Sigma^-1 F:
  sum_log = sum_i log L_ii, quad = sum_c z_c'z_c, prior = -quad / 2 - k sum_log (the `~` constant dropped),
  lp = prior + lik(F, Y), Fgrad = Fbar_head - A, grad_theta = 1/2 sum_ij (A A^T - k Sigma^-1)_ij dSigma_ij / dtheta.
"""
import functools

import numpy as np

import latent_lik_reference as lr
import vjp_reference as vr

EPS = float(np.finfo(float).eps)
FAMILIES = ("none",) + lr.FAMILIES
PARITY_JITTER = 1e-6
PARITY_ALPHA = 1.3
PARITY_SIZES = (10, 21, 100, 256, 300, 700)   # <= 256: one workgroup (small_cen = 256; by default up to the measured crossover); above: the chain
NONE_K = (1, 2, 3, 8)
COND_MAX = 2e7            # a condition on the parity inputs (tests/test_centered_gp_reference.py), not a measurement
HEAD_TOL = 1e-11          # of the sum of absolute terms, as tests/test_gpu_latent_lik.py


def k_of(family, k=None):
    return k if family == "none" else lr.K_OF[family]


def _bwd_solve_ld(L, B):
    """L^-T B by plain loops (any dtype)."""
    Y = np.zeros_like(B)
    for i in range(L.shape[0] - 1, -1, -1):
        Y[i] = (B[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def centered_reference(X, alpha, ell, F, family, Y=None, sigma=None, jitter=1e-9, dtype=float):
    """The whole call in `dtype`: float (LAPACK factorisation and solves) or np.longdouble (plain loops).  Returns a dict:
    lp, prior, lik, dlik_dsigma, sum_log_diag, quad, Fbar (the head's adjoint), A, Fgrad, grad, gabs (per theta:
    1/2 sum_ij (|sum_c a_ic a_jc| + k |Sigma^-1_ij|) |dSigma_ij / dtheta|, the scale of the contraction's rounding error)."""
    X = np.asarray(X, float).reshape(len(X), -1)
    n = X.shape[0]
    F = np.asarray(F, float).reshape(n, -1).astype(dtype)
    k = F.shape[1]
    n_ell = np.atleast_1d(ell).size
    K, _, _ = vr.se_cov(X, alpha, ell, jitter, dtype=dtype)
    if dtype is float:
        L = np.linalg.cholesky(K)
        Linv = np.linalg.solve(L, np.eye(n))
        Z = np.linalg.solve(L, F)
        A = np.linalg.solve(L.T, Z)
    else:
        L = vr._chol_ld(K)
        Linv = vr._fwd_solve_ld(L, np.eye(n, dtype=dtype))
        Z = vr._fwd_solve_ld(L, F)
        A = _bwd_solve_ld(L, Z)
    Sinv = Linv.T @ Linv
    sum_log = np.log(np.diag(L)).sum()
    quad = (Z * Z).sum()
    prior = -quad / 2 - k * sum_log
    if family == "none":
        lik, ds, Fb = dtype(0.0), dtype(0.0), np.zeros_like(F)
    else:
        lik, ds, Fb, _ = lr.head(family, F, Y, sigma, dtype=dtype)
    AA = A @ A.T
    G = (AA - k * Sinv) / 2
    Gabs = (np.abs(AA) + k * np.abs(Sinv)) / 2
    dKs = vr.dK_dtheta(X, alpha, ell, n_ell, dtype=dtype)
    grad = np.array([np.sum(G * dk) for dk in dKs], dtype=dtype)
    gabs = np.array([float(np.sum(Gabs * np.abs(dk))) for dk in dKs])
    return {"lp": prior + lik, "prior": prior, "lik": lik, "dlik_dsigma": ds, "sum_log_diag": sum_log, "quad": quad, "Fbar": Fb,
            "A": A, "Fgrad": Fb - A, "grad": grad, "gabs": gabs}


def cond2(X, alpha, ell, jitter):
    """cond_2(Sigma) in float64 (symmetric: the ratio of the extreme eigenvalues)."""
    K, _, _ = vr.se_cov(X, alpha, ell, jitter)
    w = np.linalg.eigvalsh(K)
    return float(w[-1] / w[0])


def prior_lp(X, alpha, ell, F, family, Y, sigma, jitter):
    """out[0] in float64 as a function of everything that is differentiated (for central differences)."""
    return float(centered_reference(X, alpha, ell, F, family, Y, sigma, jitter)["lp"])


# ---- lp__ of models/heteroscedastic_centered.stan (`~` constants dropped, <lower=0> log-Jacobians included) -------------------
def heteroscedastic_centered_lp(x, Y, l, sigmaf, mu, sigma_log, jitter=1e-9, dtype=float):
    mu = np.asarray(mu, float); s = np.asarray(sigma_log, float)
    r = centered_reference(np.asarray(x, float), sigmaf, [l], np.column_stack([mu, s]), "normal_logsd", Y, None, jitter, dtype)
    l_, sf = dtype(l), dtype(sigmaf)
    return (r["lp"] + 3 * np.log(l_) - 4 * l_ - sf * sf / 2 + np.log(l_) + np.log(sf) + np.log(s.astype(dtype)).sum())


def heteroscedastic_centered_lp_grad(x, Y, l, sigmaf, mu, sigma_log, jitter=1e-9, dtype=float):
    """(lp__, gradient in (l, sigmaf, mu, sigma_log))."""
    mu = np.asarray(mu, float); s = np.asarray(sigma_log, float); n = mu.size
    r = centered_reference(np.asarray(x, float), sigmaf, [l], np.column_stack([mu, s]), "normal_logsd", Y, None, jitter, dtype)
    l_, sf = dtype(l), dtype(sigmaf)
    lp = r["lp"] + 3 * np.log(l_) - 4 * l_ - sf * sf / 2 + np.log(l_) + np.log(sf) + np.log(s.astype(dtype)).sum()
    g = np.empty(2 + 2 * n, dtype=dtype)
    g[0] = r["grad"][1] + 4 / l_ - 4
    g[1] = r["grad"][0] - sf + 1 / sf
    g[2:2 + n] = r["Fgrad"][:, 0]
    g[2 + n:] = r["Fgrad"][:, 1] + 1 / s.astype(dtype)
    return lp, g


def model_case(n):
    """(x, Y, l, sigmaf, mu, sigma_log) at the reference's own size (heteroscedastic.R:7-10,38: N = 10, M = 5, l = 0.5, sigmaf = 1)
    and at N = 100 (the layout of test_gpu_latent_lik.py's model tests: linspace(0, 10), l = 0.15); the model's jitter is 1e-9."""
    rng = np.random.default_rng(40 + n)
    x = np.linspace(0.0, 3.0, n) if n <= 10 else np.linspace(0.0, 10.0, n)
    l, sf = (0.5, 1.0) if n <= 10 else (0.15, 1.1)
    Y = np.sin(x)[:, None] + 0.3 * rng.standard_normal((n, 5))
    K, _, _ = vr.se_cov(x.reshape(-1, 1), sf, [l], 1e-9)
    mu = np.linalg.cholesky(K) @ rng.standard_normal(n)
    return x, Y, l, sf, mu, 0.2 + rng.random(n)


def model_errors(got_lp, got_g, x, Y, l, sf, mu, s):
    """(relative error of lp, max-norm error of the gradient relative to max|gradient|, cond_2(Sigma)) against long double."""
    lp, g = heteroscedastic_centered_lp_grad(x, Y, l, sf, mu, s, dtype=np.longdouble)
    return (abs(float(np.longdouble(got_lp) - lp)) / abs(float(lp)), rel(got_g, g), cond2(np.asarray(x, float).reshape(-1, 1), sf, [l], 1e-9))


# ---- the configurations of the parity tests ----------------------------------------------------------------------------------
def parity_case(family, n, D, ard, m, k=None, seed=0):
    """(X, alpha, ell, F, Y, sigma) of one parity configuration, deterministic in its arguments: the layout of
    latent_lik_reference.path_case -- about one point per length-scale, X = U(0, 1)^D mean(ell) n^(1/D), so that cond(Sigma) stays
    below COND_MAX at jitter 1e-6 -- and F = chol(Sigma) N(0, 1), a draw from the prior: the quadratic form is O(n k), not
    O(|F|^2 / jitter)."""
    k = k_of(family, k)
    rng = np.random.default_rng(100000 * seed + 1000 * n + 100 * D + 10 * m + (1 if ard else 0) + 7 * FAMILIES.index(family) + 3 * k)
    ell = 0.6 + 0.4 * rng.random(D) if ard else np.array([0.8])
    X = rng.random((n, D)) * (float(np.mean(ell)) * n ** (1.0 / D))
    K, _, _ = vr.se_cov(X, PARITY_ALPHA, ell, PARITY_JITTER)
    F = np.linalg.cholesky(K) @ rng.standard_normal((n, k))
    if family == "normal_logsd":
        F[:, 1] *= 0.5
    if family == "bernoulli_logit":
        Y = (rng.uniform(size=(n, m)) < 0.4).astype(float)
    elif family == "none":
        Y = None
    else:
        Y = rng.standard_normal((n, m))
    return X, PARITY_ALPHA, ell, F, Y, (0.7 if family == "normal" else None)


def parity_cases():
    """Every (family, n, D, ard, m, k) the parity tests run: per family and size two of the six layouts below, rotated (as
    latent_lik_reference.parity_cases) so that every family meets D = 1, 2 and 3, isotropic and ARD, m = 1 and 5 on both paths;
    "none" rotates k through 1, 2, 3, 8 as well (48 cases)."""
    layouts = ((1, False, 1), (2, False, 5), (3, True, 1), (2, True, 5), (1, False, 5), (3, False, 1))
    out = []
    for fi, family in enumerate(FAMILIES):
        for ni, n in enumerate(PARITY_SIZES):
            for si, step in enumerate((0, 3)):
                D, ard, m = layouts[(fi + ni + step) % 6]
                k = NONE_K[(ni + 2 * si + (ni // 2)) % 4] if family == "none" else lr.K_OF[family]
                out.append((family, n, D, ard, m, k))
    return out


@functools.lru_cache(maxsize=None)
def parity_reference(case, longdouble=True):
    """(inputs, reference dict, cond_2(Sigma)) of one entry of parity_cases(), computed once per process."""
    family, n, D, ard, m, k = case
    inp = parity_case(family, n, D, ard, m, k)
    X, a, ell, F, Y, sg = inp
    ref = centered_reference(X, a, ell, F, family, Y, sg, PARITY_JITTER, dtype=np.longdouble if longdouble else float)
    return inp, ref, cond2(X, a, ell, PARITY_JITTER)


def rel(a, b):
    a = np.asarray(a, np.longdouble); b = np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def reference_errors(got, ref):
    """Errors of `got` (a dict with the keys of centered_reference or of Context.centered_gp_lp_grad) against `ref`: relative for
    sum_log_diag, quad and prior; max norm relative to max|Fgrad| for Fgrad; |grad - ref| per theta (absolute)."""
    e = {key: abs(float(np.longdouble(got[key]) - ref[key])) / abs(float(ref[key])) for key in ("sum_log_diag", "quad", "prior")}
    e["Fgrad"] = rel(np.asarray(got["Fgrad"]).reshape(ref["Fgrad"].shape), ref["Fgrad"])
    e["grad_abs"] = np.abs(np.asarray(got["grad"], np.longdouble) - ref["grad"]).astype(float)
    e["grad"] = float(np.max(e["grad_abs"]) / float(np.max(np.abs(ref["grad"]))))
    return e
