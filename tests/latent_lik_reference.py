"""CPU references for gpmi_latent_gp_lp_grad: the three likelihood heads (numpy float64 and np.longdouble) and the lp__ of the
three latent exact-GP models they serve, built on tests/vjp_reference.py.  Helper of tests/test_latent_lik_reference.py and
tests/test_gpu_latent_lik.py (not collected: no test_ prefix).

A head maps F (n x k) and Y (n x m) to (lik, d lik / d sigma, Fbar, sum of the absolute values of lik's terms); `~` drops
constants, so there is no -1/2 log 2 pi:
  normal          (k = 1): lik = sum(-log sigma - (y - f)^2 / (2 sigma^2))
  bernoulli_logit (k = 1): lik = sum(y f - softplus(f)), softplus(f) = max(f, 0) + log1p(exp(-|f|))
  normal_logsd    (k = 2): lik = sum(-s - (y - mu)^2 exp(-2 s) / 2), mu = F[:, 0], s = F[:, 1]
"""
import numpy as np

import vjp_reference as vr

FAMILIES = ("normal", "bernoulli_logit", "normal_logsd")
K_OF = {"normal": 1, "bernoulli_logit": 1, "normal_logsd": 2}


def head(family, F, Y, sigma=None, dtype=float):
    """(lik, dlik_dsigma, Fbar (n x k), abs_sum) in `dtype` (float or np.longdouble)."""
    F = np.asarray(F, dtype).reshape(len(F), -1)
    Y = np.asarray(Y, dtype).reshape(len(F), -1)
    n, m = Y.shape
    half = dtype(0.5)
    if family == "normal":
        s = dtype(sigma)
        R = Y - F[:, :1]
        t = -np.log(s) - half * R * R / (s * s)
        return t.sum(), -n * m / s + (R * R).sum() / s ** 3, (R.sum(axis=1) / (s * s)).reshape(n, 1), np.abs(t).sum()
    if family == "bernoulli_logit":
        f = F[:, :1]
        e = np.exp(-np.abs(f))
        sp = np.maximum(f, 0) + np.log1p(e)
        p = np.where(f >= 0, 1 / (1 + e), e / (1 + e))
        t = Y * f - sp
        return t.sum(), dtype(0.0), (Y - p).sum(axis=1).reshape(n, 1), (np.abs(Y * f) + np.abs(sp)).sum()
    if family == "normal_logsd":
        mu = F[:, :1]; s = F[:, 1:2]
        w = np.exp(-2 * s)
        R = Y - mu
        t = -s - half * R * R * w
        Fb = np.column_stack([(R * w).sum(axis=1), (R * R * w - 1).sum(axis=1)])
        return t.sum(), dtype(0.0), Fb, (np.abs(s) + half * R * R * w).sum()
    raise ValueError(family)


def head_abs(family, F, Y, sigma=None):
    """Sums of the absolute values of the terms of Fbar (n x k, per row) and of d lik / d sigma: the scale of their rounding error."""
    F = np.asarray(F, float).reshape(len(F), -1)
    Y = np.asarray(Y, float).reshape(len(F), -1)
    n, m = Y.shape
    if family == "normal":
        R = Y - F[:, :1]
        return (np.abs(R).sum(axis=1) / sigma ** 2).reshape(n, 1), n * m / sigma + (R * R).sum() / sigma ** 3
    if family == "bernoulli_logit":
        return (np.abs(Y).sum(axis=1) + m).reshape(n, 1), 0.0
    w = np.exp(-2 * F[:, 1:2]); R = Y - F[:, :1]
    return np.column_stack([(np.abs(R) * w).sum(axis=1), (R * R * w + 1).sum(axis=1)]), 0.0


def lik_of_F(family, F, Y, sigma=None):
    return float(head(family, F, Y, sigma)[0])


def latent(X, alpha, ell, Z, jitter):
    """F = chol(K + jitter I) Z in float64."""
    K, _, _ = vr.se_cov(X, alpha, ell, jitter)
    Z = np.asarray(Z, float).reshape(len(Z), -1)
    return np.linalg.cholesky(K) @ Z


def lp_grad_reference(family, X, alpha, ell, Z, Y, sigma, jitter):
    """The whole call in float64: dict of lik, dlik_dsigma, F, Fbar, Zbar, grad (vjp_reverse on the head's adjoint)."""
    F = latent(X, alpha, ell, Z, jitter)
    lik, ds, Fb, _ = head(family, F, Y, sigma)
    _, Zb, g = vr.vjp_reverse(X, alpha, ell, Z, Fb, jitter)
    return {"lik": float(lik), "dlik_dsigma": float(ds), "F": F, "Fbar": Fb, "Zbar": Zb, "grad": g}


# ---- lp__ of the models (the `~` constants dropped, <lower=0> log-Jacobians included) -------------------------------------------
def westbrook_exact_lp(x, y, z, sigma, l, jitter=1e-12):
    """models/westbrook_exact.stan; parameters (z, sigma, l), sigma the GP amplitude."""
    z = np.asarray(z, float)
    f = latent(np.asarray(x, float), sigma, [l], z, jitter)
    return (-0.5 * z @ z + 3.0 * np.log(l) - 4.0 * l - 0.5 * sigma * sigma + lik_of_F("bernoulli_logit", f, y)
            + np.log(sigma) + np.log(l))


def heteroscedastic_lp(x, Y, l, sigmaf, z1, z2):
    """models/heteroscedastic.stan; parameters (l, sigmaf, z1, z2), jitter 1e-9."""
    z1 = np.asarray(z1, float); z2 = np.asarray(z2, float)
    F = latent(np.asarray(x, float), sigmaf, [l], np.column_stack([z1, z2]), 1e-9)
    return (3.0 * np.log(l) - 4.0 * l - 0.5 * sigmaf * sigmaf - 0.5 * z1 @ z1 - 0.5 * z2 @ z2 + lik_of_F("normal_logsd", F, Y)
            + np.log(l) + np.log(sigmaf))


def fit_full_gp_lp(x, y, l, alpha, sigma, zn):
    """models/fit_full_gp.stan; parameters (l, alpha, sigma, zn), z = alpha chol(K(1, l) + 1e-12 I) zn, no prior on sigma."""
    zn = np.asarray(zn, float)
    f = alpha * latent(np.asarray(x, float), 1.0, [l], zn, 1e-12)
    return (3.0 * np.log(l) - 4.0 * l - 0.5 * alpha * alpha - 0.5 * zn @ zn + lik_of_F("normal", f, y, sigma)
            + np.log(l) + np.log(alpha) + np.log(sigma))


def westbrook_exact_lp_grad(x, y, z, sigma, l, jitter=1e-12):
    """(lp__, gradient in (z, sigma, l)) through vjp_reverse."""
    z = np.asarray(z, float); n = z.size
    r = lp_grad_reference("bernoulli_logit", np.asarray(x, float), sigma, [l], z, y, None, jitter)
    g = np.empty(n + 2)
    g[:n] = r["Zbar"][:, 0] - z
    g[n] = r["grad"][0] - sigma + 1.0 / sigma
    g[n + 1] = r["grad"][1] + 4.0 / l - 4.0
    return westbrook_exact_lp(x, y, z, sigma, l, jitter), g


def heteroscedastic_lp_grad(x, Y, l, sigmaf, z1, z2):
    z1 = np.asarray(z1, float); z2 = np.asarray(z2, float); n = z1.size
    r = lp_grad_reference("normal_logsd", np.asarray(x, float), sigmaf, [l], np.column_stack([z1, z2]), Y, None, 1e-9)
    g = np.empty(2 + 2 * n)
    g[0] = r["grad"][1] + 4.0 / l - 4.0
    g[1] = r["grad"][0] - sigmaf + 1.0 / sigmaf
    g[2:2 + n] = r["Zbar"][:, 0] - z1
    g[2 + n:] = r["Zbar"][:, 1] - z2
    return heteroscedastic_lp(x, Y, l, sigmaf, z1, z2), g


def fit_full_gp_lp_grad(x, y, l, alpha, sigma, zn):
    zn = np.asarray(zn, float); n = zn.size
    r = lp_grad_reference("normal", np.asarray(x, float), 1.0, [l], alpha * zn, y, sigma, 1e-12)
    zb = r["Zbar"][:, 0]
    g = np.empty(3 + n)
    g[0] = r["grad"][1] + 4.0 / l - 4.0
    g[1] = zb @ zn - alpha + 1.0 / alpha
    g[2] = r["dlik_dsigma"] + 1.0 / sigma
    g[3:] = alpha * zb - zn
    return fit_full_gp_lp(x, y, l, alpha, sigma, zn), g


# ---- the configurations of the GPU parity test (tests/test_gpu_latent_lik.py) and their tolerance ------------------------------
ZBAR_TOL = 1e-9    # relative, max norm: the bounds tests/test_gpu_exact_gp_vjp.py uses
GRAD_TOL = 1e-8
PARITY_JITTER = 1e-6
PARITY_SIZES = (21, 100, 256, 300, 700)   # <= 256: one workgroup; above: the chain


def parity_case(family, n, D, ard, m, seed=0):
    """(X, alpha, ell, Z, Y, sigma) of one parity configuration; deterministic in its arguments."""
    rng = np.random.default_rng(1000 * n + 100 * D + 10 * m + (1 if ard else 0) + 7 * FAMILIES.index(family) + seed)
    X = rng.uniform(0.0, 4.0, size=(n, D))
    ell = list(0.4 + 0.3 * np.arange(D)) if ard else [0.5]
    alpha = 1.3
    k = K_OF[family]
    Z = rng.standard_normal((n, k))
    if family == "bernoulli_logit":
        Y = (rng.uniform(size=(n, m)) < 0.4).astype(float)
    else:
        Y = rng.standard_normal((n, m))
    if family == "normal_logsd":
        Z[:, 1] *= 0.5
    return X, alpha, ell, Z, Y, (0.7 if family == "normal" else None)


def path_case(family, n, m=5):
    """The layout of tests/test_gpu_exact_gp_vjp.py::test_one_workgroup_and_chain_agree (D = 2, ARD, about one point per
    length-scale: cond(K) 5e6 at n = 100, 9e5 at n = 256 with jitter 1e-6) with a head's Y: the two paths factor K in different
    block orders, so their disagreement is rounding amplified by cond(K), and that test's bounds (1e-12, 1e-11) were set for this
    conditioning.  parity_case's denser points (cond 4.5e7 at n = 256) would test the bounds at 50 times the amplification."""
    rng = np.random.default_rng(n)
    ell = 0.6 + 0.4 * rng.random(2)
    X = rng.random((n, 2)) * (ell.mean() * n ** 0.5)
    k = K_OF[family]
    Z = rng.standard_normal((n, k))
    if family == "normal_logsd":
        Z[:, 1] *= 0.5
    Y = (rng.uniform(size=(n, m)) < 0.4).astype(float) if family == "bernoulli_logit" else rng.standard_normal((n, m))
    return X, 1.3, ell, Z, Y, (0.7 if family == "normal" else None)


def parity_cases():
    """Every (family, n, D, ard, m) the GPU parity test runs: per family and size two of the five layouts below, rotated so that
    every family meets D = 1 and 2, isotropic and ARD, m = 1 and 5 on both paths (30 cases)."""
    layouts = ((1, False, 1), (2, False, 5), (2, True, 1), (1, False, 5), (2, True, 5))
    out = []
    for fi, family in enumerate(FAMILIES):
        for ni, n in enumerate(PARITY_SIZES):
            for step in (0, 2):
                D, ard, m = layouts[(fi + ni + step) % 5]
                out.append((family, n, D, ard, m))
    return out


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
