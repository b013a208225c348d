"""numpy restatements of the two interpolated latent-GP models of test_interpolate.R, written from the model text:

- models/cubic_interpolated_gp.stan (+ .hpp): f = v(l) z, v the cubic Hermite blend of the tabulated factors around l
  (the blend and its l-partial come from the oracle: orc.approx_L / orc.approx_Lz_grad);
- models/interpolated_gp.stan: lookup = (Sigma_P \\ exact)^T (:10-27), L(l) = to_matrix(lookup * Kp(l), N, N) (:39-42),
  f = L z (:44), with Kp_p = exp(-(l - lp_p)^2 / (2 rho^2)).

Both share the lp__ of the conventions of exact_gp_log_prob_grad with l <lower=min(lp), upper=max(lp)>:
    lp = -z'z/2 + 3 log l - 4 l - N log sigma - |y - f|^2 / (2 sigma^2) + log(l - lo) + log(hi - l) - log(hi - lo) + log sigma
and, with ubar = (y - f) / sigma^2, the gradient
    (ubar' (dL/dl) z + 3/l - 4 + 1/(l - lo) - 1/(hi - l), -N/sigma + |y - f|^2/sigma^3 + 1/sigma, L' ubar - z)."""
import math

import numpy as np


def cov_exp_quad_1d(a, b, rho):
    a = np.asarray(a, float); b = np.asarray(b, float)
    d = a[:, None] - b[None, :]
    return np.exp(-(d * d) / (2.0 * rho * rho))


def sigma_p(lp, rho=1.0, jitter=1e-10):
    """Sigma_P = cov_exp_quad(lp, 1, rho) + jitter I (interpolated_gp.stan:10, :23-25)."""
    lp = np.asarray(lp, float)
    return cov_exp_quad_1d(lp, lp, rho) + jitter * np.eye(lp.size)


def gp_lookup(lp, exact, rho=1.0, jitter=1e-10):
    """The P lookup triangles M_p: column p of lookup = (Sigma_P \\ exact)^T reshaped to n x n (exact: P factors)."""
    E = np.stack([np.asarray(L, float).ravel(order="F") for L in exact])  # P x n^2, row p = to_row_vector(L_p)
    n = np.asarray(exact[0]).shape[0]
    X = np.linalg.solve(sigma_p(lp, rho, jitter), E)
    return [X[p].reshape((n, n), order="F") for p in range(X.shape[0])]


def gp_weights(l, lp, rho=1.0):
    """(w, dw/dl): Kp(l) and its derivative."""
    d = l - np.asarray(lp, float)
    w = np.exp(-(d * d) / (2.0 * rho * rho))
    return w, -d / (rho * rho) * w


def gp_L(l, lp, M, rho=1.0):
    w, _ = gp_weights(l, lp, rho)
    return sum(wp * Mp for wp, Mp in zip(w, M))


def gp_dL(l, lp, M, rho=1.0):
    _, wd = gp_weights(l, lp, rho)
    return sum(wp * Mp for wp, Mp in zip(wd, M))


def lp_value(f, y, l, sigma, z, lo, hi):
    z = np.asarray(z, float); y = np.asarray(y, float)
    n = z.size
    r = y - f
    return (-0.5 * float(z @ z) + 3.0 * math.log(l) - 4.0 * l - n * math.log(sigma) - 0.5 * float(r @ r) / sigma ** 2
            + math.log(l - lo) + math.log(hi - l) - math.log(hi - lo) + math.log(sigma))


def lp_grad(L, dL, y, l, sigma, z, lo, hi):
    """the analytic gradient in (l, sigma, z) for f = L z with dL = dL/dl"""
    z = np.asarray(z, float); y = np.asarray(y, float)
    n = z.size
    r = y - L @ z
    ubar = r / sigma ** 2
    g = np.empty(2 + n)
    g[0] = float(ubar @ (dL @ z)) + 3.0 / l - 4.0 + 1.0 / (l - lo) - 1.0 / (hi - l)
    g[1] = -n / sigma + float(r @ r) / sigma ** 3 + 1.0 / sigma
    g[2:] = L.T @ ubar - z
    return g


def hermite_model(orc, lp, Ls, dLs):
    """(L(l), dL/dl(l)) callables of the cubic Hermite model from the oracle's blend; dL/dl column by column from
    orc.approx_Lz_grad (the reverse-mode partial of cubic_interpolated_gp.hpp:6-32)."""
    n = Ls[0].shape[0]

    def L(l):
        return orc.approx_L(l, lp, Ls, dLs)

    def dL(l):
        return np.column_stack([orc.approx_Lz_grad(l, lp, Ls, dLs, e)[1] for e in np.eye(n)])

    return L, dL


def gp_model(lp, M, rho=1.0):
    return (lambda l: gp_L(l, lp, M, rho)), (lambda l: gp_dL(l, lp, M, rho))


def log_prob(L, y, l, sigma, z, lo, hi):
    return lp_value(L(l) @ np.asarray(z, float), y, l, sigma, z, lo, hi)


def log_prob_grad(L, dL, y, l, sigma, z, lo, hi):
    return lp_value(L(l) @ np.asarray(z, float), y, l, sigma, z, lo, hi), lp_grad(L(l), dL(l), y, l, sigma, z, lo, hi)
