"""CPU references for the vector-Jacobian product of the latent exact GP's transform (models/exact_gp.stan:17-25):
F = L Z, L = chol(K), K = alpha^2 K0(ell) + jitter I, upstream adjoint Fbar.  Helper of tests/test_exact_gp_vjp_reference.py
and tests/test_gpu_exact_gp_vjp.py (not collected: no test_ prefix).

- vjp_reverse: float64 reverse mode, Zbar = L^T Fbar, Sbar = sym(U Phi(Zbar Z^T) U^T), U = L^-T, theta_bar = <Sbar, dK/dtheta>.
- vjp_forward_longdouble: np.longdouble forward mode, theta_bar = sum(Fbar o (L Phi(L^-1 dK L^-T) Z)), plain loops.
- suffix_V: V = U Phi(W Z^T) in O(n^2 k) by suffix sums along the rows of U o w_c (the form the kernels use).
"""
import numpy as np


def _ells(ell, D):
    ell = np.atleast_1d(np.asarray(ell, dtype=float))
    return np.full(D, ell[0]) if ell.size == 1 else ell


def r2_parts(X):
    """(n, n, D) squared coordinate differences."""
    X = np.asarray(X, float).reshape(X.shape[0], -1)
    return (X[:, None, :] - X[None, :, :]) ** 2


def se_cov(X, alpha, ell, jitter, dtype=float):
    X = np.asarray(X, float)
    X = X.reshape(X.shape[0], -1)
    e = _ells(ell, X.shape[1]).astype(dtype)
    R2 = r2_parts(X).astype(dtype)
    K0 = np.exp(-0.5 * (R2 / e ** 2).sum(axis=2))
    return dtype(alpha) ** 2 * K0 + dtype(jitter) * np.eye(X.shape[0], dtype=dtype), K0, R2


def dK_dtheta(X, alpha, ell, n_ell, dtype=float):
    """[dK/dalpha, dK/dell_0, ...] (n_ell = 1: one isotropic length-scale)."""
    X = np.asarray(X, float).reshape(len(X), -1)
    D = X.shape[1]
    e = _ells(ell, D).astype(dtype)
    _, K0, R2 = se_cov(X, alpha, ell, 0.0, dtype)
    a = dtype(alpha)
    Kse = a * a * K0
    out = [2 * a * K0]
    if n_ell == 1:
        out.append(Kse * R2.sum(axis=2) / e[0] ** 3)
    else:
        out += [Kse * R2[:, :, d] / e[d] ** 3 for d in range(D)]
    return out


def phi(A):
    B = np.tril(A)
    B[np.diag_indices_from(B)] *= 0.5
    return B


def vjp_reverse(X, alpha, ell, Z, Fbar, jitter):
    """(F, Zbar, grad) in float64; Z, Fbar n x k."""
    Z = np.asarray(Z, float).reshape(len(Z), -1)
    Fb = np.asarray(Fbar, float).reshape(len(Z), -1)
    n_ell = np.atleast_1d(ell).size
    K, _, _ = se_cov(X, alpha, ell, jitter)
    L = np.linalg.cholesky(K)
    F = L @ Z
    W = L.T @ Fb
    U = np.linalg.inv(L).T
    S = U @ phi(W @ Z.T) @ U.T
    Sb = 0.5 * (S + S.T)
    grad = np.array([np.sum(Sb * dk) for dk in dK_dtheta(X, alpha, ell, n_ell)])
    return F, W, grad


def suffix_V(U, W, Z):
    """V = U Phi(W Z^T) for upper-triangular U: V_ij = sum_c z_cj (sum_{m >= max(i, j + 1)} U_im w_cm + 1/2 U_ij w_cj)."""
    n, k = W.shape
    V = np.zeros((n, n))
    for c in range(k):
        T = U * W[:, c][None, :]                                     # T_im = U_im w_cm
        S = np.cumsum(T[:, ::-1], axis=1)[:, ::-1]                   # S_ij = sum_{m >= j} T_im
        P = np.concatenate([S[:, 1:], np.zeros((n, 1))], axis=1)     # sum_{m >= j + 1}
        V += (P + 0.5 * T) * Z[:, c][None, :]
    return V


def _chol_ld(K):
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        s = K[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _fwd_solve_ld(L, B):
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def vjp_forward_longdouble(X, alpha, ell, Z, Fbar, jitter):
    """theta_bar by forward mode in np.longdouble: for each theta, Ldot = L Phi(L^-1 Kdot L^-T), theta_bar = sum(Fbar o Ldot Z)."""
    ld = np.longdouble
    Z = np.asarray(Z, float).reshape(len(Z), -1).astype(ld)
    Fb = np.asarray(Fbar, float).reshape(len(Z), -1).astype(ld)
    n_ell = np.atleast_1d(ell).size
    K, _, _ = se_cov(X, alpha, ell, jitter, dtype=ld)
    L = _chol_ld(K)
    out = []
    for Kd in dK_dtheta(X, alpha, ell, n_ell, dtype=ld):
        A = _fwd_solve_ld(L, Kd)               # L^-1 Kdot
        M = _fwd_solve_ld(L, A.T.copy())       # L^-1 (L^-1 Kdot)^T = L^-1 Kdot L^-T
        Ld = L @ phi(M)
        out.append(np.sum(Fb * (Ld @ Z)))
    return np.array(out, dtype=ld)


def central_diff(fun, theta, h_rel=1e-5):
    """Central differences of the scalar fun(theta) in every component."""
    theta = np.asarray(theta, float)
    g = np.empty(theta.size)
    for i in range(theta.size):
        h = h_rel * max(abs(theta[i]), 1.0)
        tp = theta.copy(); tm = theta.copy()
        tp[i] += h; tm[i] -= h
        g[i] = (fun(tp) - fun(tm)) / (2 * h)
    return g


def exact_gp_lp(x, y, l, sigma, z):
    """lp__ of models/exact_gp.stan restated in numpy (`~` drops constants; <lower=0> Jacobians log l + log sigma)."""
    x = np.asarray(x, float); y = np.asarray(y, float); z = np.asarray(z, float)
    K = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / l ** 2) + 1e-10 * np.eye(x.size)
    f = np.linalg.cholesky(K) @ z
    return (-0.5 * z @ z + 3.0 * np.log(l) - 4.0 * l - x.size * np.log(sigma) - 0.5 * np.sum((y - f) ** 2) / sigma ** 2
            + np.log(l) + np.log(sigma))
