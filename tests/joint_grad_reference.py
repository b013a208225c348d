"""CPU reference for gpmi_joint_logml_grad: value and gradient of the log marginal likelihood of stacked observations
yy = [y; y'] under the joint matrix of R/ode_gp_library.R:29-30 (gpmi_joint_cov, flags = 0).  A dense numpy restatement in
float64 (LAPACK) and in np.longdouble (factorisation and inverse by plain loops).  Helper of
tests/test_joint_grad_reference.py and tests/test_gpu_joint_grad.py (not collected: no test_ prefix).

With r = t_i - t_j, e = exp(-r^2 / (2 l^2)), u = r^2 / l^2 and n points (N = 2n):
  QQ0 = alpha^2 e,  QR = alpha^2 e r / l^2 = S[i, n + j] (S[n + i, j] = -QR_ij),  RR0 = alpha^2 e (1 - u) / l^2,
  S = [[QQ0 + (sigma^2 + jitter) I, QR], [QR^T, RR0 + jitter I]] = L L^T,  z = L^-1 yy,  a = S^-1 yy,
  out3 = (-z'z / 2 - sum_i log L_ii - n log(2 pi), sum_i log L_ii, z'z),
  grad_theta = sum_pq G_pq dS_pq / dtheta,  G = (a a' - S^-1) / 2,  theta in (alpha, l, sigma),
  dS/dalpha = 2 / alpha (S without its diagonal additions),  dS/dsigma = 2 sigma on the first n diagonal entries,
  dQQ0/dl = QQ0 u / l,  dQR/dl = QR (u - 2) / l,  dRR0/dl = alpha^2 e (-u^2 + 5u - 2) / l^3.
"""
import functools

import numpy as np

EPS = float(np.finfo(float).eps)
COND_MAX = 2e7            # a condition on the parity inputs (tests/test_joint_grad_reference.py), not a measurement
PARITY_ALPHA, PARITY_SIGMA, PARITY_JITTER = 1.1, 0.1, 1e-3
# (n, l): a single point; a ragged 64-tile; the reference's own size; a full tile and one point past it; odd n; orders 130 and
# 258 (one and two points past a 128-column panel and a 256 boundary); the largest order (700) the long-double loops take
PARITY_CASES = ((1, 0.5), (7, 0.5), (21, 0.9), (64, 0.3), (65, 0.3), (129, 0.2), (350, 0.1))


def joint_parts(t, alpha, l, sigma, jitter, dtype=float):
    """(S, (dS/dalpha, dS/dl, dS/dsigma)) in `dtype`, all of order 2n and symmetric."""
    t = np.asarray(t, float).astype(dtype)
    n = t.size
    a2, l2 = dtype(alpha) * dtype(alpha), dtype(l) * dtype(l)
    r = t[:, None] - t[None, :]
    u = r * r / l2
    qq = a2 * np.exp(-(r * r / (2 * l2)))
    qr = qq * r / l2
    rr = qq * (1 - u) / l2
    eye = np.eye(n, dtype=dtype)
    K = np.block([[qq, qr], [qr.T, rr]])
    S = K + np.block([[(dtype(sigma) * dtype(sigma) + dtype(jitter)) * eye, 0 * eye], [0 * eye, dtype(jitter) * eye]])
    dl = np.block([[qq * u, qr * (u - 2)], [(qr * (u - 2)).T, qq * (-u * u + 5 * u - 2) / l2]]) / dtype(l)
    ds = np.block([[2 * dtype(sigma) * eye, 0 * eye], [0 * eye, 0 * eye]])
    return S, (2 / dtype(alpha) * K, dl, ds)


def _chol_loops(S):
    n = S.shape[0]
    L = np.zeros_like(S)
    for j in range(n):
        L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _lower_inverse_loops(L):
    n = L.shape[0]
    X = np.zeros_like(L)
    for i in range(n):
        e = np.zeros(n, dtype=L.dtype)
        e[i] = 1
        X[i] = (e - L[i, :i] @ X[:i]) / L[i, i]
    return X


def joint_reference(t, yy, alpha, l, sigma, jitter, dtype=float):
    """dict: S, out3 (3,), grad (3,), gabs (3, float: sum_pq |G_pq dS_pq / dtheta|, the scale of the contraction's rounding)."""
    n = np.asarray(t).size
    S, dS = joint_parts(t, alpha, l, sigma, jitter, dtype)
    y = np.asarray(yy, float).astype(dtype)
    if dtype is float:
        L = np.linalg.cholesky(S)
        Linv = np.linalg.solve(L, np.eye(2 * n))
    else:
        L = _chol_loops(S)
        Linv = _lower_inverse_loops(L)
    z = Linv @ y
    a = Linv.T @ z
    Sinv = Linv.T @ Linv
    sld, q = np.log(np.diag(L)).sum(), z @ z
    two_pi = 2 * (np.pi if dtype is float else dtype(4) * np.arctan(dtype(1)))
    out3 = np.array([-q / 2 - sld - n * np.log(two_pi), sld, q], dtype=dtype)
    G = (np.outer(a, a) - Sinv) / 2
    grad = np.array([np.sum(G * d) for d in dS], dtype=dtype)
    gabs = np.array([float(np.sum(np.abs(G * d))) for d in dS])
    return {"S": S, "out3": out3, "grad": grad, "gabs": gabs}


def cond2(S):
    """cond_2 of a symmetric positive definite matrix in float64: the ratio of its extreme eigenvalues."""
    w = np.linalg.eigvalsh(np.asarray(S, float))
    return float(w[-1] / w[0])


def case_inputs(n, seed=None):
    """(t, yy) of a parity case: t uniform on [-1, 1], yy = [y; y'] of a smooth function plus noise, fixed by n."""
    rng = np.random.default_rng(9000 + n if seed is None else seed)
    t = rng.uniform(-1.0, 1.0, n)
    y = np.sin(3 * t) + 0.1 * rng.standard_normal(n)
    dy = 3 * np.cos(3 * t) + 0.1 * rng.standard_normal(n)
    return t, np.concatenate([y, dy])


@functools.lru_cache(maxsize=None)
def parity_reference(case, longdouble=True):
    """((t, yy), reference dict, cond_2(S)) of one entry of PARITY_CASES, computed once per process."""
    n, l = case
    t, yy = case_inputs(n)
    ref = joint_reference(t, yy, PARITY_ALPHA, l, PARITY_SIGMA, PARITY_JITTER, np.longdouble if longdouble else float)
    return (t, yy), ref, cond2(ref["S"])
