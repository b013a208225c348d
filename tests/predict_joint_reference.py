"""CPU yardstick of gpmi_gp_predict_joint, written from its formulas (include/gpmi.h) with the building blocks of
tests/predict_reference.py, in numpy for float and np.longdouble:

  Sigma = K(X, X) + (sigma^2 + jitter) I = L L^T,  T = L^-1 K(X, Xs) (n x m),  z = L^-1 y,
  mean = T^T z,   C = K(Xs, Xs) - T^T T + post_jitter I   (the latent function's covariance: alpha^2 on the diagonal of K(Xs, Xs)).

The GPU tests (tests/test_gpu_predict_joint.py) hold the mean to predict_reference.MEAN_TOL relative in the max norm and the
covariance to VAR_TOL alpha^2 absolute in the max norm -- gpmi_gp_predict's two tolerances, for the same reason: the entries of C
are differences of O(alpha^2) terms.  tests/test_predict_joint_reference.py ties both to this reference's own error."""
import numpy as np

import predict_reference as pr

JITTER = 1e-6
POST_JITTER = 1e-6


def joint(X, y, Xs, alpha, ell, sigma, jitter, post_jitter, dtype=float):
    """(mean (m,), C (m, m)) of the latent function at the rows of Xs."""
    X = np.asarray(X, dtype=dtype)
    Xs = np.asarray(Xs, dtype=dtype)
    n, m = X.shape[0], Xs.shape[0]
    S = pr.se_cov(X, X, alpha, ell, dtype) + (dtype(sigma) * dtype(sigma) + dtype(jitter)) * np.eye(n, dtype=dtype)
    L = pr.cholesky_rows(S)
    T = pr.solve_lower(L, pr.se_cov(X, Xs, alpha, ell, dtype))
    z = pr.solve_lower(L, np.asarray(y, dtype=dtype))
    Kss = pr.se_cov(Xs, Xs, alpha, ell, dtype)
    Kss[np.diag_indices(m)] = dtype(alpha) * dtype(alpha)
    return T.T @ z, Kss - T.T @ T + dtype(post_jitter) * np.eye(m, dtype=dtype)


def joint_lapack(X, y, Xs, alpha, ell, sigma, jitter, post_jitter):
    """joint(..., float) through numpy's LAPACK Cholesky (predict_reference.predict_lapack's way): the yardstick at the mid size."""
    import numpy.linalg as la
    X = np.asarray(X, float)
    Xs = np.asarray(Xs, float)
    n, m = X.shape[0], Xs.shape[0]
    S = np.asfortranarray(pr.se_cov(X, X, alpha, ell))
    S[np.diag_indices(n)] += sigma * sigma + jitter
    L = la.cholesky(S)
    del S
    rhs = np.concatenate([pr.se_cov(X, Xs, alpha, ell), np.asarray(y, float)[:, None]], axis=1)
    try:
        from scipy.linalg import solve_triangular
        T = solve_triangular(L, rhs, lower=True)
    except ImportError:
        T = pr.solve_lower(L, rhs)
    z = T[:, -1]
    T = T[:, :-1]
    Kss = pr.se_cov(Xs, Xs, alpha, ell)
    Kss[np.diag_indices(m)] = alpha * alpha
    return T.T @ z, Kss - T.T @ T + post_jitter * np.eye(m)


def _ell(D):
    return tuple(np.linspace(0.3, 0.8, D) * np.sqrt(D / 3.0))


def cases():
    """(name, n, D, m, alpha, ell, sigma) with inputs predict_reference.inputs(n, D, m); jitter JITTER, post_jitter POST_JITTER."""
    return [
        ("n21_d1", 21, 1, 41, 1.0, (0.3,), 0.05),
        ("n21_d3", 21, 3, 41, 1.0, pr.ARD3, 0.05),
        ("n100_d3", 100, 3, 64, 1.0, pr.ARD3, 0.1),
        ("n130_d8", 130, 8, 125, 1.5, _ell(8), 0.1),
        ("n300_d3", 300, 3, 259, 1.0, pr.ARD3, 0.05),
        ("n700_d3", 700, 3, 300, 1.0, (0.3,), 0.1),
        ("n300_d17", 300, 17, 200, 1.0, _ell(17), 0.1),
    ]


def case(name):
    for c in cases():
        if c[0] == name:
            return c
    raise KeyError(name)
