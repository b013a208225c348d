"""CPU yardstick of gpmi_gp_predict and gpmi_seq_marginals, written from their formulas (include/gpmi.h) in numpy for float and
np.longdouble:

  predict:        Sigma = K(X, X) + (sigma^2 + jitter) I = L L^T, t_j = L^-1 K(X, xs_j), z = L^-1 y,
                  mean_j = t_j . z, var_j = alpha^2 - t_j . t_j;
  seq_marginals:  K~ = K(X, X) + jitter I = L L^T, B = I - L^-1 Kn L^-T, b = L^-1 mn,
                  mean_j = t_j . b, var_j = alpha^2 + jitter - t_j^T B t_j.

K is the ARD squared exponential alpha^2 exp(-1/2 sum_d ((x_d - y_d) / ell_d)^2) (QQard, R/kernels.R:11-19).  The Cholesky
factorisation and the forward substitution are loops over rows with vectorised bodies, so that they run in any numpy dtype
(numpy's LAPACK routines are float64 only).

Tolerances of the GPU parity tests (tests/test_gpu_predict.py), tied to this reference's own float64-vs-longdouble error by
tests/test_predict_reference.py:
  MEAN_TOL  relative error of the mean in the max norm (the bound the VJP tests use for their linear outputs);
  VAR_TOL   absolute error of the variance as a fraction of the prior variance alpha^2 -- var is a difference of O(alpha^2)
            terms and can itself be 1e-3 alpha^2 or less, so an error relative to var would measure its cancellation.
"""
import numpy as np

MEAN_TOL = 1e-9
VAR_TOL = 1e-9


def se_cov(X, Y, alpha, ell, dtype=float):
    X = np.asarray(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    D = X.shape[1]
    ell = np.broadcast_to(np.asarray(ell, dtype=dtype).ravel(), (D,)) if np.size(ell) == 1 else np.asarray(ell, dtype=dtype).ravel()
    s = np.zeros((X.shape[0], Y.shape[0]), dtype=dtype)
    for d in range(D):
        r = (X[:, d][:, None] - Y[:, d][None, :]) / ell[d]
        s = s + r * r
    return dtype(alpha) * dtype(alpha) * np.exp(-s / dtype(2))


def cholesky_rows(A):
    """Lower factor by the right-looking column form with vectorised updates (n = 300 well under a second); raises on a
    non-positive pivot."""
    A = np.array(A)
    n = A.shape[0]
    for j in range(n):
        d = A[j, j]
        if not d > 0:
            raise np.linalg.LinAlgError("leading minor of order %d is not positive" % (j + 1))
        d = np.sqrt(d)
        A[j, j] = d
        if j + 1 < n:
            A[j + 1:, j] = A[j + 1:, j] / d
            c = A[j + 1:, j]
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.outer(c, c)
    return np.tril(A)


def solve_lower(L, Bm):
    """L^-1 B for a matrix (or vector) B by forward substitution, one row at a time."""
    Bm = np.array(Bm, dtype=L.dtype)
    vec = Bm.ndim == 1
    if vec:
        Bm = Bm[:, None]
    n = L.shape[0]
    for i in range(n):
        if i:
            Bm[i] = Bm[i] - L[i, :i] @ Bm[:i]
        Bm[i] = Bm[i] / L[i, i]
    return Bm[:, 0] if vec else Bm


def predict(X, y, Xs, alpha, ell, sigma, jitter, dtype=float):
    """(mean, var) of the latent function at the rows of Xs."""
    X = np.asarray(X, dtype=dtype)
    Xs = np.asarray(Xs, dtype=dtype)
    n = X.shape[0]
    S = se_cov(X, X, alpha, ell, dtype) + (dtype(sigma) * dtype(sigma) + dtype(jitter)) * np.eye(n, dtype=dtype)
    L = cholesky_rows(S)
    T = solve_lower(L, se_cov(X, Xs, alpha, ell, dtype))       # n x m: column j is t_j
    z = solve_lower(L, np.asarray(y, dtype=dtype))
    return T.T @ z, dtype(alpha) * dtype(alpha) - np.sum(T * T, axis=0)


def seq_marginals(X, mn, Kn, alpha, ell, jitter, Xs, dtype=float):
    """(mean, var): the first step of a fresh create_p_dotXnS sampler at each row of Xs."""
    X = np.asarray(X, dtype=dtype)
    Xs = np.asarray(Xs, dtype=dtype)
    n = X.shape[0]
    L = cholesky_rows(se_cov(X, X, alpha, ell, dtype) + dtype(jitter) * np.eye(n, dtype=dtype))
    G = solve_lower(L, solve_lower(L, np.asarray(Kn, dtype=dtype)).T)   # L^-1 Kn L^-T (Kn symmetric)
    Bm = np.eye(n, dtype=dtype) - (G + G.T) / dtype(2)
    b = solve_lower(L, np.asarray(mn, dtype=dtype))
    T = solve_lower(L, se_cov(X, Xs, alpha, ell, dtype))
    return T.T @ b, dtype(alpha) * dtype(alpha) + dtype(jitter) - np.sum(T * (Bm @ T), axis=0)


def predict_lapack(X, y, Xs, alpha, ell, sigma, jitter):
    """predict(..., float) through numpy's LAPACK Cholesky on a column-major array: the yardstick at the full sizes."""
    import numpy.linalg as la
    X = np.asarray(X, float)
    n = X.shape[0]
    S = np.asfortranarray(se_cov(X, X, alpha, ell))
    S[np.diag_indices(n)] += sigma * sigma + jitter
    L = la.cholesky(S)
    del S
    Ks = se_cov(X, np.asarray(Xs, float), alpha, ell)
    rhs = np.concatenate([Ks, np.asarray(y, float)[:, None]], axis=1)
    try:
        from scipy.linalg import solve_triangular
        T = solve_triangular(L, rhs, lower=True)
    except ImportError:
        T = solve_lower(L, rhs)
    z = T[:, -1]
    T = T[:, :-1]
    return T.T @ z, alpha * alpha - np.sum(T * T, axis=0)


# ---- the project's inputs, seeded ------------------------------------------------------------------------------------------
def inputs(n, D, m, seed=0):
    """X ~ U[0, 1)^D, y = sin(2 pi sum x) + 0.1 eps, Xs ~ U[-0.1, 1.1)^D."""
    rng = np.random.default_rng(1000 + 7 * n + 13 * D + seed)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    y = np.sin(2 * np.pi * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    Xs = np.asfortranarray(rng.uniform(-0.1, 1.1, size=(m, D)))
    return X, y, Xs


ARD3 = (0.3, 0.5, 0.8)


def parity_cases():
    """(name, n, D, m, alpha, ell, sigma, jitter) of the GPU parity test; sigma >= 0.05 (a noise-free fit is ill-conditioned
    beyond what the two tolerances are for: status and property tests cover it)."""
    return [
        ("n21_d1", 21, 1, 41, 1.0, (0.3,), 0.05, 1e-6),
        ("n100_d1", 100, 1, 64, 1.0, (0.3,), 0.1, 1e-6),
        ("n300_d3_iso", 300, 3, 128, 1.0, (0.3,), 0.1, 1e-6),
        ("n300_d3_ard", 300, 3, 128, 1.0, ARD3, 0.05, 1e-6),
        ("n1024_d3", 1024, 3, 1000, 1.0, (0.3,), 0.1, 1e-6),
        ("n4096_d3", 4096, 3, 1537, 1.0, ARD3, 0.1, 1e-6),
    ]


def max_rel(a, b):
    a = np.asarray(a, float)
    b = np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
