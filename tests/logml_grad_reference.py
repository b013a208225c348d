"""CPU reference for gpmi_logml_grad / gpmi_logml_grad_grid: value and gradient of the log marginal likelihood of
models/fit_hyperparameters.stan:18-32 with ARD length-scales, in float64 (LAPACK) and in np.longdouble (plain loops).  Built on
tests/vjp_reference.py (covariance, its derivatives, long-double factorisation) and tests/centered_gp_reference.py (the backward
substitution, cond_2).  Helper of tests/test_logml_grad_reference.py and tests/test_gpu_logml_grad_parity.py (not collected: no
test_ prefix).

With S = alpha^2 K0(X; ell) + (sigma^2 + jitter) I = L L^T, z = L^-1 y, a = S^-1 y:
  out3 = (-z'z / 2 - sum_i log L_ii - n / 2 log(2 pi), sum_i log L_ii, z'z),
  grad_theta = sum_ij G_ij dS_ij / dtheta, G = (a a' - S^-1) / 2, theta in (alpha, ell_0 .., sigma),
  dS/dsigma = 2 sigma I: grad_sigma = sigma (a'a - tr S^-1).
This is centered_gp_reference.centered_reference(X, alpha, ell, y[:, None], "none", jitter=sigma^2 + jitter) plus d/dsigma
(tests/test_logml_grad_reference.py asserts the identity).

The floor of the bound on sum_i log L_ii.  tests/test_gpu_joint_grad.py bounds out3[1] by 10 cond eps, relative.  That alone does
not hold here, because the logs can cancel while each log L_ii carries the RELATIVE error of L_ii as an ABSOLUTE error
whatever the sum comes to: on CANCEL_CASE (n = 2, cond = 10, det S = 1 to rounding, sum_log = 7e-17 from terms of 0.27) the
float64 (LAPACK) value is 2.9 eps off, nine times its own size.  So
  |sum_log - ref| <= 10 cond eps |ref| + SUM_LOG_FLOOR_C n eps,
SUM_LOG_FLOOR_C the smallest power of two for which the float64 value stays within HALF of that bound on every parity input,
measured on the CPU against the long-double value (never against the device): c = 4.  The worst float64 error is then 0.37 of
the bound (CANCEL_CASE: 2.94 eps of 8 eps; c = 2 leaves it at 0.73); no other parity input uses more than 0.09 of it.
"""
import functools
import math

import numpy as np

import centered_gp_reference as cg
import vjp_reference as vr

EPS = float(np.finfo(float).eps)
COND_MAX = 2e7            # a condition on the parity inputs (tests/test_logml_grad_reference.py), not a measurement
PARITY_ALPHA, PARITY_JITTER = 1.3, 1e-6
SIGMAS = (0.15, 1e-3, 0.0)
SUM_LOG_FLOOR_C = 4.0     # see the module docstring
MAXD = 8                  # up to here the register-resident contraction (k_grad_partial) and the one-workgroup kernel

# one workgroup: the 64-row tile, the 128 panel, the 16-wide load groups of a = U z, the row-pair stores of U = I at odd n, the
# LDS coordinate buffers at n = 256, D = 8
ONE_WG_SIZES = (1, 2, 17, 63, 64, 65, 127, 128, 129, 193, 255, 256)
CHAIN_SIZES = (1, 2, 63, 65, 129, 257, 385)
SMALL_LAYOUTS = ((1, False), (8, True), (2, True), (3, False), (5, True), (8, False), (1, True), (2, False), (3, True), (5, False))
# D > 8 (k_grad_partial_big): grad_ns rounded up to 8, exactly one 16-dimension stage, one past it, two stages and one past
# them, four stages
BIG_LAYOUTS = ((9, True), (64, False), (17, True), (33, False), (16, True), (9, False), (64, True), (17, False), (33, True), (16, False))
DUP = 5                   # coincident points of the "dup" cases (n = 65, sigma = 0.15)
# n = 2, D = 1 with the distance chosen so that det S = 1: log L_00 = -log L_11 and sum_i log L_ii cancels to rounding (cond 10)
CANCEL_CASE = (2, 1, False, 0.15, "cancel")


def _cases():
    """(one-workgroup cases, chain cases), each (n, D, ard, sigma, variant): the layouts rotate over the sizes (no cross
    product, as centered_gp_reference.parity_cases) and the noise level over the cases; variant "" (plain), "dup" (coincident
    points: r = 0 off the diagonal) or "cancel" (CANCEL_CASE)."""
    one, chain = [], []
    for ni, n in enumerate(ONE_WG_SIZES):
        for q in (0, 1):
            D, ard = SMALL_LAYOUTS[(ni + 5 * q) % 10]
            one.append((n, D, ard, SIGMAS[(ni + q) % 3], ""))
    one.append((65, 3, True, 0.15, "dup"))
    one.append(CANCEL_CASE)
    for ni, n in enumerate(CHAIN_SIZES):
        for q in (0, 1):
            D, ard = SMALL_LAYOUTS[(2 * ni + q + 3) % 10]
            chain.append((n, D, ard, SIGMAS[(ni + q) % 3], ""))
            D, ard = BIG_LAYOUTS[(2 * ni + q) % 10]
            chain.append((n, D, ard, SIGMAS[(ni + q + 1) % 3], ""))
    chain.append((65, 2, False, 0.15, "dup"))
    chain.append((65, 17, True, 0.15, "dup"))
    chain.append(CANCEL_CASE)
    return tuple(one), tuple(chain)


ONE_WG_CASES, CHAIN_CASES = _cases()
PARITY_CASES = tuple(dict.fromkeys(ONE_WG_CASES + CHAIN_CASES))


def case_id(case):
    n, D, ard, sigma, variant = case
    return "n%d-D%d-%s-s%g%s" % (n, D, "ard" if ard else "iso", sigma, "-" + variant if variant else "")


def case_inputs(n, D, ard, sigma, variant=""):
    """(X, y, alpha, ell, sigma, jitter), deterministic in the arguments.  D <= 8: the layout of
    centered_gp_reference.parity_case, about one point per length-scale, X = U(0, 1)^D mean(ell) n^(1/D).  D > 8: that layout
    gives a nearly diagonal matrix (cond 1.5 at D = 64); X = U(0, 1)^D ell sqrt(18 / D) instead, so that the scaled squared
    distance sum_d ((x_d - y_d) / ell_d)^2 has mean D (18 / D) / 6 = 3.  variant "dup": the last DUP rows repeat the first
    ones; "cancel" (n = 2, D = 1, isotropic): the second point at the distance where K0 = sqrt((alpha^2 + d)^2 - 1) / alpha^2,
    d = sigma^2 + jitter, so that det S = 1."""
    rng = np.random.default_rng(100000 * n + 100 * D + (1 if ard else 0))
    ell = 0.6 + 0.4 * rng.random(D) if ard else np.array([0.8])
    if D <= MAXD:
        X = rng.random((n, D)) * (float(np.mean(ell)) * n ** (1.0 / D))
    else:
        X = rng.random((n, D)) * (ell * math.sqrt(18.0 / D))
    y = np.sin(3 * X.sum(axis=1) / math.sqrt(D)) + 0.1 * rng.standard_normal(n)
    if variant == "dup":
        X[n - DUP:] = X[:DUP]
    elif variant == "cancel":
        dd = PARITY_ALPHA ** 2 + float(sigma) ** 2 + PARITY_JITTER
        X[1] = X[0] + ell[0] * math.sqrt(-2.0 * math.log(math.sqrt(dd * dd - 1.0) / PARITY_ALPHA ** 2))
    return X, y, PARITY_ALPHA, ell, float(sigma), PARITY_JITTER


def scaled_sq_dist(X, ell):
    """The off-diagonal scaled squared distances sum_d ((x_id - x_jd) / ell_d)^2, i > j."""
    X = np.asarray(X, float).reshape(len(X), -1)
    Z = X / vr._ells(ell, X.shape[1])
    R = ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(axis=2)
    return R[np.tril_indices(len(X), -1)]


def logml_grad_reference(X, y, alpha, ell, sigma, jitter, dtype=float):
    """The whole call in `dtype`: float (LAPACK factorisation and solves) or np.longdouble (plain loops).  Returns a dict:
    out3 (3,), grad (2 + n_ell,), gabs (2 + n_ell, float: per theta the sum of the absolute terms of the contraction,
    1/2 sum_ij (|a_i a_j| + |S^-1_ij|) |dS_ij / dtheta|; for sigma |sigma| (a'a + sum_i |S^-1_ii|))."""
    X = np.asarray(X, float).reshape(len(X), -1)
    n = X.shape[0]
    yv = np.asarray(y, float).astype(dtype)
    n_ell = np.atleast_1d(ell).size
    sg = dtype(sigma)
    K, _, _ = vr.se_cov(X, alpha, ell, sg * sg + dtype(jitter), dtype=dtype)
    if dtype is float:
        L = np.linalg.cholesky(K)
        Linv = np.linalg.solve(L, np.eye(n))
        z = np.linalg.solve(L, yv)
        a = np.linalg.solve(L.T, z)
    else:
        L = vr._chol_ld(K)
        Linv = vr._fwd_solve_ld(L, np.eye(n, dtype=dtype))
        z = vr._fwd_solve_ld(L, yv)
        a = cg._bwd_solve_ld(L, z)
    Sinv = Linv.T @ Linv
    sld, q = np.log(np.diag(L)).sum(), z @ z
    two_pi = 2 * (np.pi if dtype is float else dtype(4) * np.arctan(dtype(1)))
    out3 = np.array([-q / 2 - sld - n * np.log(two_pi) / 2, sld, q], dtype=dtype)
    AA = np.outer(a, a)
    G = (AA - Sinv) / 2
    Gabs = (np.abs(AA) + np.abs(Sinv)) / 2
    dKs = vr.dK_dtheta(X, alpha, ell, n_ell, dtype=dtype)
    grad = np.array([np.sum(G * dk) for dk in dKs] + [sg * (a @ a - np.trace(Sinv))], dtype=dtype)
    gabs = np.array([float(np.sum(Gabs * np.abs(dk))) for dk in dKs] + [float(abs(sg) * (a @ a + np.abs(np.diag(Sinv)).sum()))])
    return {"out3": out3, "grad": grad, "gabs": gabs}


def cond2(X, alpha, ell, sigma, jitter):
    """cond_2(S) in float64."""
    return cg.cond2(X, alpha, ell, float(sigma) ** 2 + jitter)


@functools.lru_cache(maxsize=None)
def parity_reference(case, longdouble=True):
    """(inputs, reference dict, cond_2(S)) of one (n, D, ard, sigma, variant), computed once per process."""
    inp = case_inputs(*case)
    ref = logml_grad_reference(*inp, dtype=np.longdouble if longdouble else float)
    return inp, ref, cond2(inp[0], inp[2], inp[3], inp[4], inp[5])


@functools.lru_cache(maxsize=None)
def point_reference(case, alpha, rho, sigma, jitter):
    """(reference dict, cond_2(S)) in long double on the inputs of `case` at another isotropic (alpha, rho, sigma): the grid."""
    X, y = case_inputs(*case)[:2]
    return logml_grad_reference(X, y, alpha, [rho], sigma, jitter, np.longdouble), cond2(X, alpha, [rho], sigma, jitter)


def bounds(ref, cond, n, scale=1.0):
    """(bound on |sum_log - ref|, relative bound on z'z, per-theta bound on |grad - ref|) for a backward-stable float64
    evaluation (the module docstring; tests/test_gpu_joint_grad.py), all times `scale` (1: the device against the reference;
    2: two device evaluations against each other)."""
    ce = cond * EPS
    gmax = float(np.max(np.abs(ref["grad"])))
    return (scale * (10.0 * ce * abs(float(ref["out3"][1])) + SUM_LOG_FLOOR_C * n * EPS), scale * 10.0 * ce,
            scale * (10.0 * ce * gmax + 32.0 * EPS * ref["gabs"]))


def errors(out3, grad, ref):
    """(|sum_log - ref|, relative error of z'z, |grad - ref| per theta) of a float64 result against the long-double one."""
    o = np.asarray(out3, np.longdouble)
    return (abs(float(o[1] - ref["out3"][1])), abs(float((o[2] - ref["out3"][2]) / ref["out3"][2])),
            np.abs(np.asarray(grad, np.longdouble) - ref["grad"]).astype(float))


def value_bound(ref, cond, n, scale=1.0):
    """Bound on |logml - ref| = |(z'z - ref) / 2 + (sum_log - ref)|: the two parts' bounds added."""
    bs, bq, _ = bounds(ref, cond, n, scale)
    return 0.5 * bq * abs(float(ref["out3"][2])) + bs
