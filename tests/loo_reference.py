"""CPU reference for gpmi_logml_loo: exact leave-one-out cross-validation of the GP of models/fit_hyperparameters.stan:18-32
(Rasmussen & Williams, section 5.4.2) in np.longdouble (plain loops), and the device's algebra in float64 (LAPACK).  Built on
tests/vjp_reference.py (covariance, its derivatives, long-double factorisation), tests/centered_gp_reference.py (the backward
substitution) and the inputs of tests/logml_grad_reference.py.  Helper of tests/test_loo_reference.py and tests/test_gpu_loo.py
(not collected: no test_ prefix).

With S = alpha^2 K0(X; ell) + (sigma^2 + jitter) I, A = S^-1, a = A y, d = diag A:
  mu_i = y_i - a_i / d_i,  var_i = 1 / d_i (of the observation),  lpd_i = -1/2 log(2 pi) + 1/2 log d_i - a_i^2 / (2 d_i),
  loo = sum_i lpd_i,
  d loo / d theta = sum_i (a_i [Z a]_i - 1/2 (1 + a_i^2 / d_i) [Z A]_ii) / d_i,  Z = A dS/dtheta        (R&W 5.13),
one matrix product PER hyper-parameter: the reference gradient (loo_reference).  The device forms
  G = (b a' + a b') / 2 - A diag(v) A,  u = a / d,  v = (1 + a^2 / d) / (2 d),  b = A u,  d loo / d theta = sum_kl G_kl dS_kl,
which loo_identity states in any dtype; the reference never uses it.

Bounds (the form of tests/logml_grad_reference.py), for a float64 evaluation against the long-double one, C = BOUND_C:
  var_i:  C cond eps, relative;
  mu_i:   C cond eps (|y_i| + max_j |a_j| / d_i);
  lpd_i = -1/2 log(2 pi) - 1/2 log var_i - r_i^2 / (2 var_i), r_i = y_i - mu_i, the two bounds propagated:
          bvar / 2 + |r_i| bmu_i / var_i + r_i^2 / (2 var_i) bvar + LPD_FLOOR_C eps   (bvar the relative bound on var_i);
  loo:    sum_i of the lpd_i bounds;
  grad:   C cond eps max|grad| + 32 eps gabs_theta, gabs_theta = sum_kl ((|a_k b_l| + |b_k a_l|) / 2 + (|A| diag(v) |A|)_kl) |dS_kl|,
          the sum of the absolute terms of the contraction.
C starts at 10 and is the smallest of 10, 16, 32, ... for which the float64 implementation (loo_float64) stays within HALF of
every bound on every parity input (logml_grad_reference.CHAIN_CASES), measured on the CPU against the long-double value,
never against the device.  Measured worst error / bound of the float64 implementation at C = 10, LPD_FLOOR_C = 8 (print them
with `python tests/loo_reference.py`): var 0.100 (n = 1), mu 0.012, lpd 0.063, loo 0.036, grad 0.054 (the n = 2 case whose
log-determinant cancels) -- so C = 10 stands.  The floor is not measured but reasoned: where the propagated terms vanish,
lpd_i is -0.92 plus half a log below 8 (d_i <= 1e6 here) plus a small quadratic term; the log and the two additions are each
rounded to half an ulp of a number below 8, 2 eps each: 6 eps, and the next power of two is c = 8.
"""
import functools

import numpy as np

import centered_gp_reference as cg
import logml_grad_reference as lg
import vjp_reference as vr

EPS = lg.EPS
BOUND_C = 10.0
LPD_FLOOR_C = 8.0
CASES = lg.CHAIN_CASES
# the inputs of the test that needs no formula: every point deleted in turn (n = 17), five of them (n = 65)
DELETE_CASES = (((17, 2, False, 0.15, ""), tuple(range(17))), ((65, 3, True, 0.15, ""), (0, 13, 32, 51, 64)))


def _inverse(X, y, alpha, ell, sigma, jitter, dtype):
    """(S, A = S^-1, a = A y) in `dtype`: float (LAPACK) or np.longdouble (plain loops)."""
    X = np.asarray(X, float).reshape(len(X), -1)
    n = X.shape[0]
    yv = np.asarray(y, float).astype(dtype)
    sg = dtype(sigma)
    S, _, _ = vr.se_cov(X, alpha, ell, sg * sg + dtype(jitter), dtype=dtype)
    if dtype is float:
        L = np.linalg.cholesky(S)
        Linv = np.linalg.solve(L, np.eye(n))
        a = np.linalg.solve(L.T, np.linalg.solve(L, yv))
    else:
        L = vr._chol_ld(S)
        Linv = vr._fwd_solve_ld(L, np.eye(n, dtype=dtype))
        a = cg._bwd_solve_ld(L, vr._fwd_solve_ld(L, yv))
    return S, Linv.T @ Linv, a


def _points(yv, A, a, dtype):
    d = np.diag(A).copy()
    two_pi = 2 * (np.pi if dtype is float else dtype(4) * np.arctan(dtype(1)))
    lpd = -np.log(two_pi) / 2 + np.log(d) / 2 - a * a / (2 * d)
    return d, {"mu": yv - a / d, "var": 1 / d, "lpd": lpd, "loo": lpd.sum()}


def _dS(X, alpha, ell, sigma, dtype):
    """dS/dtheta for theta in (alpha, ell.., sigma)."""
    X = np.asarray(X, float).reshape(len(X), -1)
    n_ell = np.atleast_1d(ell).size
    return vr.dK_dtheta(X, alpha, ell, n_ell, dtype=dtype) + [2 * dtype(sigma) * np.eye(X.shape[0], dtype=dtype)]


def loo_reference(X, y, alpha, ell, sigma, jitter, dtype=np.longdouble, want_grad=True):
    """The whole call in `dtype`, the gradient by R&W (5.13), one product per hyper-parameter.  Returns a dict: mu, var, lpd
    (n,), loo, grad (2 + n_ell,), gabs (2 + n_ell, float: the module docstring), amax (max_j |a_j|, float), y."""
    yv = np.asarray(y, float).astype(dtype)
    _, A, a = _inverse(X, y, alpha, ell, sigma, jitter, dtype)
    d, out = _points(yv, A, a, dtype)
    out.update(amax=float(np.max(np.abs(a))), y=np.asarray(y, float))
    if not want_grad:
        return out
    w = (1 + a * a / d) / 2
    grad = []
    for dS in _dS(X, alpha, ell, sigma, dtype):
        Z = A @ dS
        grad.append(np.sum((a * (Z @ a) - w * np.sum(Z * A, axis=1)) / d))   # [Z A]_ii = sum_k Z_ik A_ik: A is symmetric
    out["grad"] = np.array(grad, dtype=dtype)
    out["gabs"] = _gabs(X, alpha, ell, sigma, A, a, d, dtype)
    return out


def _identity_G(A, a, d):
    u, v = a / d, (1 + a * a / d) / (2 * d)
    b = A @ u
    M = A * np.sqrt(v)[None, :]
    return (np.outer(b, a) + np.outer(a, b)) / 2 - M @ M.T, b, v


def _gabs(X, alpha, ell, sigma, A, a, d, dtype):
    _, b, v = _identity_G(A, a, d)
    Gabs = (np.abs(np.outer(b, a)) + np.abs(np.outer(a, b))) / 2 + (np.abs(A) * v[None, :]) @ np.abs(A)
    return np.array([float(np.sum(Gabs * np.abs(dS))) for dS in _dS(X, alpha, ell, sigma, dtype)])


def loo_identity(X, y, alpha, ell, sigma, jitter, dtype=np.longdouble):
    """d loo / d theta by the device's identity, sum_kl G_kl dS_kl, in `dtype`."""
    _, A, a = _inverse(X, y, alpha, ell, sigma, jitter, dtype)
    G, _, _ = _identity_G(A, a, np.diag(A).copy())
    return np.array([np.sum(G * dS) for dS in _dS(X, alpha, ell, sigma, dtype)], dtype=dtype)


def loo_float64(X, y, alpha, ell, sigma, jitter):
    """The device's algebra in float64 (LAPACK): the points from A and a, the gradient by the identity.  Sizes the bounds."""
    yv = np.asarray(y, float)
    _, A, a = _inverse(X, y, alpha, ell, sigma, jitter, float)
    d, out = _points(yv, A, a, float)
    G, _, _ = _identity_G(A, a, d)
    out["grad"] = np.array([np.sum(G * dS) for dS in _dS(X, alpha, ell, sigma, float)])
    return out


def loo_value(X, y, alpha, ell, sigma, jitter, dtype=np.longdouble):
    """loo alone (for central differences)."""
    return loo_reference(X, y, alpha, ell, sigma, jitter, dtype, want_grad=False)["loo"]


def delete_one(X, y, alpha, ell, sigma, jitter, i, dtype=np.longdouble):
    """(mean, variance of the observation) of y_i predicted from the other n - 1 points, by factoring the matrix without row and
    column i: no leave-one-out formula."""
    X = np.asarray(X, float).reshape(len(X), -1)
    n = X.shape[0]
    sg = dtype(sigma)
    S, _, _ = vr.se_cov(X, alpha, ell, sg * sg + dtype(jitter), dtype=dtype)
    keep = np.array([k for k in range(n) if k != i], dtype=int)
    if keep.size == 0:
        return dtype(0), S[i, i]
    L = vr._chol_ld(S[np.ix_(keep, keep)])
    t = vr._fwd_solve_ld(L, S[keep, i])
    z = vr._fwd_solve_ld(L, np.asarray(y, float).astype(dtype)[keep])
    return t @ z, S[i, i] - t @ t


@functools.lru_cache(maxsize=None)
def parity_reference(case):
    """(inputs, long-double reference dict, cond_2(S)) of one entry of CASES, computed once per process."""
    inp = lg.case_inputs(*case)
    return inp, loo_reference(*inp), lg.cond2(inp[0], inp[2], inp[3], inp[4], inp[5])


@functools.lru_cache(maxsize=None)
def delete_reference(case):
    """(inputs, long-double reference dict without gradient, cond_2(S)) of one entry of DELETE_CASES."""
    inp = lg.case_inputs(*case)
    return inp, loo_reference(*inp, want_grad=False), lg.cond2(inp[0], inp[2], inp[3], inp[4], inp[5])


def bounds(ref, cond, scale=1.0):
    """Bounds on |x - ref| for x in mu (n,), var (n,), lpd (n,), loo, grad (per theta; absent when the reference has none), all
    times `scale` (1: against the reference; 2: two float64 evaluations against each other)."""
    ce = BOUND_C * cond * EPS
    var = np.asarray(ref["var"], float)
    r = ref["y"] - np.asarray(ref["mu"], float)
    bmu = ce * (np.abs(ref["y"]) + ref["amax"] * var)
    blpd = ce / 2 + np.abs(r) * bmu / var + r * r / (2 * var) * ce + LPD_FLOOR_C * EPS
    out = {"mu": scale * bmu, "var": scale * ce * var, "lpd": scale * blpd, "loo": scale * float(blpd.sum())}
    if "grad" in ref:
        out["grad"] = scale * (ce * float(np.max(np.abs(ref["grad"]))) + 32.0 * EPS * ref["gabs"])
    return out


def errors(got, ref):
    """|x - ref| of a float64 result (a dict with the keys of loo_reference or of Context.logml_loo) against the long-double one."""
    out = {k: np.abs(np.asarray(got[k], np.longdouble) - ref[k]).astype(float) for k in ("mu", "var", "lpd")}
    out["loo"] = abs(float(np.longdouble(got["loo"]) - ref["loo"]))
    if "grad" in ref and got.get("grad") is not None:
        out["grad"] = np.abs(np.asarray(got["grad"], np.longdouble) - ref["grad"]).astype(float)
    return out


def ratios(got, ref, cond, scale=1.0):
    """Worst error / bound per quantity (a bound of zero admits an error of zero only)."""
    e, b = errors(got, ref), bounds(ref, cond, scale)
    out = {}
    for k, ev in e.items():
        ev, bv = np.atleast_1d(ev), np.atleast_1d(b[k])
        out[k] = float(np.max(np.where(bv > 0, ev / np.where(bv > 0, bv, 1.0), np.where(ev == 0, 0.0, np.inf))))
    return out


if __name__ == "__main__":   # the figures of the module docstring
    worst = {}
    for case in CASES:
        inp, ref, cond = parity_reference(case)
        r = ratios(loo_float64(*inp), ref, cond)
        print(lg.case_id(case), "cond %.1e" % cond, " ".join("%s %.3f" % kv for kv in r.items()))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst", worst)
