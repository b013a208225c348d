"""CPU reference for gpmi_logml_hess: the exact Hessian of the log marginal likelihood of models/fit_hyperparameters.stan:18-32 in
theta = (alpha, ell.., sigma), in np.longdouble (plain loops), and the device's algebra in float64 (LAPACK).  Built on
tests/vjp_reference.py (covariance, long-double factorisation), tests/centered_gp_reference.py (the backward substitution, through
tests/loo_reference.py's inverse) and the inputs of tests/logml_grad_reference.py.  Helper of tests/test_hess_reference.py and
tests/test_gpu_hess.py (not collected: no test_ prefix).

With S = alpha^2 K0(X; ell) + (sigma^2 + jitter) I = K + s I, A = S^-1, a = A y, G = (a a' - A) / 2, S_i = dS/dtheta_i,
S_ij = d^2 S/dtheta_i dtheta_j, b_i = S_i a, P_i = A S_i:
  H_ij = <G, S_ij> - b_i' A b_j + 1/2 sum_kl P_i[k,l] P_j[l,k],
  S_alpha = (2 / alpha) K, S_sigma = 2 sigma I, S_ell_d = K o R_d, R_d = r_d^2 / ell_d^3 (one length-scale: sum_d r_d^2 / ell^3),
  S_alpha,alpha = (2 / alpha^2) K, S_alpha,ell_d = (2 / alpha) K o R_d, S_ell_d,ell_e = K o R_d o R_e - [d = e] 3 K o r_d^2 / ell_d^4,
  S_sigma,sigma = 2 I, S_alpha,sigma = S_ell,sigma = 0.
hess_reference states this with ONE explicit product per hyper-parameter, alpha and sigma included.  The device (hess_shortcut,
in float64 hess_float64) multiplies for the length-scales only: P_alpha = (2 / alpha) (I - s A), P_sigma = 2 sigma A, so that
their traces come from tr A, |A|_F^2, tr P_d and tr(A P_d), and b_alpha = (2 / alpha) (y - s a), b_sigma = 2 sigma a.  The
reference never uses these.

Bound, in the form of tests/logml_grad_reference.py, for a float64 evaluation against the long-double one:
  |H_ij - ref| <= C cond eps hmax + 32 eps habs_ij,   hmax = max |H|,
habs_ij the same three terms with every factor (a, A, S_i, S_ij) replaced by its absolute value.  C = BOUND_C is the smallest of
10, 16, 32, 64 for which hess_float64 stays within HALF of every bound on every HESS_CASES input, measured on the CPU against
the long-double value, never against the device.  Measured worst error / bound of hess_float64 at C = 10 (print them with
`python tests/hess_reference.py`): 0.120 (CANCEL_CASE, n = 2), then 0.052 (n = 65, D = 1, sigma = 1e-3, cond 3.7e6), 0.030
(n = 2) and 0.027 (the coincident points); n = 257: 0.021, 0.003, 0.000; n = 385: 0.001, 0.004, 0.000 -- so C = 10 stands.
"""
import functools

import numpy as np

import logml_grad_reference as lg
import loo_reference as lr
import vjp_reference as vr

EPS = lg.EPS
BOUND_C = 10.0
MAX_ELL = 8   # length-scales gpmi_logml_hess takes: one, or one per dimension up to D = 8


def n_ell_of(case):
    return case[1] if case[2] else 1


# the chain cases with at most MAX_ELL length-scales: n = 1, 2, 63, 65, 129, 257, 385; D = 1 .. 8 ARD and isotropic, isotropic
# D = 9 .. 64; sigma in (0.15, 1e-3, 0); coincident points; CANCEL_CASE
HESS_CASES = tuple(c for c in lg.CHAIN_CASES if n_ell_of(c) <= MAX_ELL)
# central differences of the gradient: the inputs of the reference's own check, and of the device's (tests/test_gpu_hess.py)
DIFF_CASES = ((7, 1, False, 0.15, ""), (40, 3, True, 0.15, ""), (2, 1, True, 0.0, ""), (17, 2, False, 1e-3, ""))
FD_CASE = (63, 3, True, 0.15, "")
FD_HREL, FD_HMIN = 1e-4, 1e-3


def _derivatives(X, alpha, ell, sigma, dtype):
    """(K, [S_i], [[S_ij]]) for theta = (alpha, ell.., sigma); None stands for a zero matrix."""
    X = np.asarray(X, float).reshape(len(X), -1)
    n, D = X.shape
    m = np.atleast_1d(ell).size
    e = vr._ells(ell, D).astype(dtype)
    K, K0, R2 = vr.se_cov(X, alpha, ell, 0.0, dtype=dtype)
    al, sg = dtype(alpha), dtype(sigma)
    if m == 1:
        r2 = [R2.sum(axis=2)]
        ls = [e[0]]
    else:
        r2 = [R2[:, :, d] for d in range(D)]
        ls = [e[d] for d in range(D)]
    R = [r2[d] / ls[d] ** 3 for d in range(m)]
    eye = np.eye(n, dtype=dtype)
    S1 = [2 * al * K0] + [K * R[d] for d in range(m)] + [2 * sg * eye]
    q = m + 2
    S2 = [[None] * q for _ in range(q)]
    S2[0][0] = 2 * K0
    for d in range(m):
        S2[0][1 + d] = S2[1 + d][0] = 2 * al * K0 * R[d]
        for f in range(m):
            S2[1 + d][1 + f] = K * R[d] * R[f] - (3 * K * r2[d] / ls[d] ** 4 if d == f else 0)
    S2[q - 1][q - 1] = 2 * eye
    return K, S1, S2


def hess_reference(X, y, alpha, ell, sigma, jitter, dtype=np.longdouble):
    """The textbook formula in `dtype`, one product per hyper-parameter.  Returns a dict: hess (q x q), habs (q x q, float), hmax."""
    _, A, a = lr._inverse(X, y, alpha, ell, sigma, jitter, dtype)
    _, S1, S2 = _derivatives(X, alpha, ell, sigma, dtype)
    q = len(S1)
    G = (np.outer(a, a) - A) / 2
    absA, absa = np.abs(A), np.abs(a)
    Gabs = (np.outer(absa, absa) + absA) / 2
    b = [Si @ a for Si in S1]
    c = [A @ bi for bi in b]
    P = [A @ Si for Si in S1]
    babs = [np.abs(Si) @ absa for Si in S1]
    cabs = [absA @ bi for bi in babs]
    Pabs = [absA @ np.abs(Si) for Si in S1]
    H = np.zeros((q, q), dtype=dtype)
    habs = np.zeros((q, q))
    for i in range(q):
        for j in range(q):
            t1 = np.sum(G * S2[i][j]) if S2[i][j] is not None else dtype(0)
            t1a = np.sum(Gabs * np.abs(S2[i][j])) if S2[i][j] is not None else 0.0
            H[i, j] = t1 - b[i] @ c[j] + np.sum(P[i] * P[j].T) / 2
            habs[i, j] = float(t1a + babs[i] @ cabs[j] + np.sum(Pabs[i] * Pabs[j].T) / 2)
    return {"hess": H, "habs": habs, "hmax": float(np.max(np.abs(H)))}


def hess_shortcut(X, y, alpha, ell, sigma, jitter, dtype=float):
    """The device's algebra in `dtype`: products for the length-scales only, the sums assembled as k_hess_finish does."""
    yv = np.asarray(y, float).astype(dtype)
    _, A, a = lr._inverse(X, y, alpha, ell, sigma, jitter, dtype)
    _, S1, S2 = _derivatives(X, alpha, ell, sigma, dtype)
    n, q = len(yv), len(S1)
    m = q - 2
    al, sg = dtype(alpha), dtype(sigma)
    s = sg * sg + dtype(jitter)
    G = (np.outer(a, a) - A) / 2
    b = [(2 / al) * (yv - s * a)] + [S1[1 + d] @ a for d in range(m)] + [2 * sg * a]
    c = [A @ bi for bi in b]
    P = [A @ S1[1 + d] for d in range(m)]
    tA, fA = np.trace(A), np.sum(A * A)
    tP = [np.trace(Pd) for Pd in P]
    AP = [np.sum(A * Pd.T) for Pd in P]
    H = np.zeros((q, q), dtype=dtype)
    for j in range(q):
        for i in range(j + 1):
            t1 = np.sum(G * S2[i][j]) if S2[i][j] is not None else dtype(0)
            if j == 0:
                t3 = (2 / (al * al)) * ((n - 2 * s * tA) + s * s * fA)
            elif j <= m and i == 0:
                t3 = (tP[j - 1] - s * AP[j - 1]) / al
            elif j <= m:
                t3 = np.sum(P[i - 1] * P[j - 1].T) / 2
            elif i == 0:
                t3 = (2 * sg / al) * (tA - s * fA)
            elif i <= m:
                t3 = sg * AP[i - 1]
            else:
                t3 = 2 * sg * sg * fA
            H[i, j] = H[j, i] = (t1 - b[i] @ c[j]) + t3
    return H


def hess_float64(X, y, alpha, ell, sigma, jitter):
    return hess_shortcut(X, y, alpha, ell, sigma, jitter, float)


@functools.lru_cache(maxsize=None)
def parity_reference(case):
    """(inputs, long-double reference dict, cond_2(S)) of one (n, D, ard, sigma, variant), computed once per process."""
    inp = lg.case_inputs(*case)
    return inp, hess_reference(*inp), lg.cond2(inp[0], inp[2], inp[3], inp[4], inp[5])


def bounds(ref, cond, scale=1.0):
    """q x q bounds on |H - ref|, times `scale`."""
    return scale * (BOUND_C * cond * EPS * ref["hmax"] + 32.0 * EPS * ref["habs"])


def errors(H, ref):
    return np.abs(np.asarray(H, np.longdouble) - ref["hess"]).astype(float)


def ratio(H, ref, cond, scale=1.0):
    """Worst error / bound over the entries (a bound of zero admits an error of zero only)."""
    e, b = errors(H, ref), bounds(ref, cond, scale)
    return float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e == 0, 0.0, np.inf))))


def fd_steps(alpha, ell, sigma, hrel=FD_HREL, hmin=FD_HMIN):
    theta = np.concatenate([[alpha], np.atleast_1d(ell), [sigma]]).astype(float)
    return theta, hrel * np.maximum(np.abs(theta), hmin)


def fd_hessian(grad_fun, theta, h, dtype=float):
    """Central differences of a gradient: column k = (grad(theta + h_k e_k) - grad(theta - h_k e_k)) / (2 h_k).  grad_fun(theta)
    returns the gradient; theta and h are float64 (the points are exactly representable in every dtype)."""
    q = theta.size
    F = np.zeros((q, q), dtype=dtype)
    for k in range(q):
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h[k]
        tm[k] -= h[k]
        # the step actually taken, so that no rounding of theta + h enters the quotient
        F[:, k] = (np.asarray(grad_fun(tp), dtype) - np.asarray(grad_fun(tm), dtype)) / dtype(tp[k] - tm[k])
    return F


@functools.lru_cache(maxsize=None)
def fd_reference(case):
    """The stencil of tests/test_gpu_hess.py on `case` in long double: (inputs, theta, h, Hessian reference dict, cond, the
    truncation |FD - H| (q x q), the per-column sum of the two gradient bounds of lg.bounds divided by 2 h_k (q x q))."""
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    theta, h = fd_steps(a, ell, s)
    ref = hess_reference(X, y, a, ell, s, jit)
    cond = lg.cond2(X, a, ell, s, jit)
    q = theta.size
    gb = np.zeros((q, q))
    cols = np.zeros((q, q), dtype=np.longdouble)
    for k in range(q):
        g = []
        for sgn in (1.0, -1.0):
            t = theta.copy()
            t[k] += sgn * h[k]
            r = lg.logml_grad_reference(X, y, t[0], t[1:-1], t[-1], jit, np.longdouble)
            g.append((t[k], r["grad"]))
            gb[:, k] += lg.bounds(r, lg.cond2(X, t[0], t[1:-1], t[-1], jit), case[0])[2]
        step = g[0][0] - g[1][0]
        cols[:, k] = (g[0][1] - g[1][1]) / np.longdouble(step)
        gb[:, k] /= step
    trunc = np.abs(cols - ref["hess"]).astype(float)
    return (X, y, a, ell, s, jit), theta, h, ref, cond, trunc, gb


if __name__ == "__main__":   # the figures of the module docstring
    worst = 0.0
    for case in HESS_CASES:
        inp, ref, cond = parity_reference(case)
        r = ratio(hess_float64(*inp), ref, cond)
        print(lg.case_id(case), "cond %.1e" % cond, "hmax %.3e" % ref["hmax"], "error / bound %.3f" % r, flush=True)
        worst = max(worst, r)
    print("worst", worst)
