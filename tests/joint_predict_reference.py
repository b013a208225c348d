"""CPU reference for gpmi_joint_predict: the posterior of f, f', f'' at new times ts given stacked observations yy = [y; y'] under
the joint matrix of R/ode_gp_library.R:29-30.  A dense numpy restatement in float64 (LAPACK) and in np.longdouble (factorisation
and inverse by the plain loops of joint_grad_reference).  Helper of tests/test_joint_predict_reference.py and
tests/test_gpu_joint_predict.py (not collected: no test_ prefix).

With r = x - y, e = alpha^2 exp(-r^2 / (2 l^2)), u = r^2 / l^2 and the kind letters Q, R, T for the derivative orders 0, 1, 2 of the
first and of the second argument (derivative_kernels.R:39-73):
  QQ = e,  QR = e r / l^2,  RQ = -QR,  RR = e (1 - u) / l^2,  QT = TQ = e (u - 1) / l^2,
  RT = e r (3 - u) / l^4,  TR = -RT,  TT = e (3 - 6 u + u^2) / l^4,
  S = joint_grad_reference.joint_parts (gpmi_joint_logml's matrix),  Ks block a = [kind(a, Q)(ts, t), kind(a, R)(ts, t)],
  Kss block (a, b) = kind(a, b)(ts, ts),  mean = Ks S^-1 yy,  C = Kss - Ks S^-1 Ks^T + diag(post_jitter[a] on block a),
every output stacked by requested order, m rows per block.

The cases are joint_grad_reference.PARITY_CASES with its inputs, alpha, sigma and jitter; m = MS[i] new times
default_rng(77 + n).uniform(-1.1, 1.1, m); post_jitter[a] = 1e-6 alpha^2 / l^(2a).

Tolerances of the GPU tests.  e_mean = max over order blocks of max|mean64 - meanLD| / max|meanLD|, e_cov = max over blocks (a, b) of
max|C64 - CLD| / (alpha^2 / l^(a + b)); rho = e / (eps cond_2(S)).  The GPU differs from the float64 reference in summation order
and a few ulp of exp, inside the same eps cond bound, so its tolerances are C_mean eps cond_2(S) and C_cov eps cond_2(S) with
C = MARGIN = 32 times the largest rho over every case and every order set of ORDER_SETS -- computed here from the two
references, never from the library.  Measured (x86-64 long double, numpy's LAPACK):
  rho_mean: 1.060 at n = 1 (orders 7 and 5; 0.204 for orders 2), 0.006 / 0.016 / 0.048 / 0.047 / 0.796 / 0.672 at
            n = 7 / 21 / 64 / 65 / 129 / 350 (the largest of the three order sets);
  rho_cov:  0.768 at n = 1 (orders 7 and 5; 0.047 for orders 2), at most 0.005 at every n >= 7;
  so C_mean = 33.9 and C_cov = 24.6 (tests/test_joint_predict_reference.py prints the figures of the machine it runs on).
"""
import functools

import numpy as np

import joint_grad_reference as jg

LD = np.longdouble
EPS = jg.EPS
MS = (1, 5, 41, 30, 43, 86, 100)      # new times per entry of jg.PARITY_CASES
ORDER_SETS = (7, 2, 5)                # bit masks: (f, f', f''), (f'), (f, f'')
MARGIN = 32
POST_REL = 1e-6


def orders_of(mask):
    return tuple(a for a in range(3) if (mask >> a) & 1)


def case_m(case):
    return MS[jg.PARITY_CASES.index(case)]


def inputs(case):
    """(t, yy, ts) of one entry of jg.PARITY_CASES."""
    n, _ = case
    t, yy = jg.case_inputs(n)
    ts = np.random.default_rng(77 + n).uniform(-1.1, 1.1, case_m(case))
    return t, yy, ts


def post_jitter(l, mask, alpha=jg.PARITY_ALPHA):
    return np.array([POST_REL * alpha * alpha / l ** (2 * a) for a in orders_of(mask)])


def scales(l, mask, m, alpha=jg.PARITY_ALPHA):
    """s_i = alpha / l^a of every output row: |C_ij| is measured in units of s_i s_j."""
    return np.repeat([alpha / l ** a for a in orders_of(mask)], m)


def blocks(x, y, alpha, l, dtype=float):
    """k[a][b] = alpha^2 kind(a, b)(x, y) = d^a/dx^a d^b/dy^b of alpha^2 exp(-(x - y)^2 / (2 l^2)), a, b in 0..2."""
    x = np.asarray(x, float).astype(dtype)
    y = np.asarray(y, float).astype(dtype)
    a2, l2 = dtype(alpha) * dtype(alpha), dtype(l) * dtype(l)
    r = x[:, None] - y[None, :]
    u = r * r / l2
    e = a2 * np.exp(-(r * r / (2 * l2)))
    qr = e * r / l2
    qt = e * (u - 1) / l2
    rt = e * r * (3 - u) / (l2 * l2)
    return [[e, qr, qt], [-qr, e * (1 - u) / l2, rt], [qt, -rt, e * (3 - 6 * u + u * u) / (l2 * l2)]]


def prior(t, ts, alpha, l, mask, dtype=float):
    """(Ks (p m x 2n), Kss (p m x p m)) for the orders of `mask`."""
    od = orders_of(mask)
    kx, ks = blocks(ts, t, alpha, l, dtype), blocks(ts, ts, alpha, l, dtype)
    return np.block([[kx[a][0], kx[a][1]] for a in od]), np.block([[ks[a][b] for b in od] for a in od])


def posterior(t, yy, alpha, l, sigma, jitter, ts, mask, pj, dtype=float, Linv=None):
    """(mean, C) in `dtype`.  Linv: the inverse factor of S when the caller has it (long double: loops)."""
    S, _ = jg.joint_parts(t, alpha, l, sigma, jitter, dtype)
    Ks, Kss = prior(t, ts, alpha, l, mask, dtype)
    y = np.asarray(yy, float).astype(dtype)
    if dtype is float:
        L = np.linalg.cholesky(S)
        T, z = np.linalg.solve(L, Ks.T), np.linalg.solve(L, y)
    else:
        if Linv is None:
            Linv = jg._lower_inverse_loops(jg._chol_loops(S))
        T, z = Linv @ Ks.T, Linv @ y
    m = np.asarray(ts).size
    return T.T @ z, Kss - T.T @ T + np.diag(np.repeat(np.asarray(pj, float).astype(dtype), m))


@functools.lru_cache(maxsize=None)
def _case_factor(case):
    """(cond_2(S), long-double inverse factor of S) of one case, once per process."""
    n, l = case
    t, _ = jg.case_inputs(n)
    S, _ = jg.joint_parts(t, jg.PARITY_ALPHA, l, jg.PARITY_SIGMA, jg.PARITY_JITTER, LD)
    return jg.cond2(S), jg._lower_inverse_loops(jg._chol_loops(S))


def case_cond(case):
    return _case_factor(case)[0]


@functools.lru_cache(maxsize=None)
def reference(case, mask, longdouble=True):
    """(mean, C) of a case and an order mask; shared by every test of a process and never modified."""
    _, l = case
    t, yy, ts = inputs(case)
    out = posterior(t, yy, jg.PARITY_ALPHA, l, jg.PARITY_SIGMA, jg.PARITY_JITTER, ts, mask, post_jitter(l, mask),
                    LD if longdouble else float, _case_factor(case)[1] if longdouble else None)
    for a in out:
        a.setflags(write=False)
    return out


def mean_error(got, want, m):
    """max over order blocks of max|got - want| / max|want| (want: long double)."""
    d = np.abs((np.asarray(got).astype(LD) - want).astype(float)).reshape(-1, m)
    return float(np.max(d.max(axis=1) / np.abs(want.astype(float)).reshape(-1, m).max(axis=1)))


def cov_error(got, want, s):
    """max|got - want| / (s_i s_j) (want: long double)."""
    return float(np.max(np.abs((np.asarray(got).astype(LD) - want).astype(float)) / np.outer(s, s)))


@functools.lru_cache(maxsize=None)
def rho(case, mask):
    """(rho_mean, rho_cov): the float64 reference's own error against the long-double one, in units of eps cond_2(S)."""
    _, l = case
    m = case_m(case)
    m64, c64 = reference(case, mask, False)
    mld, cld = reference(case, mask, True)
    scale = EPS * case_cond(case)
    return mean_error(m64, mld, m) / scale, cov_error(c64, cld, scales(l, mask, m)) / scale


@functools.lru_cache(maxsize=None)
def constants():
    """(C_mean, C_cov) = MARGIN x the largest rho over every case and order set."""
    r = [rho(case, mask) for case in jg.PARITY_CASES for mask in ORDER_SETS]
    return MARGIN * max(x[0] for x in r), MARGIN * max(x[1] for x in r)


def tolerances(case):
    """(mean, cov) tolerances of the GPU parity tests for one case."""
    cm, cc = constants()
    return cm * EPS * case_cond(case), cc * EPS * case_cond(case)
