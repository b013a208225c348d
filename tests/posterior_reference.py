"""CPU reference of the derivative-observation posteriors -- gpmi_deriv_cov / gpmi_deriv_elem, gpmi_gp_condition,
gpmi_sample_derivs[_batch] and the sampler gpmi_seq_create / _step / _commit -- written from the formulas of include/gpmi.h in
float64 (LAPACK Cholesky, triangular solves) and in np.longdouble (plain loops: predict_reference.cholesky_rows / solve_lower).
Inputs are float64 and are widened exactly, so every rounding of the arguments belongs to the code under test.  Helper of
tests/test_posterior_reference.py and tests/test_gpu_posterior_parity.py (not collected: no test_ prefix).

Kernels (1-D, r = x - y, e = exp(-arg), arg = r^2 / (2 l^2), the row argument first; Q value, R first, T second derivative):
  QQ = e                         QR = d/dy   = e r / l^2                  RQ(x, y) = QR(y, x)
  RR = d2/dxdy = e / l^2 - e r^2 / l^4        QT = d2/dy2 = -e / l^2 + e r^2 / l^4             TQ(x, y) = QT(y, x)
  RT = d3/dxdy2 = 3 e r / l^4 - e r^3 / l^6   TT = 3 e / l^4 - 6 e r^2 / l^6 + e r^4 / l^8     TR(x, y) = RT(y, x)
all times alpha^2; GPMI_COMPAT_RR: alpha^2 multiplies the first term of RR only.
  condition:      K + s2 I = L L^T, T = L^-1 Ks^T, z = L^-1 y, mn = T^T z, Kn = Kss - T^T T + jitter I;
  sample_derivs:  (mu, cov) = condition with (QQ, RQ, RR), alpha = a, s2 = sy^2;  draw = mu + chol(cov) z;
  sampler:        K~ = K_XX + jitter I = L L^T, m = K_sX K~^-1 mn, K* = K_ss - K_sX (K~^-1 - K~^-1 Kn K~^-1) K_Xs + jitter I = Ls Ls^T,
                  w = Ls^-1 (commits - m), condMean_i = m_i + l_i . w, condVar_i = K*_ii - l_i . l_i (l_i: row i of Ls left of the
                  diagonal; row i depends on the leading block only).

Bounds (u = eps / 2, eps = 2^-52; "cond" is cond_2 in float64; the factor 10 is the project's: tests/test_gpu_joint_grad.py,
logml_grad_reference.bounds).  They are what a backward-stable float64 evaluation delivers, never what the device delivers.
  kernel entry:  |K - ref| <= C_K u (1 + arg) absterms + floor.  absterms is the sum of the absolute values of the polynomial
                 terms times e (the terms of RR, QT, RT, TT cancel, each carrying its own relative rounding); an error of the
                 float64 argument of exp is a relative error arg u of the exponential (as in se_cov_reference.py), hence 1 + arg.
                 floor = C_F 2^-1074 (1 + absterms / e): where e is subnormal or underflows its absolute error is one subnormal
                 spacing, multiplied by the polynomial (closed form in arg and l: poly_abs), and so is the rounding of the product.
  Kn[j, k]:      10 cond eps max|Kss| + C_S eps (|Kss_jk| + sum_i |T_ij T_ik|): the factorisation's backward error, plus the
                 rounding of the entry's own sum.
  mn:            10 cond eps max|mn|.
  draw:          10 cond(cov) eps max|chol(cov) z| + the bound on mu: what the device is held to.  This one the float64 routes
                 meet, but not by half: they use up to 0.58 of it (n = m = 199).  The 10 takes a cov that is rounded at its own
                 size; cov = Kss - T^T T is rounded at the size of its two terms, g = max(|Kss| + |T|^T |T|) / max|cov|, about 25,
                 times its own, and chol(cov) z feels that with cond(cov): split by routes, all of the float64 error of a draw
                 comes from the 3e-15 by which cov is off, none from its factorisation.  The CPU tests therefore hold the float64
                 routes to the bound itself and to half of (10 + C_D g) cond(cov) eps max|chol(cov) z| + the bound on mu; the
                 device gets the narrower of the two, the first.
  sampler:       condMean: 10 (cond(K~) + cond(K*)) eps max(|m|, |commits|);  condVar: 10 (cond(K~) + cond(K*)) eps max|K*|.
Where the reference itself underflows (|ref| < 2^-1022) the GPU test asks for an exact zero or a subnormal and nothing else.
Each constant is the smallest power of two for which the float64 route of this module stays within HALF of the bound on every
parity input, measured on the CPU against the long-double route, never against the device
(tests/test_posterior_reference.py asserts the half, and that half the constant does not do):
  C_K = 16:   worst float64 kernel entry 0.275 of the bound (RT, TR at l = 0.05; C_K = 8 leaves 0.550);
  C_F = 1:    worst 0.475 (RR at l = 0.05, e a subnormal of 28 spacings; C_F = 1/2: 0.950);
  C_D = 1/8:  worst draw 0.455 of the CPU bound over three float64 orders of the sums -- LAPACK (0.451), condition_schur (right-looking
              elimination of the joint matrix: 0.278), orc.cholesky(blocked=True) for both factors (0.455); C_D = 1/16: 0.508;
  C_S = 1:    one rounding per term of the entry's own sum.  No parity input needs it: the worst Kn entry is 0.055 of the bound
              at n = 1 and below 0.002 from n = 2 on, where 10 cond eps max|Kss| dominates; mn uses 0.036 of its bound at the most
              (three routes), the sampler's condMean 0.001 and condVar 0.001 of theirs.
Conditions on the parity inputs (asserted, not measured): every cond_2 <= COND_MAX = 2e7 (K + s2 I: 1.6e2 .. 6.2e3; cov: up to
3.9e6; K~ 2.5e6, K* 1.6e6 at the most) and every bound on a diagonal entry of Kn / cov / K* <= jitter / 8 (at most 0.075 jitter).
"""
import functools

import numpy as np

import predict_reference as pr

LD = np.longdouble
EPS = float(np.finfo(float).eps)
U = EPS / 2
SUBNORMAL = 2.0 ** -1074
TINY = float(np.finfo(float).tiny)
COND_MAX = 2e7          # a condition on the parity inputs (tests/test_posterior_reference.py), not a measurement
C_K, C_F, C_S, C_D = 16.0, 1.0, 1.0, 0.125   # see the module docstring

KINDS = ("QQ", "QR", "RQ", "RR", "QT", "TQ", "RT", "TR", "TT")
SWAPPED = {"RQ": "QR", "TQ": "QT", "TR": "RT"}
# (observed, target) in {Q, R, T}: K = kind(oo), Ks = kind(to) (rows: targets), Kss = kind(tt); the last one with GPMI_COMPAT_RR
TRIPLES = (("QQ", "QQ", "QQ", False), ("QQ", "RQ", "RR", False), ("QQ", "TQ", "TT", False),
           ("RR", "QR", "QQ", False), ("RR", "RR", "RR", False), ("RR", "TR", "TT", False),
           ("TT", "QT", "QQ", False), ("TT", "RT", "RR", False), ("TT", "TT", "TT", False),
           ("QQ", "RQ", "RR", True))
ONE_LAUNCH_SIZES = ((1, 1), (2, 1), (21, 30), (64, 65), (100, 79))      # n + m + 1 <= 180
NEXT_ROUTE_SIZE = (100, 80)                                            # 181 rows: past the default small_gc
BIG_LAUNCH_SIZE = (40, 300)                                            # one launch at small_gc = 1024, m > 256
CHAIN_SIZES = ((127, 130), (129, 127), (199, 150), (120, 260), (257, 130), (385, 257))
SD_SIZES = ((25, 25, 3), (129, 127, 5), (199, 199, 4), (100, 300, 3))  # (n, m, B)
SD_JITTER = 1e-6
SEQ_CASES = ((65, 1, 260), (300, 3, 260))                              # (n, D, steps)
SEQ_JITTER = 1e-6
SEQ_DENSITY = 0.9       # data points per unit volume at D > 1 (length-scales 0.8 .. 1.2)
SEQ_SKIP = 130          # an uncommitted step is made in front of this one


def _cases():
    sizes = ONE_LAUNCH_SIZES + (NEXT_ROUTE_SIZE, BIG_LAUNCH_SIZE) + CHAIN_SIZES
    # 13 sizes over 10 triples: every triple at least once on each side of the one-launch / chain divide
    return tuple((n, m, (3 * i + 1) % 10) for i, (n, m) in enumerate(sizes))


COND_CASES = _cases()   # (n, m, index into TRIPLES)


def case_id(case):
    n, m, k = case
    kk, ks, kss, compat = TRIPLES[k]
    return "n%d-m%d-%s-%s-%s%s" % (n, m, kk, ks, kss, "-compat" if compat else "")


def cond_case(n, m):
    return next(c for c in COND_CASES if c[:2] == (n, m))


# ---- kernels ---------------------------------------------------------------------------------------------------------------
def _terms(kind, r, l2, tt_mid):
    one = np.ones_like(r)
    if kind == "QQ":
        return [one]
    if kind == "QR":
        return [r / l2]
    if kind == "RR":
        return [one / l2, -(r * r) / (l2 * l2)]
    if kind == "QT":
        return [-one / l2, (r * r) / (l2 * l2)]
    if kind == "RT":
        return [3 * r / (l2 * l2), -(r * r * r) / (l2 * l2 * l2)]
    if kind == "TT":
        return [3 * one / (l2 * l2), -tt_mid * (r * r) / (l2 * l2 * l2), (r * r * r * r) / (l2 * l2 * l2 * l2)]
    raise ValueError(kind)


def deriv_cov(kind, x, y, alpha, l, compat=False, dtype=float, tt_mid=6):
    """(K, absterms, arg): alpha^2 kind(x_i, y_j; l) in `dtype`; absterms (float) the sum of the absolute polynomial terms times
    e; arg (float) = r^2 / (2 l^2).  tt_mid: TT's middle coefficient (6; the mutation check passes 3)."""
    x = np.asarray(x, float).ravel().astype(dtype)
    y = np.asarray(y, float).ravel().astype(dtype)
    if kind in SWAPPED:         # the transposed forms: kind(x, y) = base(y, x)
        r = y[None, :] - x[:, None]
        kind = SWAPPED[kind]
    else:
        r = x[:, None] - y[None, :]
    l2 = dtype(l) * dtype(l)
    a2 = dtype(alpha) * dtype(alpha)
    arg = (r * r) / (2 * l2)
    e = np.exp(-arg)
    terms = _terms(kind, r, l2, tt_mid)
    if compat and kind == "RR":
        terms[0] = a2 * terms[0]
    else:
        terms = [a2 * t for t in terms]
    s, sa = terms[0], np.abs(terms[0])
    for t in terms[1:]:
        s, sa = s + t, sa + np.abs(t)
    return e * s, (e * sa).astype(float), arg.astype(float)


def poly_abs(kind, arg, alpha, l, compat=False):
    """absterms / e in closed form (float64; for the floor, where e underflows): with s = sqrt(2 arg) = |r| / l."""
    s = np.sqrt(2.0 * np.asarray(arg, float))
    a2, li = float(alpha) ** 2, 1.0 / float(l)
    kind = SWAPPED.get(kind, kind)
    if compat and kind == "RR":
        return (a2 + s * s) * li ** 2
    p = {"QQ": 1.0 + 0 * s, "QR": s * li, "RR": (1 + s * s) * li ** 2, "QT": (1 + s * s) * li ** 2,
         "RT": (3 * s + s ** 3) * li ** 3, "TT": (3 + 6 * s * s + s ** 4) * li ** 4}[kind]
    return a2 * p


def kernel_bound(kind, absterms, arg, alpha, l, compat=False, c_k=C_K, c_f=C_F):
    return c_k * U * (1.0 + arg) * absterms + SUBNORMAL * (c_f * (1.0 + poly_abs(kind, arg, alpha, l, compat)))


# ---- conditioning ----------------------------------------------------------------------------------------------------------
def _chol(A, dtype):
    return np.linalg.cholesky(A) if dtype is float else pr.cholesky_rows(A)


def _solve(L, B, dtype):
    if dtype is float:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, B, lower=True)
    return pr.solve_lower(L, B)


def condition_parts(t, ts, y, alpha, l, s2, jitter, kinds, compat=False, dtype=float, tt_mid=6, chol=None):
    """Everything of one conditioning as a dict: mn, Kn, Kss, T (n x m), sabs = |T|^T |T| (float).  chol: another float64
    Cholesky routine (the second summation order)."""
    n, m = np.size(t), np.size(ts)
    K = deriv_cov(kinds[0], t, t, alpha, l, compat, dtype, tt_mid)[0] + dtype(s2) * np.eye(n, dtype=dtype)
    Ks = deriv_cov(kinds[1], ts, t, alpha, l, compat, dtype, tt_mid)[0]
    Kss = deriv_cov(kinds[2], ts, ts, alpha, l, compat, dtype, tt_mid)[0]
    L = chol(K) if chol is not None else _chol(K, dtype)
    T = _solve(L, Ks.T, dtype)
    z = _solve(L, np.asarray(y, float).astype(dtype), dtype)
    Kn = Kss - T.T @ T + dtype(jitter) * np.eye(m, dtype=dtype)
    Ta = np.abs(T).astype(float)
    return {"mn": T.T @ z, "Kn": Kn, "Kss": Kss, "T": T, "sabs": Ta.T @ Ta}


def condition(t, ts, y, alpha, l, s2, jitter, kinds, compat=False, dtype=float, tt_mid=6):
    """(mn, Kn) of gpmi_gp_condition through one Cholesky of K + s2 I."""
    p = condition_parts(t, ts, y, alpha, l, s2, jitter, kinds, compat, dtype, tt_mid)
    return p["mn"], p["Kn"]


def condition_schur(t, ts, y, alpha, l, s2, jitter, kinds, compat=False, dtype=float):
    """(mn, Kn) by another order of the sums: right-looking elimination of the first n columns of the joint matrix
    [[K + s2 I, Ks^T, y], [Ks, Kss, 0], [y^T, 0, 0]] -- Kn is the trailing block + jitter I, mn minus the last row."""
    n, m = np.size(t), np.size(ts)
    A = np.zeros((n + m + 1, n + m + 1), dtype=dtype)
    A[:n, :n] = deriv_cov(kinds[0], t, t, alpha, l, compat, dtype)[0] + dtype(s2) * np.eye(n, dtype=dtype)
    A[n:n + m, :n] = deriv_cov(kinds[1], ts, t, alpha, l, compat, dtype)[0]
    A[n:n + m, n:n + m] = deriv_cov(kinds[2], ts, ts, alpha, l, compat, dtype)[0]
    A[-1, :n] = np.asarray(y, float).astype(dtype)
    A[:n, n:] = A[n:, :n].T
    for j in range(n):
        d = np.sqrt(A[j, j])
        c = A[j + 1:, j] / d
        A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.outer(c, c)
    return -A[-1, n:n + m], A[n:n + m, n:n + m] + dtype(jitter) * np.eye(m, dtype=dtype)


def sample_derivs(t, ts, y, l, a, sy, jitter, z, dtype=float, schur=False):
    """(mu, cov, draw) of gpmi_sample_derivs: the (QQ, RQ, RR) moments with alpha = a, s2 = sy^2; draw = mu + chol(cov) z.
    schur: the moments by condition_schur (the second order of the sums)."""
    mu, cov = (condition_schur if schur else condition)(t, ts, y, a, l, dtype(sy) * dtype(sy), jitter, ("QQ", "RQ", "RR"), False, dtype)
    return mu, cov, mu + _chol(cov, dtype) @ np.asarray(z, float).astype(dtype)


# ---- the sampler -----------------------------------------------------------------------------------------------------------
def seq_setup(X, mn, Kn, alpha, ell, jitter, pts, dtype=float):
    """(m, K*, Ls, K~): the joint law of all star points and its factor."""
    X = np.asarray(X, float).reshape(len(X), -1)
    P = np.asarray(pts, float).reshape(len(pts), -1)
    n, s = X.shape[0], P.shape[0]
    Kt = pr.se_cov(X, X, alpha, ell, dtype) + dtype(jitter) * np.eye(n, dtype=dtype)
    L = _chol(Kt, dtype)
    T = _solve(L, pr.se_cov(X, P, alpha, ell, dtype), dtype)                    # n x s: L^-1 K_Xs
    b = _solve(L, np.asarray(mn, float).astype(dtype), dtype)
    G = _solve(L, _solve(L, np.asarray(Kn, float).astype(dtype), dtype).T, dtype)   # L^-1 Kn L^-T
    G = (G + G.T) / 2
    Ks = pr.se_cov(P, P, alpha, ell, dtype) - T.T @ T + T.T @ (G @ T) + dtype(jitter) * np.eye(s, dtype=dtype)
    Ks = (Ks + Ks.T) / 2
    return T.T @ b, Ks, _chol(Ks, dtype), Kt


def _chain(m, Ks, Ls, z=None, commits=None, w_from_var=False):
    s = len(m)
    dt = Ls.dtype.type
    w = np.zeros(s, dtype=Ls.dtype)
    out = np.zeros((s, 2), dtype=Ls.dtype)
    com = np.zeros(s)
    for i in range(s):
        li = Ls[i, :i]
        out[i] = m[i] + li @ w[:i], Ks[i, i] - li @ li
        com[i] = float(out[i, 0] + np.sqrt(out[i, 1]) * dt(z[i])) if commits is None else commits[i]
        w[i] = (dt(com[i]) - out[i, 0]) / (out[i, 1] if w_from_var else np.sqrt(out[i, 1]))
    return out, com


def seq_chain(X, mn, Kn, alpha, ell, jitter, pts, commits, dtype=float, w_from_var=False):
    """(steps, 2): (condMean_i, condVar_i) given the first i entries of `commits`, the values committed to the sampler.
    w_from_var: the mutation check's w_i = (commit_i - condMean_i) / condVar_i."""
    m, Ks, Ls, _ = seq_setup(X, mn, Kn, alpha, ell, jitter, pts, dtype)
    return _chain(m, Ks, Ls, commits=np.asarray(commits, float), w_from_var=w_from_var)[0]


def seq_commits(X, mn, Kn, alpha, ell, jitter, pts, z, dtype=LD):
    """The chain that draws as it goes: commits_i = float64(condMean_i + sqrt(condVar_i) z_i).  Returns (out, commits)."""
    m, Ks, Ls, _ = seq_setup(X, mn, Kn, alpha, ell, jitter, pts, dtype)
    return _chain(m, Ks, Ls, z=np.asarray(z, float))


# ---- conditions, bounds, errors --------------------------------------------------------------------------------------------
def cond2(A):
    """cond_2 of a symmetric positive definite matrix, in float64."""
    ev = np.linalg.eigvalsh(np.asarray(A, float))
    return float(ev[-1] / ev[0])


def condition_bounds(parts, cond, scale=1.0):
    """(bound on |mn - ref| (scalar), bound on |Kn - ref| per entry) from the long-double parts of one conditioning."""
    kss = np.abs(parts["Kss"]).astype(float)
    ce = 10.0 * cond * EPS
    return (scale * ce * float(np.max(np.abs(parts["mn"]))),
            scale * (ce * float(np.max(kss)) + C_S * EPS * (kss + parts["sabs"])))


def draw_bound(mu_bound, cond_cov, parts, draw, scale=1.0, c_d=0.0):
    """Bound on |draw - ref|: (10 + c_d max(|Kss| + |T|^T |T|) / max|cov|) cond(cov) eps max|chol(cov) z| + the bound on mu
    (already scaled).  c_d = 0: the bound of the device; c_d = C_D: the one the float64 routes keep half of."""
    grow = float(np.max(np.abs(parts["Kss"]).astype(float) + parts["sabs"]) / np.max(np.abs(parts["Kn"])))
    return scale * (10.0 + c_d * grow) * cond_cov * EPS * float(np.max(np.abs(draw - parts["mn"]))) + mu_bound


def seq_bounds(ref, commits, m, Ks, Kt, scale=1.0):
    """(bound on condMean, bound on condVar, cond(K~), cond(K*))."""
    ct, cs = cond2(Kt), cond2(Ks)
    ce = 10.0 * (ct + cs) * EPS
    mag = max(float(np.max(np.abs(m))), float(np.max(np.abs(commits))))
    return scale * ce * mag, scale * ce * float(np.max(np.abs(Ks))), ct, cs


def errors(got, ref):
    """|got - ref| in float64, the difference taken in long double."""
    return np.abs(np.asarray(got, LD) - np.asarray(ref, LD)).astype(float)


def ratios(got, ref, bound):
    """|got - ref| / bound per entry, formed in long double (an error below 2^-1074 does not round to zero first)."""
    e = np.abs(np.asarray(got, LD) - np.asarray(ref, LD))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e == 0, LD(0), e / np.asarray(bound, LD)).astype(float)


# ---- the parity inputs, deterministic in their arguments -------------------------------------------------------------------
PARITY_ALPHA, PARITY_L = 1.2, 1.0


def kind00(kind, alpha, l, compat=False):
    """alpha^2 kind(0, 0; l): the diagonal entry that the noise and the jitter are scaled by."""
    return float(deriv_cov(kind, [0.0], [0.0], alpha, l, compat)[0][0, 0])


def cond_inputs(n, m, k):
    """(t, ts, y, alpha, l, s2, jitter, kinds, compat): t, ts ~ sorted U(0, n / 10) (about ten points per length-scale),
    y = sin(t) + 0.05 eps, s2 = 0.01 K(0, 0), jitter = 1e-8 Kss(0, 0)."""
    kk, ks, kss, compat = TRIPLES[k]
    rng = np.random.default_rng(1000 * n + m)
    t = np.sort(rng.uniform(0, n / 10.0, n))
    ts = np.sort(rng.uniform(0, n / 10.0, m))
    y = np.sin(t) + 0.05 * rng.standard_normal(n)
    a, l = PARITY_ALPHA, PARITY_L
    return t, ts, y, a, l, 0.01 * kind00(kk, a, l, compat), 1e-8 * kind00(kss, a, l, compat), (kk, ks, kss), compat


@functools.lru_cache(maxsize=None)
def cond_reference(case, longdouble=True):
    """(inputs, parts, cond_2(K + s2 I)) of one COND_CASES entry, once per process."""
    inp = cond_inputs(*case)
    t, ts, y, a, l, s2, jit, kinds, compat = inp
    parts = condition_parts(t, ts, y, a, l, s2, jit, kinds, compat, LD if longdouble else float)
    K = deriv_cov(kinds[0], t, t, a, l, compat)[0] + s2 * np.eye(len(t))
    return inp, parts, cond2(K)


def sd_inputs(n, m, B):
    """(t, ts, Y (n, B), P (B, 3) rows (l, a, sy), Z (m, B), jitter)."""
    rng = np.random.default_rng(7000 + 10 * n + m)
    t = np.sort(rng.uniform(0, n / 10.0, n))
    ts = np.sort(rng.uniform(0, n / 10.0, m))
    P = np.column_stack([0.8 + 0.3 * rng.random(B), 1.0 + 0.4 * rng.random(B), 0.08 + 0.05 * rng.random(B)])
    Y = np.asfortranarray(np.sin(t)[:, None] + 0.1 * rng.standard_normal((n, B)))
    Z = np.asfortranarray(rng.standard_normal((m, B)))
    return t, ts, Y, P, Z, SD_JITTER


@functools.lru_cache(maxsize=None)
def sd_reference(case, b, longdouble=True):
    """Draw b of one SD_SIZES entry: dict mu, cov, draw, mu_bound, draw_bound (the device's), draw_bound_cpu, cond (K + sy^2 I), cond_cov, parts."""
    t, ts, Y, P, Z, jit = sd_inputs(*case)
    dtype = LD if longdouble else float
    l, a, sy = P[b]
    parts = condition_parts(t, ts, Y[:, b], a, l, dtype(sy) * dtype(sy), jit, ("QQ", "RQ", "RR"), False, dtype)
    mu, cov = parts["mn"], parts["Kn"]
    draw = mu + _chol(cov, dtype) @ Z[:, b].astype(dtype)
    K = deriv_cov("QQ", t, t, a, l)[0] + sy * sy * np.eye(len(t))
    cond, cond_cov = cond2(K), cond2(cov)
    mb = 10.0 * cond * EPS * float(np.max(np.abs(mu)))
    return {"mu": mu, "cov": cov, "draw": draw, "cond": cond, "cond_cov": cond_cov, "mu_bound": mb, "parts": parts,
            "draw_bound": draw_bound(mb, cond_cov, parts, draw), "draw_bound_cpu": draw_bound(mb, cond_cov, parts, draw, c_d=C_D)}


def seq_inputs(n, D, steps):
    """(X, mn, Kn, alpha, ell, jitter, pts, z).  X ~ U(0, side)^D with about two points per length-scale volume (D = 1: a
    jittered grid of spacing 0.5); the star points spread over the same range; (mn, Kn) the (QQ, RQ, RR) posterior of sin on n
    points (float64: an input like any other)."""
    rng = np.random.default_rng(300 * n + D)
    if D == 1:
        X = (0.5 * np.arange(n) + rng.uniform(-0.1, 0.1, n)).reshape(-1, 1)
        side = 0.5 * n
        ell = np.array([0.9])
    else:
        side = (n / SEQ_DENSITY) ** (1.0 / D)
        X = rng.uniform(0, side, (n, D))
        ell = 0.8 + 0.4 * rng.random(D)
    pts = rng.uniform(0, side, (steps, D))
    t = np.linspace(0, 0.15 * n, n)
    mn, Kn = condition(t, t, np.sin(t), 1.0, 0.9, 0.01, 0.0, ("QQ", "RQ", "RR"))
    Kn = (Kn + Kn.T) / 2
    return np.asfortranarray(X), mn, np.asfortranarray(Kn), 1.1, ell, SEQ_JITTER, np.asfortranarray(pts), rng.standard_normal(steps)


@functools.lru_cache(maxsize=None)
def seq_reference(case):
    """(inputs, out (steps, 2) long double, commits (float64), bound on condMean, bound on condVar, cond(K~), cond(K*))."""
    inp = seq_inputs(*case)
    X, mn, Kn, a, ell, jit, pts, z = inp
    m, Ks, Ls, Kt = seq_setup(X, mn, Kn, a, ell, jit, pts, LD)
    out, commits = _chain(m, Ks, Ls, z=z)
    return (inp, out, commits) + seq_bounds(out, commits, m, Ks, Kt)


# ---- the kernel inputs -------------------------------------------------------------------------------------------------------
KERNEL_LS = (0.05, 0.6, 30.0)
KERNEL_RECTS = ((1, 1), (17, 257), (131, 70))
KERNEL_ALPHA = 1.3


def kernel_points(n, m, l, seed=0):
    """(x, y): points over a few length-scales, with coincident pairs (y repeats entries of x) and, for n, m > 1, one point of
    each far enough for arg > 745 (40 length-scales: arg = 800) and one pair whose e is subnormal."""
    rng = np.random.default_rng(50 * n + m + seed)
    x = rng.uniform(0, 6 * l, n)
    y = rng.uniform(0, 6 * l, m)
    k = min(n, m, 5)
    y[:k] = x[:k]
    if n > 1:
        x[-1] = 46 * l
    if m > 1:
        y[-1] = -40 * l
    if n > 1 and m > 2:
        y[-2] = x[-1] - 38.5 * l        # arg = 741.1: e = 1.4e-322, a subnormal of 28 spacings
    return x, y
