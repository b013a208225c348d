"""CPU reference for the Hermite-eigenfunction low-rank GP (gpmi_hermite_basis, gpmi_lowrank_logml_grad,
gpmi_lowrank_latent_lp_grad).  Written from the formulas of include/gpmi.h, section "low-rank (Hermite-eigenfunction) GP".  Helper
of tests/test_lowrank_reference.py and tests/test_gpu_lowrank.py (not collected: no test_ prefix).

Three independent statements of the same quantities:
  * basis_ld: the CLOSED FORM in 50-digit mpmath -- Phi[i, k] = amp sqrt(lambda_k) phi_k(x_i) with mpmath.hermite -- and its
    l-derivative from the closed form's own product rule (dH_k/dt = 2 k H_(k-1)) with the derivatives of the scalars c0(l),
    r(l), delta^2(l), alpha beta(l) taken by mpmath.diff; rounded once to np.longdouble.
  * marginal_dense: y ~ N(0, Phi Phi^T + sigma^2 I) by an n x n long-double Cholesky (plain loops), the gradient by one trace
    per parameter, 1/2 a^T dSigma a - 1/2 tr(Sigma^-1 dSigma) with Sigma^-1 from the n x n factor: not the device's M x M
    identity.  marginal_identity is that identity in any dtype (the device's algebra; float64 = what "sizes the bounds").
    The two inputs too large for an n x n long-double factorisation inside a test (n = 1438, 2049) are recorded in
    tests/golden/lowrank_dense.json by `python tests/lowrank_reference.py --golden`; test_lowrank_reference.py checks the record
    against marginal_identity in long double.
  * latent_ref: q = Phi z and the two heads in long double.

Bounds for a float64 evaluation against these, C = BOUND_C, eps = 2^-52 (bounds()/latent_bounds() state each scale):
  Phi[i, k]:   C eps max(colmax_k, rowrun_ik), colmax_k = max_i |Phi[i, k]| and rowrun_ik = max_{j <= k} |Phi[i, j]|: the
               recurrence carries the rounding of the earlier columns of its row forward; likewise dPhi with its own maxima
               plus those of Phi / l.
  marginal:    with A = sigma^2 I + Phi^T Phi and its componentwise condition, cond = || |A^-1| |A| ||_inf (Skeel):
               out3[2] (Q):   C eps cond y'y / sigma^2
               out3[1] (hld): C eps (|(n - M) log sigma| + sum |log L_kk| + tr(|A^-1| |A|))
               out3[0]:       the two combined plus eps n log(2 pi) / 2
               grad:          C eps cond times the sum of the absolute values of the terms of each formula.
  latent:      q_i: C eps sum_k |Phi_ik z_k| plus the basis bound carried through z; lik, qbar, zbar and grad: the bounds of
               their inputs carried through the formula plus C eps times the sum of the absolute terms.
C is the smallest of 10, 16, 32, 64, ... at which the float64 transcription (basis_f64, marginal_identity, latent_f64) stays
within HALF of every bound on every entry of CASES, measured on the CPU against the references above, never against the device.
`python tests/lowrank_reference.py` prints the worst ratios; C = 16 leaves Phi at 0.53 (M = 128), so C = 32.
"""
import functools
import json
import os

import mpmath as mp
import numpy as np

import centered_gp_reference as cg
import vjp_reference as vr

mp.mp.dps = 50
LD = np.longdouble
EPS = 2.0 ** -52
BOUND_C = 32.0
SCALE = 0.25
AMP = 1.3
SIGMA = 0.35
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowrank_dense.json")

# (n, M, l): x in [-0.5, 0.5], scale 0.25.  Every n and every M of the GPU test appears at least once
CASES = ((1, 1, 1.0), (1, 2, 0.3), (3, 3, 0.3), (3, 2, 1.0), (21, 10, 1.0), (21, 17, 0.3), (64, 16, 0.3), (65, 17, 0.3),
         (65, 128, 0.1), (257, 10, 1.0), (257, 40, 0.3), (64, 1, 1.0), (257, 3, 0.3))
BIG_CASES = ((1438, 10, 1.0), (2049, 3, 0.3))   # dense reference from the golden record


def case_inputs(n, M, l, seed=0):
    """x (sorted, in [-0.5, 0.5]), y, z, Y (n x 2 of 0 / 1) of one case, the same on every call."""
    rng = np.random.default_rng(1000 * n + M + seed)
    x = np.sort(rng.uniform(-0.5, 0.5, n))
    y = np.sin(3.0 * x) + 0.3 * rng.standard_normal(n)
    z = rng.standard_normal(M)
    Y = (rng.uniform(size=(n, 2)) < 0.5).astype(float)
    return x, y, z, Y


# ---- the closed form -----------------------------------------------------------------------------------------------------
def _scalars(scale, l):
    """(c0 / amp, r, delta^2, alpha beta) of the closed form in mpmath."""
    a = 1 / (4 * mp.mpf(scale) ** 2)
    e2 = 1 / (2 * mp.mpf(l) ** 2)
    al2 = 2 * a
    be = (1 + 4 * e2 / al2) ** mp.mpf("0.25")
    d2 = al2 * (be * be - 1) / 2
    Dn = al2 + d2 + e2
    return mp.sqrt(mp.sqrt(al2 / Dn)) * mp.sqrt(be), e2 / Dn, d2, mp.sqrt(al2) * be


def _to_ld(v):
    return LD(mp.nstr(v, 30))


@functools.lru_cache(maxsize=None)
def _basis_ld_cached(xkey, M, scale, amp, l):
    x = [mp.mpf(float(v)) for v in xkey]
    c0, r, d2, ab = _scalars(scale, l)
    dc0, dr, dd2, dab = (mp.diff(lambda t, q=q: _scalars(scale, t)[q], mp.mpf(l)) for q in range(4))
    n = len(x)
    Phi = np.zeros((n, M), LD)
    dPhi = np.zeros((n, M), LD)
    ampm = mp.mpf(amp)
    for i, xi in enumerate(x):
        e = mp.exp(-d2 * xi * xi)
        prev = mp.mpf(0)
        for k in range(M):
            s = mp.sqrt(r ** k / (mp.mpf(2) ** k * mp.factorial(k)))
            v = ampm * c0 * s * e * mp.hermite(k, ab * xi)
            # d/dl: the logarithmic derivative of the prefactor, and 2 k H_(k-1) dt/dl = sqrt(2 k r) x (alpha beta)' Phi_(k-1)
            dv = v * (dc0 / c0 + k * dr / (2 * r) - dd2 * xi * xi) + mp.sqrt(2 * k * r) * xi * dab * prev
            Phi[i, k] = _to_ld(v)
            dPhi[i, k] = _to_ld(dv)
            prev = v
    Phi.setflags(write=False)
    dPhi.setflags(write=False)
    return Phi, dPhi


def basis_ld(x, M, scale, amp, l):
    """(Phi, dPhi/dl), n x M np.longdouble, from the 50-digit closed form; computed once per input."""
    return _basis_ld_cached(tuple(float(v) for v in np.asarray(x, float)), int(M), float(scale), float(amp), float(l))


# ---- the device's algebra in float64 (or any dtype) -------------------------------------------------------------------------
def lr_params(scale, amp, l, dtype=float):
    """The launch scalars of csrc/lowrank_kernels.hip (lr_params), statement by statement."""
    t = dtype
    scale, amp, l = t(scale), t(amp), t(l)
    al2 = 1 / (2 * scale * scale)
    al = np.sqrt(al2)
    ep2 = 1 / (2 * l * l)
    dep2 = -1 / (l * l * l)
    be = np.sqrt(np.sqrt(1 + 4 * ep2 / al2))
    dbe = dep2 / (al2 * be * be * be)
    d2 = 2 * ep2 / (be * be + 1)
    dd2 = al2 * be * dbe
    Dn = al2 + d2 + ep2
    dDn = dd2 + dep2
    r = ep2 / Dn
    dr = (dep2 * Dn - ep2 * dDn) / (Dn * Dn)
    c0 = amp * np.sqrt(np.sqrt(al2 / Dn)) * np.sqrt(be)
    return {"c0": c0, "dc0": c0 * (dbe / be / 2 - dDn / Dn / 4), "d2": d2, "dd2": dd2, "ab": al * be,
            "pl": dbe / be + dr / r / 2, "r": r, "dr": dr}


def basis_f64(x, M, scale, amp, l, dtype=float):
    """(Phi, dPhi/dl) by the three-term recurrence and its forward tangent, in the device's operation order."""
    P = lr_params(scale, amp, l, dtype)
    x = np.asarray(x, float).astype(dtype)
    n = len(x)
    Phi = np.zeros((n, M), dtype)
    dPhi = np.zeros((n, M), dtype)
    x2 = x * x
    e = np.exp(-(P["d2"] * x2))
    v = P["c0"] * e
    dv = P["dc0"] * e - P["dd2"] * x2 * v
    vm = np.zeros(n, dtype)
    dvm = np.zeros(n, dtype)
    Phi[:, 0], dPhi[:, 0] = v, dv
    for k in range(M - 1):
        k1 = dtype(k + 1)
        p = P["ab"] * np.sqrt(2 * P["r"] / k1)
        s = np.sqrt(dtype(k) / k1)
        dp, q, dq = p * P["pl"], P["r"] * s, P["dr"] * s
        xv = x * v
        vn = p * xv - q * vm
        dvn = (dp * xv + p * (x * dv)) - (dq * vm + q * dvm)
        vm, dvm, v, dv = v, dv, vn, dvn
        Phi[:, k + 1], dPhi[:, k + 1] = v, dv
    return Phi, dPhi


def _chol(A, dtype):
    return np.linalg.cholesky(A) if dtype is float else vr._chol_ld(A)


def _linv(L, dtype):
    n = L.shape[0]
    return np.linalg.solve(L, np.eye(n)) if dtype is float else vr._fwd_solve_ld(L, np.eye(n, dtype=dtype))


def marginal_identity(x, y, M, scale, amp, l, sigma, dtype=float, basis=None):
    """out3, grad and the quantities the bounds use, by the M x M identity (the algebra of k_lr_finish) in `dtype`; `basis`
    overrides the (Phi, dPhi) of basis_f64 (the long-double closed form, for the golden record's check)."""
    Phi, dPhi = basis if basis is not None else basis_f64(x, M, scale, amp, l, dtype)
    Phi, dPhi = Phi.astype(dtype), dPhi.astype(dtype)
    yv = np.asarray(y, float).astype(dtype)
    n = len(yv)
    sg, am = dtype(sigma), dtype(amp)
    s2 = sg * sg
    G = Phi.T @ Phi
    S = Phi.T @ dPhi
    S = S + S.T
    b, c, yy = Phi.T @ yv, dPhi.T @ yv, yv @ yv
    A = G + s2 * np.eye(M, dtype=dtype)
    L = _chol(A, dtype)
    W = _linv(L, dtype)
    t = W @ b
    u = W.T @ t
    T1 = np.sum(W * W)
    trs = np.sum((W @ S) * W)
    tt, uu, uc, usu = t @ t, u @ u, u @ c, u @ (S @ u)
    ld = np.sum(np.log(np.diag(L)))
    nm = dtype(n - M)
    Q = (yy - tt) / s2
    hld = nm * np.log(sg) + ld
    half_log_2pi = np.log(2 * (np.pi if dtype is float else dtype(4) * np.arctan(dtype(1)))) / 2
    out3 = np.array([-hld - Q / 2 - half_log_2pi * n, hld, Q])
    grad = np.array([(uu - M + s2 * T1) / am, (uc - usu / 2) / s2 - trs / 2, Q / sg - uu / sg - nm / sg - sg * T1])
    Ainv = W.T @ W
    au = np.abs(u)
    gabs = np.array([(uu + M + s2 * T1) / am,
                     (au @ np.abs(c) + au @ (np.abs(S) @ au) / 2) / s2 + np.sum(np.abs(Ainv) * np.abs(S)) / 2,
                     ((yy + tt) / s2 + uu + abs(nm)) / sg + sg * T1])   # Q by its two terms: they cancel
    AA = np.abs(np.asarray(Ainv, float)) @ np.abs(np.asarray(A, float))
    return {"out3": out3, "grad": grad, "gabs": gabs.astype(float), "cond": float(np.max(AA.sum(axis=1))), "trcond": float(np.trace(AA)),
            "yy": float(yy), "sumlog": float(np.sum(np.abs(np.log(np.diag(L))))), "n": n, "M": M, "sigma": float(sigma)}


def marginal_dense(x, y, M, scale, amp, l, sigma):
    """The long-double reference: n x n Cholesky of Phi Phi^T + sigma^2 I, gradient by one trace per parameter."""
    Phi, dPhi = basis_ld(x, M, scale, amp, l)
    yv = np.asarray(y, float).astype(LD)
    n = len(yv)
    sg, am = LD(sigma), LD(amp)
    Sig = Phi @ Phi.T + sg * sg * np.eye(n, dtype=LD)
    L = vr._chol_ld(Sig)
    zf = vr._fwd_solve_ld(L, yv)
    a = cg._bwd_solve_ld(L, zf)
    Li = vr._fwd_solve_ld(L, np.eye(n, dtype=LD))
    Sinv = Li.T @ Li
    hld = np.sum(np.log(np.diag(L)))
    Q = zf @ zf
    half_log_2pi = np.log(2 * LD(4) * np.arctan(LD(1))) / 2
    out3 = np.array([-hld - Q / 2 - half_log_2pi * n, hld, Q])
    dS = (2 / am * (Phi @ Phi.T), dPhi @ Phi.T + Phi @ dPhi.T, 2 * sg * np.eye(n, dtype=LD))
    grad = np.array([a @ (d @ a) / 2 - np.sum(Sinv * d) / 2 for d in dS])
    return {"out3": out3, "grad": grad}


@functools.lru_cache(maxsize=None)
def marginal_reference(case):
    """(inputs, dense long-double reference, float64 identity record) of one entry of CASES or BIG_CASES."""
    n, M, l = case
    x, y, z, Y = case_inputs(*case)
    if case in BIG_CASES:
        rec = json.load(open(GOLDEN))["%d_%d_%g" % case]
        ref = {"out3": np.array([LD(s) for s in rec["out3"]]), "grad": np.array([LD(s) for s in rec["grad"]])}
    else:
        ref = marginal_dense(x, y, M, SCALE, AMP, l, SIGMA)
    return (x, y, z, Y), ref, marginal_identity(x, y, M, SCALE, AMP, l, SIGMA)


def bounds(rec):
    """Bounds on |out3 - ref| (3) and |grad - ref| (3) from the record of marginal_identity."""
    ce = BOUND_C * EPS * rec["cond"]
    n, M, sg = rec["n"], rec["M"], rec["sigma"]
    bQ = ce * rec["yy"] / (sg * sg)
    bh = BOUND_C * EPS * (abs((n - M) * np.log(sg)) + rec["sumlog"] + rec["trcond"])
    return {"out3": np.array([bh + bQ / 2 + EPS * n * 0.9189385332046727, bh, bQ]), "grad": ce * rec["gabs"]}


def basis_bounds(Phi, dPhi, l):
    """Bounds on |Phi - ref| and |dPhi - ref| (n x M each) from the long-double reference."""
    aP, aD = np.abs(np.asarray(Phi, float)), np.abs(np.asarray(dPhi, float))
    sP = np.maximum(aP.max(axis=0)[None, :], np.maximum.accumulate(aP, axis=1))
    sD = np.maximum(aD.max(axis=0)[None, :], np.maximum.accumulate(aD, axis=1))
    return BOUND_C * EPS * sP, BOUND_C * EPS * (sD + sP / l)


# ---- the latent form -------------------------------------------------------------------------------------------------------
NORMAL, BERNOULLI = 0, 1


def _head(q, Y, family, sigma, dtype):
    m = Y.shape[1]
    if family == NORMAL:
        r = Y - q[:, None]
        s2 = sigma * sigma
        return (np.sum(-np.log(sigma) - r * r / (2 * s2)), np.sum(-1 / sigma + r * r / (s2 * sigma)), r.sum(axis=1) / s2)
    sp = np.maximum(q, 0) + np.log1p(np.exp(-np.abs(q)))
    pr = 1 / (1 + np.exp(-q))
    return np.sum(Y.sum(axis=1) * q - m * sp), dtype(0), Y.sum(axis=1) - m * pr


def latent_ref(x, M, scale, amp, l, z, family, Y, sigma, dtype=LD):
    """out (2), q, qbar, zbar, grad (2) in long double from the closed form (dtype=float: the float64 transcription)."""
    Phi, dPhi = basis_ld(x, M, scale, amp, l) if dtype is LD else basis_f64(x, M, scale, amp, l)
    Y = np.asarray(Y, float).reshape(len(x), -1).astype(dtype)
    zv = np.asarray(z, float).astype(dtype)
    q = Phi @ zv
    lik, dsig, qbar = _head(q, Y, family, dtype(sigma), dtype)
    return {"out": np.array([lik, dsig]), "q": q, "qbar": qbar, "zbar": Phi.T @ qbar,
            "grad": np.array([qbar @ q / dtype(amp), qbar @ (dPhi @ zv)])}


latent_f64 = functools.partial(latent_ref, dtype=float)


def latent_bounds(x, M, scale, amp, l, z, family, Y, sigma):
    """Bounds on every output of the latent call from the long-double reference."""
    Phi, dPhi = basis_ld(x, M, scale, amp, l)
    ref = latent_ref(x, M, scale, amp, l, z, family, Y, sigma)
    bP, bD = basis_bounds(Phi, dPhi, l)
    aP, aD = np.abs(np.asarray(Phi, float)), np.abs(np.asarray(dPhi, float))
    az = np.abs(np.asarray(z, float))
    Y = np.asarray(Y, float).reshape(len(x), -1)
    m = Y.shape[1]
    ce = BOUND_C * EPS
    q, qbar = np.asarray(ref["q"], float), np.asarray(ref["qbar"], float)
    bq = bP @ az + ce * (aP @ az)
    bqd = bD @ az + ce * (aD @ az)
    qd = np.asarray(dPhi @ np.asarray(z, float).astype(LD), float)
    if family == NORMAL:
        s2 = sigma * sigma
        r = Y - q[:, None]
        bqbar = m * bq / s2 + ce * np.abs(r).sum(axis=1) / s2
        blik = float(np.sum(np.abs(qbar) * bq) + ce * np.sum(np.abs(np.log(sigma)) + r * r / (2 * s2)))
        bds = float(np.sum(2 * np.abs(r).sum(axis=1) * bq) / (s2 * sigma) + ce * np.sum(1 / sigma + r * r / (s2 * sigma)))
    else:
        bqbar = m * bq / 4 + ce * m
        blik = float(np.sum(np.abs(qbar) * bq) + ce * np.sum(m * (np.abs(q) + 1.0)))
        bds = 0.0
    aqb = np.abs(qbar)
    bz = aP.T @ bqbar + bP.T @ aqb + ce * (aP.T @ aqb)
    bg0 = float(bqbar @ np.abs(q) + aqb @ bq + ce * (aqb @ np.abs(q))) / amp
    bg1 = float(bqbar @ np.abs(qd) + aqb @ bqd + ce * (aqb @ np.abs(qd)))
    return ref, {"out": np.array([blik, bds]), "q": bq, "qbar": bqbar, "zbar": bz, "grad": np.array([bg0, bg1])}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (a bound of zero admits an error of zero only)."""
    e = np.abs(np.asarray(got, LD) - np.asarray(ref, LD)).astype(float).ravel()
    b = np.broadcast_to(np.asarray(bound, float), np.asarray(ref).shape).ravel()
    if e.size == 0:
        return 0.0
    return float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e == 0, 0.0, np.inf))))


def truncation_bound(M, scale, amp, l, xmax):
    """An upper bound on max |amp^2 exp(-(x_i - x_j)^2 / (2 l^2)) - (Phi Phi^T)_ij| for |x| <= xmax, reasoned, not measured: the
    entry's error is the tail sum_{k >= M} Phi_ik Phi_jk, at most the tail of the diagonal (Cauchy-Schwarz).  With t = alpha beta x,
    exp(-delta^2 x^2) = exp(-t^2 / 2) exp(alpha^2 x^2 / 2), and Cramer's inequality |H_k(t)| exp(-t^2 / 2) <= 1.0865 sqrt(2^k k!)
    gives Phi_ik^2 <= amp^2 sqrt(alpha^2 / Dn) beta 1.0865^2 exp(alpha^2 x^2) r^k, a geometric series in r = eps^2 / Dn."""
    c0, r, _, _ = (float(v) for v in _scalars(scale, l))
    al2 = 1.0 / (2.0 * scale * scale)
    return amp * amp * c0 * c0 * 1.0865 ** 2 * np.exp(al2 * xmax * xmax) * r ** M / (1.0 - r)


# the points at which Phi Phi^T has converged to the kernel (x in [-0.5, 0.5], scale 0.25): (l, M)
CONVERGED = ((1.0, 10), (0.3, 20), (0.3, 40), (0.1, 64), (0.1, 128))


def se_kernel_ld(x, amp, l):
    xv = np.asarray(x, float).astype(LD)
    return LD(amp) ** 2 * np.exp(-((xv[:, None] - xv[None, :]) ** 2) / (2 * LD(l) ** 2))


def all_ratios(case):
    """Worst error / bound of the float64 transcription on one case, per quantity."""
    n, M, l = case
    (x, y, z, Y), ref, rec = marginal_reference(case)
    Phi, dPhi = basis_ld(x, M, SCALE, AMP, l)
    bP, bD = basis_bounds(Phi, dPhi, l)
    P64, D64 = basis_f64(x, M, SCALE, AMP, l)
    b = bounds(rec)
    out = {"Phi": worst_ratio(P64, Phi, bP), "dPhi": worst_ratio(D64, dPhi, bD),
           "out3": worst_ratio(rec["out3"], ref["out3"], b["out3"]), "grad": worst_ratio(rec["grad"], ref["grad"], b["grad"])}
    for fam, Yc in ((NORMAL, Y), (BERNOULLI, Y[:, :1])):
        lref, lb = latent_bounds(x, M, SCALE, AMP, l, z, fam, Yc, SIGMA)
        got = latent_f64(x, M, SCALE, AMP, l, z, fam, Yc, SIGMA)
        for k in lb:
            out["lat%d_%s" % (fam, k)] = worst_ratio(got[k], lref[k], lb[k])
    return out


def write_golden():
    rec = {}
    for case in BIG_CASES:
        x, y, _, _ = case_inputs(*case)
        ref = marginal_dense(x, y, case[1], SCALE, AMP, case[2], SIGMA)
        rec["%d_%d_%g" % case] = {k: [np.format_float_scientific(v, precision=22, unique=False) for v in ref[k]] for k in ("out3", "grad")}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":   # the figures of the module docstring
    import sys
    if "--golden" in sys.argv[1:]:
        write_golden()
        sys.exit(0)
    worst = {}
    for case in CASES + BIG_CASES:
        r = all_ratios(case)
        print(case, " ".join("%s %.3f" % kv for kv in r.items()))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst", {k: round(v, 3) for k, v in worst.items()})
