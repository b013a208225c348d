"""CPU references for the squared-exponential covariance builder (se_cov_tile, k_se_cov_big and the hand-written exp_nonpos of
gp_amd/csrc/se_device.h).  Helper of tests/test_se_cov_reference.py and tests/test_gpu_se_cov_accuracy.py (not collected: no
test_ prefix).

exp_nonpos alone.  Context.se_cov(X=[[0.0]], Y=t[:, None], alpha=1, ell=[1]) returns exactly exp_nonpos(-0.5 rn(t^2)): the
scaling by 1 / 1 and the difference from 0 are exact, fma(d, d, 0) is one rounding (numpy's t * t), the halving is exact and
alpha^2 = 1.  The reference is np.exp of that same float64 argument in np.longdouble (64-bit significand: 2^-11 ulp of a
double).  Errors are counted in ulps of the double at the reference value, below 2^-1022 in the subnormal spacing 2^-1074.

The whole builder.  K_ij = alpha^2 exp(-1/2 s), s = sum_d d_d^2, d_d = (x_d - y_d) / ell_d.  The kernels compute, with
u = 2^-53 and every operation rounded once,
  ie_d = rn(1 / ell_d),  xs = rn(x_d ie_d),  ys = rn(y_d ie_d),  dh_d = rn(xs - ys),  sh = fma(dh_d, dh_d, sh) (d = 0 .. D - 1),
  K = rn(rn(alpha^2) exp_nonpos(-sh / 2)).
  |dh_d - d_d| <= u (2 |d_d| + (|x_d| + |y_d|) / ell_d)       ie and the subtraction: u |d_d| each; the two scalings: u |x_d| / ell_d
                                                              and u |y_d| / ell_d
  |sum dh^2 - s| <= 2 sum_d |d_d| |dh_d - d_d| = u (4 s + 2 sum_d |d_d| (|x_d| + |y_d|) / ell_d)
  |sh - sum dh^2| <= D u s                                    the fma chain: term d is rounded D - d times, all terms >= 0
so |sh - s| <= u ((D + 4) s + 2 sum_d |d_d| (|x_d| + |y_d|) / ell_d), and an error e of the argument -s / 2 is a relative
error e of the exponential.  exp_nonpos adds EXP_ULPS ulps = at most 2 EXP_ULPS u relative, rn(alpha^2) and the product u each:
  |K - K_exact| / K_exact <= u (C0 + (D + 5) / 2 s + sum_d |d_d| (|x_d| + |y_d|) / ell_d),   C0 = 2 + 2 EXP_ULPS + 1,
where D + 5 instead of D + 4 lets the float64 numpy restatement square and add in two roundings (it has no fma: u s more), and
the last 1 of C0 covers the terms of second order and the long-double reference's own error (2^-11 of all the above).  Nothing
here is fitted to what the device returns; EXP_ULPS is the code's documented claim.
"""
import functools
import math

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(float).eps)
U = EPS / 2
EXP_ULPS = 1.0            # se_device.h: "<= 1 ulp of error like the library routine"
ALPHA = 1.3
LN2 = math.log(2.0)
# (n, m, D): ragged and whole 64 / 128 tiles of k_se_cov<D> (D <= 3) and k_se_cov_big, one to four 16-dimension stages, m = 1
RECT_CASES = ((65, 130, 3), (130, 129, 8), (70, 33, 9), (64, 64, 16), (129, 193, 17), (100, 70, 33), (65, 1, 48), (100, 70, 64))


# ---- exp_nonpos ----------------------------------------------------------------------------------------------------------------
def exp_points():
    """t >= 0 whose arguments x = -0.5 rn(t^2) cover [-745, 0] (4000 evenly spaced t in [0, 38.7]), the arguments next to the
    reduction boundaries x = k ln2 +- ln2 / 2 for k in {0, -1, -2, -511, -1022, -1023, -1074} (the three doubles on either side of
    each t), and t = 40 (x = -800, the clamp: the result is exactly 0)."""
    t = [np.linspace(0.0, 38.7, 4000)]
    for k in (0, -1, -2, -511, -1022, -1023, -1074):
        for half in (-0.5, 0.5):
            x = (k + half) * LN2
            if x < 0:
                c = math.sqrt(-2.0 * x)
                lo = c
                hi = c
                near = [c]
                for _ in range(3):
                    lo = np.nextafter(lo, 0.0)
                    hi = np.nextafter(hi, np.inf)
                    near += [lo, hi]
                t.append(np.array(near))
    t.append(np.array([40.0]))
    return np.concatenate(t)


def exp_argument(t):
    """The float64 argument the kernel hands exp_nonpos for the pair (0, t) at ell = 1."""
    t = np.asarray(t, float)
    return -0.5 * (t * t)


def ulp_at(v):
    """Spacing of the doubles at |v| (v long double): 2^(e - 52) for 2^e <= |v| < 2^(e + 1), 2^-1074 below 2^-1022."""
    _, ex = np.frexp(np.asarray(v, LD))
    return np.ldexp(LD(1), np.maximum(ex - 1, -1022) - 52)


def exp_errors(got, arg):
    """(error of `got` against the long-double exp(arg) in ulps of the double there, real-valued; distance of `got` from the
    correctly rounded double in the same unit, an integer; mask of the results below 2^-1022)."""
    ref = np.exp(np.asarray(arg, float).astype(LD))
    ulp = ulp_at(ref)
    g = np.asarray(got, float).astype(LD)
    real = (np.abs(g - ref) / ulp).astype(float)
    rounded = ref.astype(float).astype(LD)
    return real, (np.abs(g - rounded) / ulp).astype(float), np.asarray(ref < np.ldexp(LD(1), -1022))


# ---- the whole builder -----------------------------------------------------------------------------------------------------------
def _ells(ell, D):
    ell = np.atleast_1d(np.asarray(ell, dtype=float))
    return np.full(D, ell[0]) if ell.size == 1 else ell


@functools.lru_cache(maxsize=None)
def rect_case(n, m, D, ard):
    """(X, Y, alpha, ell), deterministic in the arguments: the layouts of logml_grad_reference.case_inputs (D <= 8: about one
    point per length-scale over max(n, m) points; D > 8: coordinates in [0, ell sqrt(18 / D)], mean scaled squared distance 3),
    and one row of X equal to a row of Y: an exact alpha^2 off the diagonal of a rectangular call."""
    rng = np.random.default_rng(100000 * n + 100 * m + 2 * D + (1 if ard else 0))
    ell = 0.6 + 0.4 * rng.random(D) if ard else np.array([0.8])
    scale = float(np.mean(ell)) * max(n, m) ** (1.0 / D) if D <= 8 else ell * math.sqrt(18.0 / D)
    X = rng.random((n, D)) * scale
    Y = rng.random((m, D)) * scale
    X[n // 2] = Y[m // 3]
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, ALPHA, ell


def se_cov_longdouble(X, Y, alpha, ell):
    """alpha^2 exp(-1/2 sum_d ((x_d - y_d) / ell_d)^2) in long double, the formula as specified (divisions, no reciprocal)."""
    X = np.asarray(X, float).astype(LD)
    Y = np.asarray(Y, float).astype(LD)
    e = _ells(ell, X.shape[1]).astype(LD)
    s = np.zeros((X.shape[0], Y.shape[0]), dtype=LD)
    for d in range(X.shape[1]):
        r = (X[:, d][:, None] - Y[:, d][None, :]) / e[d]
        s += r * r
    return LD(alpha) * LD(alpha) * np.exp(-s / 2)


def se_cov_float64(X, Y, alpha, ell):
    """The kernels' order of operations in float64 numpy: reciprocal length-scales, scaled coordinates, differences, squares
    added dimension by dimension (two roundings where the device's fma has one), libm's exp, alpha^2 last."""
    X = np.asarray(X, float)
    Y = np.asarray(Y, float)
    ie = 1.0 / _ells(ell, X.shape[1])
    s = np.zeros((X.shape[0], Y.shape[0]))
    for d in range(X.shape[1]):
        r = (X[:, d] * ie[d])[:, None] - (Y[:, d] * ie[d])[None, :]
        s = s + r * r
    return (alpha * alpha) * np.exp(-0.5 * s)


def se_cov_rel_bound(X, Y, ell, exp_ulps=EXP_ULPS):
    """The per-entry bound on |K - K_exact| / K_exact derived in the module docstring (float64 arithmetic on exact inputs is
    accurate enough for a bound: its own relative error is 1e-15)."""
    X = np.asarray(X, float)
    Y = np.asarray(Y, float)
    D = X.shape[1]
    e = _ells(ell, D)
    s = np.zeros((X.shape[0], Y.shape[0]))
    t = np.zeros_like(s)
    for d in range(D):
        r = np.abs(X[:, d][:, None] - Y[:, d][None, :]) / e[d]
        s += r * r
        t += r * (np.abs(X[:, d])[:, None] + np.abs(Y[:, d])[None, :]) / e[d]
    return U * ((2.0 + 2.0 * exp_ulps + 1.0) + (D + 5) / 2.0 * s + t)


def rel_errors(K, ref):
    """|K - ref| / ref per entry (ref long double, positive)."""
    return (np.abs(np.asarray(K, float).astype(LD) - ref) / ref).astype(float)


@functools.lru_cache(maxsize=None)
def rect_reference(n, m, D, ard):
    """(long-double K, per-entry relative bound) of rect_case(n, m, D, ard), computed once per process."""
    X, Y, alpha, ell = rect_case(n, m, D, ard)
    return se_cov_longdouble(X, Y, alpha, ell), se_cov_rel_bound(X, Y, ell)
