"""GPU: relative accuracy of the squared-exponential covariance builder against long double (tests/se_cov_reference.py, whose
docstring derives the bounds; tests/test_se_cov_reference.py shows the conditions they rest on).

exp_nonpos (gp_amd/csrc/se_device.h) in ulps over its whole range -- the two-part argument reduction at large |x|, both sides
of the reduction boundaries, the subnormal results, the clamp at -800 -- through the guarded edge tiles and the unguarded
interior tiles of k_se_cov<1>; and every entry of the full builder at D = 3 .. 64 (k_se_cov<3>, k_se_cov_big with one to four
16-dimension stages) on inputs whose entries are not negligible, where tests/test_gpu_parity.py::test_se_cov_rect bounds the
absolute error only."""
import numpy as np
import pytest

import se_cov_reference as sr

pytestmark = pytest.mark.gpu

CASES = [(n, m, D, ard) for (n, m, D) in sr.RECT_CASES for ard in (False, True)]
IDS = ["%dx%d-D%d-%s" % (n, m, D, "ard" if ard else "iso") for (n, m, D, ard) in CASES]


def test_exp_nonpos_in_ulps(ctx):
    """The claim of the comment in se_device.h, "<= 1 ulp of error": normal results within EXP_ULPS = 1 ulp of the long-double
    value (so within 1 ulp of the correctly rounded double as well); results below 2^-1022, where ldexp rounds a second time,
    within 1 subnormal spacing of the correctly rounded one."""
    t = sr.exp_points()
    x = sr.exp_argument(t)
    got = ctx.se_cov(np.zeros((1, 1)), t[:, None], 1.0, [1.0])
    assert got.shape == (1, t.size)
    got = got[0]
    real, rounded, sub = sr.exp_errors(got, x)
    kn, ks = int(np.argmax(np.where(sub, 0, real))), int(np.argmax(np.where(sub, real, 0)))
    print("exp_nonpos against long double: worst %.3f ulp at x = %r (normal results), %.3f spacings at x = %r (subnormal results); "
          "from the correctly rounded double: %g ulp" % (real[kn], x[kn], real[ks], x[ks], rounded.max()))
    assert np.all(real[~sub] <= sr.EXP_ULPS), (x[kn], real[kn])
    assert np.all(rounded <= 1.0), (x[np.argmax(rounded)], rounded.max())
    assert got[x == 0.0][0] == 1.0 and got[t == 40.0][0] == 0.0 and np.all(got >= 0.0)
    assert np.all(np.diff(got[:4000]) <= 0.0)    # monotone over the evenly spaced part (t increasing)
    assert np.count_nonzero(got[sub] > 0) >= 40  # the subnormal results are there, not flushed to zero


def test_exp_nonpos_same_bits_in_interior_and_edge_tiles(ctx):
    """65 identical rows: rows 0 .. 63 of the whole column tiles run the unguarded interior form, row 64 and the last, ragged
    column tile the guarded one; every row equals the one-row call bit for bit."""
    t = sr.exp_points()
    one = ctx.se_cov(np.zeros((1, 1)), t[:, None], 1.0, [1.0])[0]
    K = ctx.se_cov(np.zeros((65, 1)), t[:, None], 1.0, [1.0])
    assert t.size % 64 != 0 and K.shape == (65, t.size)
    assert np.array_equal(K, np.broadcast_to(one, K.shape))
    # ... and as rows of the operand on the other side (the column coordinate is the wave-uniform one)
    KT = ctx.se_cov(t[:, None], np.zeros((65, 1)), 1.0, [1.0])
    assert np.array_equal(KT, K.T)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_relative_accuracy_of_every_entry(ctx, case):
    X, Y, alpha, ell = sr.rect_case(*case)
    ref, bound = sr.rect_reference(*case)
    n, m, D, _ = case
    K = ctx.se_cov(X, Y, alpha, ell)
    err = sr.rel_errors(K, ref)
    k = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    print("%s: worst error / bound %.3f at %s (error %.2f eps, entry %.2e)" % (case, err[k] / bound[k], k, err[k] / sr.EPS, K[k]))
    assert np.all(err <= bound), (k, err[k] / bound[k])
    assert K[n // 2, m // 3] == alpha * alpha    # the coincident pair: exp(0) = 1 exactly


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_symmetric_call(ctx, case):
    """Y = None: the same bound on the lower triangle, bit-symmetric, the diagonal exactly alpha^2 + diag_add, and the LOWER
    form equal to the lower triangle of the full one with nothing written above it."""
    from gp_amd._lib import LOWER
    X, _, alpha, ell = sr.rect_case(*case)
    n = case[0]
    ref = sr.se_cov_longdouble(X, X, alpha, ell)
    bound = sr.se_cov_rel_bound(X, X, ell)
    K = ctx.se_cov(X, None, alpha, ell, diag_add=0.0225)
    Kl = ctx.se_cov(X, None, alpha, ell, diag_add=0.0225, flags=LOWER)
    off = ~np.eye(n, dtype=bool)
    err = sr.rel_errors(K, ref)
    print("%s symmetric: worst error / bound %.3f" % (case, float(np.max((err / bound)[off]))))
    assert np.all(err[off] <= bound[off])
    assert np.array_equal(K, K.T)
    assert np.all(np.diag(K) == alpha * alpha + 0.0225)
    assert np.array_equal(np.tril(Kl), np.tril(K)) and np.all(np.triu(Kl, 1) == 0.0)
