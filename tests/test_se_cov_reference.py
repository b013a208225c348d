"""CPU: what tests/test_gpu_se_cov_accuracy.py rests on (tests/se_cov_reference.py).  The long-double exp is an adequate
reference for a 1-ulp claim (float64 libm, an independent implementation, stays under 1 ulp of it over the whole range, the
subnormal results included); the points reach every reduction boundary, the subnormal range and the clamp; a float64 restatement
of the kernels' order of operations stays inside the derived per-entry bound on every case; and the cases' entries are large
enough for a relative bound to mean something (a builder that wrote zeros off the diagonal must not pass again)."""
import numpy as np
import pytest

import se_cov_reference as sr

CASES = [(n, m, D, ard) for (n, m, D) in sr.RECT_CASES for ard in (False, True)]
IDS = ["%dx%d-D%d-%s" % (n, m, D, "ard" if ard else "iso") for (n, m, D, ard) in CASES]


def test_exp_points_cover_the_range_the_boundaries_and_the_clamp():
    t = sr.exp_points()
    x = sr.exp_argument(t)
    assert 4000 <= t.size <= 4200 and np.all(t >= 0) and np.all(x <= 0)
    assert x.max() == 0.0 and x.min() == -800.0
    inside = x[x > -800.0]
    assert inside.min() < -745.0 and inside.min() > -750.0          # down to the last subnormal and just past it
    assert np.max(np.diff(np.sort(inside))) < 0.5                   # no gap: every binade of the result is hit
    n = np.rint(inside / sr.LN2)
    for k in (0, -1, -2, -511, -1022, -1023, -1074):                # both sides of each boundary, within a few ulps of it
        for half in (-0.5, 0.5):
            b = (k + half) * sr.LN2
            if b < 0:
                near = inside[np.abs(inside - b) <= 8 * np.spacing(abs(b))]
                assert near.size >= 5 and near.min() < b < near.max(), (k, half)
                assert set(np.rint(near / sr.LN2)) == {k + (-1 if half < 0 else 0), k + (0 if half < 0 else 1)}, (k, half)
    assert n.min() <= -1075
    real, _, sub = sr.exp_errors(np.exp(x), x)
    assert np.count_nonzero(sub) >= 50 and np.count_nonzero(~sub) >= 3900


def test_long_double_exp_is_an_adequate_reference():
    """float64 libm against the long-double exp at the same arguments: under 1 ulp (1 subnormal spacing below 2^-1022)
    everywhere.  Two independent implementations that agree to that are each good to it; the long-double one has 11 more bits."""
    x = sr.exp_argument(sr.exp_points())
    real, rounded, sub = sr.exp_errors(np.exp(x), x)
    print("float64 libm exp against long double: worst %.3f ulp (normal results), %.3f spacings (subnormal results)"
          % (real[~sub].max(), real[sub].max()))
    assert real.max() < 1.0
    assert rounded.max() <= 1.0
    assert np.finfo(sr.LD).nmant >= 63 and np.finfo(sr.LD).minexp <= -16000   # an x87 extended double, not an alias of double


def test_ulp_at():
    assert float(sr.ulp_at(sr.LD(1.0))) == 2.0 ** -52 and float(sr.ulp_at(sr.LD(0.75))) == 2.0 ** -53
    assert float(sr.ulp_at(sr.LD(2.0) ** -1022)) == 2.0 ** -1074 and float(sr.ulp_at(sr.LD(2.0) ** -1030)) == 2.0 ** -1074
    assert float(sr.ulp_at(sr.LD(2.0) ** -1021)) == 2.0 ** -1073


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_restatement_within_the_derived_bound(case):
    X, Y, alpha, ell = sr.rect_case(*case)
    ref, bound = sr.rect_reference(*case)
    err = sr.rel_errors(sr.se_cov_float64(X, Y, alpha, ell), ref)
    n, m, D, _ = case
    off = np.ones((n, m), bool)
    off[n // 2, m // 3] = False                                     # the coincident pair
    share = float(np.mean(ref[off] > 1e-12 * alpha ** 2)) if off.any() else 1.0
    print("%s: error / bound %.3f (bound %.1f .. %.1f eps); entries %.1e .. %.1e alpha^2, %.1f %% above 1e-12 alpha^2"
          % (case, float(np.max(err / bound)), bound.min() / sr.EPS, bound.max() / sr.EPS, float(ref.min()) / alpha ** 2,
             float(ref[off].max() if off.any() else ref.max()) / alpha ** 2, 100 * share))
    assert np.all(err <= bound)
    assert share >= 0.9
    assert float(ref[n // 2, m // 3]) == pytest.approx(alpha ** 2, rel=1e-15)
    assert bound.max() <= 1e4 * sr.EPS                              # the bound itself stays a statement about rounding
    # teeth: the same restatement with one dimension's length-scale taken from its neighbour leaves the bound
    if case[3] and D > 1:
        wrong = np.array(ell)
        wrong[[0, 1]] = wrong[[1, 0]]
        assert np.any(sr.rel_errors(sr.se_cov_float64(X, Y, alpha, wrong), ref) > bound)


def test_symmetric_restatement_within_the_bound():
    X, _, alpha, ell = sr.rect_case(129, 193, 17, True)
    ref = sr.se_cov_longdouble(X, X, alpha, ell)
    bound = sr.se_cov_rel_bound(X, X, ell)
    K = sr.se_cov_float64(X, X, alpha, ell)
    assert np.all(sr.rel_errors(K, ref) <= bound)
    assert np.array_equal(K, K.T)
