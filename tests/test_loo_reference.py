"""CPU: the references of tests/loo_reference.py against each other, before the device is compared with them
(tests/test_gpu_loo.py): the parity inputs satisfy the conditioning the bounds assume; the float64 statement of the device's
algebra stays within HALF of every bound; the long-double hold-out means and variances are those of a model refitted without
the point; the long-double gradient (one product per hyper-parameter) equals central differences of the long-double value and
the gradient by the device's identity."""
import numpy as np
import pytest

import logml_grad_reference as lg
import loo_reference as lr

EPS_LD = float(np.finfo(np.longdouble).eps)


@pytest.mark.parametrize("case", lr.CASES, ids=lg.case_id)
def test_float64_is_within_half_of_every_bound(case):
    inp, ref, cond = lr.parity_reference(case)
    assert cond <= lg.COND_MAX, cond
    r = lr.ratios(lr.loo_float64(*inp), ref, cond)
    print(lg.case_id(case), "cond %.1e" % cond, r)
    assert set(r) == {"mu", "var", "lpd", "loo", "grad"}
    for key, v in r.items():
        assert v <= 0.5, (key, v)


def test_the_delete_cases_are_as_well_conditioned():
    for case, _ in lr.DELETE_CASES:
        assert lr.delete_reference(case)[2] <= lg.COND_MAX


def _delete_check(inp, ref, idx):
    for i in idx:
        m, v = lr.delete_one(*inp, i)
        # two long-double evaluations of the same numbers: cond x a few hundred long-double roundings
        assert abs(float(m - ref["mu"][i])) <= 1e-11 * (abs(float(inp[1][i])) + ref["amax"] * float(ref["var"][i])), (i, m, ref["mu"][i])
        assert abs(float(v - ref["var"][i])) <= 1e-11 * float(ref["var"][i]), (i, v, ref["var"][i])


@pytest.mark.parametrize("case,idx", [(c, tuple(range(c[0]))) for c in lr.CASES if c[0] <= 17] + list(lr.DELETE_CASES)
                         + [((65, 2, False, 0.15, "dup"), (0, 4, 33, 60, 64))],
                         ids=lambda v: lg.case_id(v) if len(v) == 5 and isinstance(v[2], bool) else "i%d" % len(v))
def test_long_double_points_equal_deleting_the_point(case, idx):
    """Every i at n <= 17, five indices at n = 65 (two of them coincident points of the "dup" case)."""
    if case in lr.CASES:
        inp, ref, _ = lr.parity_reference(case)
    else:
        inp, ref, _ = lr.delete_reference(case)
    _delete_check(inp, ref, idx)


DIFF_CASES = ((7, 1, False, 0.15, ""), (40, 3, True, 0.15, ""), (2, 1, True, 0.0, ""), (17, 2, False, 1e-3, ""))


@pytest.mark.parametrize("case", DIFF_CASES, ids=lg.case_id)
def test_long_double_gradient_equals_central_differences(case):
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    ref = lr.loo_reference(X, y, a, ell, s, jit)
    ld = np.longdouble
    theta = np.concatenate([[a], ell, [s]]).astype(ld)
    scale = float(np.max(np.abs(ref["grad"])))
    for k in range(theta.size):
        h = ld(1e-6) * max(abs(theta[k]), ld(1e-3))
        vals = []
        for sgn in (1, -1):
            t = theta.copy()
            t[k] += sgn * h
            vals.append(lr.loo_value(X, y, t[0], t[1:-1], t[-1], jit))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(float(fd - ref["grad"][k])) <= 1e-8 * scale, (k, fd, ref["grad"][k])


@pytest.mark.parametrize("case", lr.CASES, ids=lg.case_id)
def test_identity_gradient_equals_the_per_parameter_gradient_in_long_double(case):
    inp, ref, cond = lr.parity_reference(case)
    g = lr.loo_identity(*inp)
    bound = 100.0 * EPS_LD * (cond * float(np.max(np.abs(ref["grad"]))) + ref["gabs"])
    err = np.abs(g - ref["grad"]).astype(float)
    assert np.all(err <= bound), (err, bound)
