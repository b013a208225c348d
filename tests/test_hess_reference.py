"""CPU: the references of tests/hess_reference.py against each other, before the device is compared with them
(tests/test_gpu_hess.py): the parity inputs satisfy the conditioning the bound assumes; the float64 statement of the device's
algebra stays within HALF of every bound; the long-double Hessian (one product per hyper-parameter) is symmetric, equals central
differences of the long-double gradient, and equals the device's algebra (closed forms for alpha and sigma) in long double."""
import numpy as np
import pytest

import hess_reference as hr
import logml_grad_reference as lg

EPS_LD = float(np.finfo(np.longdouble).eps)


def test_the_cases_cover_what_the_kernels_branch_on():
    cases = hr.HESS_CASES
    assert {c[0] for c in cases} == {1, 2, 63, 65, 129, 257, 385}
    assert all(hr.n_ell_of(c) <= hr.MAX_ELL for c in cases)
    assert any(c[2] and c[1] == 8 for c in cases) and any(c[2] and 1 < c[1] < 8 for c in cases)      # ARD, D = 8 and below
    assert any(not c[2] and c[1] > 8 for c in cases) and any(not c[2] and c[1] == 64 for c in cases)   # isotropic, D > 8
    assert {c[3] for c in cases} == {0.15, 1e-3, 0.0}
    assert any(c[4] == "dup" for c in cases) and lg.CANCEL_CASE in cases


@pytest.mark.parametrize("case", hr.HESS_CASES, ids=lg.case_id)
def test_float64_is_within_half_of_every_bound(case):
    inp, ref, cond = hr.parity_reference(case)
    assert cond <= lg.COND_MAX, cond
    q = 2 + hr.n_ell_of(case)
    assert ref["hess"].shape == (q, q) and ref["habs"].shape == (q, q)
    r = hr.ratio(hr.hess_float64(*inp), ref, cond)
    print(lg.case_id(case), "cond %.1e" % cond, "error / bound %.3f" % r)
    assert r <= 0.5, r


@pytest.mark.parametrize("case", hr.HESS_CASES, ids=lg.case_id)
def test_long_double_hessian_is_symmetric_and_equals_the_closed_forms(case):
    inp, ref, cond = hr.parity_reference(case)
    H = ref["hess"]
    # two long-double evaluations of the same numbers: a few hundred long-double roundings times cond
    tol = 300.0 * EPS_LD * (cond * ref["hmax"] + ref["habs"])
    assert np.all(np.abs(H - H.T).astype(float) <= tol)
    err = np.abs(hr.hess_shortcut(*inp, dtype=np.longdouble) - H).astype(float)
    assert np.all(err <= tol), float(np.max(err / tol))


@pytest.mark.parametrize("case", hr.DIFF_CASES, ids=lg.case_id)
def test_long_double_hessian_equals_central_differences_of_the_gradient(case):
    """The tolerance of test_long_double_gradient_equals_central_differences (tests/test_loo_reference.py: step 1e-6, 1e-8 of the
    scale), relative to hmax: a check of the reference, not a device tolerance."""
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    ref = hr.hess_reference(X, y, a, ell, s, jit)
    theta, h = hr.fd_steps(a, ell, s, hrel=1e-6, hmin=1e-3)
    grad = lambda t: lg.logml_grad_reference(X, y, t[0], t[1:-1], t[-1], jit, np.longdouble)["grad"]
    F = hr.fd_hessian(grad, theta, h, np.longdouble)
    err = np.abs(F - ref["hess"]).astype(float)
    assert np.all(err <= 1e-8 * ref["hmax"]), (err / ref["hmax"])


def test_the_finite_difference_case_is_well_conditioned():
    _, theta, h, ref, cond, trunc, gb = hr.fd_reference(hr.FD_CASE)
    assert cond <= lg.COND_MAX and theta.size == 5
    print("cond %.1e; truncation / hmax %.2e; gradient bounds over 2 h / hmax %.2e" % (
        cond, float(np.max(trunc)) / ref["hmax"], float(np.max(gb)) / ref["hmax"]))
    # the stencil resolves the Hessian: what it cannot see is below a thousandth of the largest entry
    assert float(np.max(trunc + gb)) <= 1e-3 * ref["hmax"]
