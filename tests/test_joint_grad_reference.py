"""CPU: the reference of gpmi_joint_logml_grad (tests/joint_grad_reference.py) against the oracle's joint matrix and value,
against central differences of itself, float64 against long double on every parity input (with the cap on cond_2 that the
GPU bounds of tests/test_gpu_joint_grad.py rest on), and the ABI declarations of the three entry points."""
import os
import re

import numpy as np
import pytest

import joint_grad_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmi_joint_logml_grad", "gpmi_joint_logml_grad_dev", "gpmi_joint_logml_grad_grid")


def test_matrix_and_value_equal_the_oracle(orc):
    t = np.linspace(-2, 2, 21)
    yy = np.concatenate([np.sin(t), np.cos(t)])
    a, l, s, jit = 1.1, 0.9, 0.05, 1e-6
    ref = jr.joint_reference(t, yy, a, l, s, jit)
    K = orc.joint_cov(t, a, l, s, jit)
    np.testing.assert_allclose(ref["S"], K, rtol=1e-14, atol=0)
    lm, sld, q, info = orc.joint_logml(t, yy, a, l, s, jit)
    assert info == 0
    # the tolerance of tests/test_oracle.py::test_joint_cov_and_posteriors for this function
    assert float(ref["out3"][0]) == pytest.approx(lm, rel=1e-9)
    assert float(ref["out3"][1]) == pytest.approx(sld, rel=1e-9) and float(ref["out3"][2]) == pytest.approx(q, rel=1e-9)


def test_gradient_equals_central_differences_of_the_value():
    """Well conditioned (cond ~ 1e3): the formulas, not the arithmetic."""
    t, yy = jr.case_inputs(30, seed=5)
    th = np.array([1.1, 0.25, 0.4])
    jit = 1e-2

    def f(p):
        return float(jr.joint_reference(t, yy, p[0], p[1], p[2], jit)["out3"][0])

    g = jr.joint_reference(t, yy, *th, jit)["grad"]
    h = 1e-6
    fd = np.array([(f(th + h * e) - f(th - h * e)) / (2 * h) for e in np.eye(3)])
    assert np.max(np.abs(g - fd)) <= 1e-8 * np.max(np.abs(g)), (g, fd)


@pytest.mark.parametrize("case", jr.PARITY_CASES, ids=lambda c: "n%d-l%g" % c)
def test_float64_against_long_double(case):
    """The conditions the centred-GP reference test sets: cond <= COND_MAX, and the float64 restatement within
    1 cond eps max|grad| + 32 eps gabs of the long-double one."""
    _, ref, cond = jr.parity_reference(case)
    _, r64, _ = jr.parity_reference(case, False)
    assert cond <= jr.COND_MAX, cond
    ce = cond * jr.EPS
    err = np.abs(r64["grad"].astype(np.longdouble) - ref["grad"]).astype(float)
    bound = ce * float(np.max(np.abs(ref["grad"]))) + 32 * jr.EPS * ref["gabs"]
    e3 = np.abs((r64["out3"].astype(np.longdouble) - ref["out3"]) / ref["out3"]).astype(float)
    print("n %d l %g: cond %.1e; grad error / bound %s; out3 in cond eps %s" % (case[0], case[1], cond, err / bound, e3 / ce))
    assert np.all(err <= bound), err / bound
    assert np.all(e3[1:] <= ce), e3 / ce


def test_abi_declares_the_three_functions():
    from gp_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmi.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"GPMI_API\s+int\s+%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+GPMI_VERSION\s+302\b", src)
