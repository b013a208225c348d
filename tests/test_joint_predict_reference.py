"""CPU: the yardstick of gpmi_joint_predict (tests/joint_predict_reference.py) -- the conditions its parity inputs meet, the
constants that tie the GPU parity tests' tolerances to the reference's own float64-vs-longdouble error, the new entry points'
presence in the header, the built library and the bindings, and what the compiler makes of the new one-workgroup kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import joint_grad_reference as jg
import joint_predict_reference as jp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmi_joint_predict", "gpmi_joint_predict_dev")


@pytest.mark.parametrize("case", jg.PARITY_CASES, ids=lambda c: "n%d" % c[0])
def test_inputs_meet_their_conditions(case):
    """cond_2(S) <= COND_MAX; for every order set the float64 reference's C factors, and scaled by 1 / (s_i s_j), s_i = alpha / l^a,
    its smallest eigenvalue is at least 0.99e-6 (post_jitter puts 1e-6 on the scaled diagonal).  Conditions, not tolerances."""
    _, l = case
    m = jp.case_m(case)
    cond = jp.case_cond(case)
    assert cond <= jg.COND_MAX
    for mask in jp.ORDER_SETS:
        C = np.asarray(jp.reference(case, mask, False)[1])
        s = jp.scales(l, mask, m)
        lam = float(np.linalg.eigvalsh(C / np.outer(s, s))[0])
        print("n = %d orders %d: cond_2(S) %.2e smallest scaled eigenvalue %.3e" % (case[0], mask, cond, lam))
        np.linalg.cholesky(C)
        assert lam >= 0.99e-6


def test_tolerance_constants_come_from_the_reference_own_error():
    for case in jg.PARITY_CASES:
        for mask in jp.ORDER_SETS:
            print("n = %d orders %d: rho_mean %.3f rho_cov %.3f" % ((case[0], mask) + jp.rho(case, mask)))
    cm, cc = jp.constants()
    print("C_mean = %.3f  C_cov = %.3f" % (cm, cc))
    assert np.isfinite(cm) and cm > 0
    assert np.isfinite(cc) and cc > 0


def test_blocks_are_the_derivatives_of_the_kernel():
    """The nine closed forms against nested central differences of the QQ block in long double, step h = 1e-3: truncation of the
    order of h^2 / l^2 = 3e-6 per difference, rounding at most 1e-19 / h^4 = 1e-7 (two second differences), both relative to the
    block's scale alpha^2 / l^(a + b).  A check of signs and argument order, to 1e-4 of that scale."""
    x = np.array([-0.7, 0.1, 0.45])
    y = np.array([-0.3, 0.2])
    alpha, l = 1.1, 0.6
    h = jp.LD(1e-3)
    k = jp.blocks(x, y, alpha, l, jp.LD)

    def q(dx, dy):
        return jp.blocks(x.astype(jp.LD) + dx * h, y.astype(jp.LD) + dy * h, alpha, l, jp.LD)[0][0]

    def diff(f, order):   # central difference of the given order of f(step)
        return (f(1) - f(-1)) / (2 * h) if order == 1 else (f(1) - 2 * f(0) + f(-1)) / (h * h)

    for a in range(3):
        for b in range(3):
            fx = (lambda dy: q(0, dy)) if a == 0 else (lambda dy, a=a: diff(lambda dx: q(dx, dy), a))
            got = fx(0) if b == 0 else diff(fx, b)
            scale = alpha ** 2 / l ** (a + b)
            assert float(np.max(np.abs(got - k[a][b]))) <= 1e-4 * scale, (a, b)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    from gp_amd import _build, _lib
    lib = _build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for nm in NAMES:
        assert re.search(r"GPMI_API int %s\(" % nm, hdr), nm
        assert nm in exported, nm
        assert nm in _lib.SYMBOLS, nm
    assert callable(_lib.Context.joint_predict) and callable(_lib.Context.joint_predict_dev)
    rsrc = open(os.path.join(ROOT, "r", "gpmi.R")).read()
    shim = open(os.path.join(ROOT, "r", "gpmi_shim.c")).read()
    assert re.search(r"^joint_predict <- function", rsrc, flags=re.M)
    assert '.Call("gpmi_R_joint_predict"' in rsrc and re.search(r"^SEXP gpmi_R_joint_predict\(", shim, flags=re.M)


def test_one_workgroup_kernel_stays_inside_its_siblings_resources():
    """k_joint_predict_wg lives in small_kernels.hip beside the kernel it is modelled on: 256 registers, no AGPR copies around
    factor16's DPP chain, and no more scratch than k_gp_predict_joint_wg.  The figures come from the one compilation
    tests/test_small_kernels_build.py shares (minutes)."""
    from test_small_kernels_build import small_kernels
    kernels = small_kernels()
    new = kernels["k_joint_predict_wg"]
    sib = kernels["k_gp_predict_joint_wg"]
    print("k_joint_predict_wg", new, "k_gp_predict_joint_wg", sib)
    assert new["AGPRs"] == 0
    assert new["VGPRs"] <= 256
    assert new["ScratchSize [bytes/lane]"] <= sib["ScratchSize [bytes/lane]"]
