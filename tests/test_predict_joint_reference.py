"""CPU: the yardstick of gpmi_gp_predict_joint (tests/predict_joint_reference.py) -- the tie between the GPU parity tests' two
tolerances and the reference's own float64-vs-longdouble error, the identity that pins its covariance to gpmi_gp_predict's
variance, the new entry points' presence in the header, the built library and the binding list, and what the compiler makes of
the new one-workgroup kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import predict_joint_reference as pj
import predict_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmi_gp_predict_joint", "gpmi_gp_predict_joint_dev")


@pytest.mark.parametrize("case", [c for c in pj.cases() if c[1] <= 300], ids=lambda c: c[0])
def test_tolerances_stand_on_the_reference_own_error(case):
    """100 x the float64-vs-longdouble disagreement of the reference stays below MEAN_TOL / VAR_TOL on every case up to n = 300,
    and C is positive definite by the margin post_jitter gives it."""
    name, n, D, m, alpha, ell, sigma = case
    X, y, Xs = pr.inputs(n, D, m)
    mf, Cf = pj.joint(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER, float)
    ml, Cl = pj.joint(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER, np.longdouble)
    em = pr.max_rel(mf, ml.astype(float))
    ec = float(np.max(np.abs(Cf - Cl.astype(float)))) / alpha ** 2
    lam = float(np.linalg.eigvalsh(Cf)[0])
    print("%s: mean %.2e cov/alpha^2 %.2e smallest eigenvalue %.3e" % (name, em, ec, lam))
    assert em <= pr.MEAN_TOL / 100
    assert ec <= pr.VAR_TOL / 100
    assert np.array_equal(Cf, Cf.T)
    assert lam >= 0.99 * pj.POST_JITTER


@pytest.mark.parametrize("case", [c for c in pj.cases() if c[1] <= 300], ids=lambda c: c[0])
def test_diagonal_is_the_pointwise_variance(case):
    """diag(C) - post_jitter is predict_reference.predict's variance and the mean is its mean.  Both sides form alpha^2 - t.t from
    the same whitened columns t (|t|^2 <= alpha^2); they differ in the order of the n-term dot product (a matrix product
    against a column sum) and in one addition and subtraction of post_jitter: each dot product is within n eps alpha^2 of the
    exact one, the two roundings of post_jitter within eps (alpha^2 + post_jitter) each."""
    name, n, D, m, alpha, ell, sigma = case
    X, y, Xs = pr.inputs(n, D, m)
    mean, Cm = pj.joint(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER)
    want_mean, want_var = pr.predict(X, y, Xs, alpha, ell, sigma, pj.JITTER)
    eps = np.finfo(float).eps
    bound = (2 * n + 4) * eps * alpha ** 2
    err = float(np.max(np.abs(np.diag(Cm) - pj.POST_JITTER - want_var)))
    print("%s: diagonal %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    np.testing.assert_array_equal(mean, want_mean)   # the same expression on the same numbers


def test_lapack_form_agrees_with_the_loops():
    name, n, D, m, alpha, ell, sigma = pj.case("n100_d3")
    X, y, Xs = pr.inputs(n, D, m)
    a = pj.joint(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER)
    b = pj.joint_lapack(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER)
    assert pr.max_rel(a[0], b[0]) < 1e-12 and np.max(np.abs(a[1] - b[1])) < 1e-12


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
    assert callable(_lib.Context.gp_predict_joint) and callable(_lib.Context.gp_predict_joint_dev)
    rsrc = open(os.path.join(ROOT, "r", "gpmi.R")).read()
    shim = open(os.path.join(ROOT, "r", "gpmi_shim.c")).read()
    assert re.search(r"^gp_predict_joint <- function", rsrc, flags=re.M)
    assert '.Call("gpmi_R_gp_predict_joint"' in rsrc and re.search(r"^SEXP gpmi_R_gp_predict_joint\(", shim, flags=re.M)


def test_one_workgroup_kernel_stays_inside_its_siblings_resources():
    """k_gp_predict_joint_wg lives in small_kernels.hip beside the kernels it is composed from: 256 registers, no AGPR copies
    around factor16's DPP chain, and no more scratch than k_sample_derivs_small_batch, its nearest sibling with two
    factorisations.  The figures come from the one compilation tests/test_small_kernels_build.py shares (minutes)."""
    from test_small_kernels_build import small_kernels
    kernels = small_kernels()
    new = kernels["k_gp_predict_joint_wg"]
    sib = kernels["k_sample_derivs_small_batch"]
    print("k_gp_predict_joint_wg", new, "k_sample_derivs_small_batch", sib)
    assert new["AGPRs"] == 0
    assert new["VGPRs"] <= 256
    assert new["ScratchSize [bytes/lane]"] <= sib["ScratchSize [bytes/lane]"]
