"""CPU: the yardsticks of the exact-GP vector-Jacobian product (tests/vjp_reference.py) pinned by central differences, the
O(n^2 k) suffix-sum form of V = U Phi(W Z^T) the kernels use, and the new entry points' presence in the header, the
Python binding list, the built library and the R wrapper."""
import os
import re

import numpy as np
import pytest

import vjp_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(n, D, n_ell, k, seed=0):
    rng = np.random.default_rng(seed)
    ell = 0.7 + 0.3 * rng.random(n_ell)
    X = rng.random((n, D)) * (ell.mean() * n ** (1.0 / D))     # about one point per length-scale
    return X, 1.3, ell, rng.standard_normal((n, k)), rng.standard_normal((n, k))


def _sum_fbar_f(X, ell_n, Z, Fb, jitter):
    def fun(theta):
        K, _, _ = vr.se_cov(X, theta[0], theta[1:], jitter)
        return float(np.sum(Fb * (np.linalg.cholesky(K) @ Z)))
    return fun


@pytest.mark.parametrize("n,D,n_ell,k", [(40, 2, 2, 2), (40, 1, 1, 1), (25, 3, 1, 3)])
def test_reverse_mode_matches_central_differences(n, D, n_ell, k):
    X, a, ell, Z, Fb = _problem(n, D, n_ell, k)
    F, Zb, g = vr.vjp_reverse(X, a, ell, Z, Fb, 1e-6)
    cd = vr.central_diff(_sum_fbar_f(X, n_ell, Z, Fb, 1e-6), np.concatenate([[a], ell]))
    np.testing.assert_allclose(g, cd, rtol=1e-6, atol=1e-6 * np.abs(cd).max())
    K, _, _ = vr.se_cov(X, a, ell, 1e-6)
    L = np.linalg.cholesky(K)
    np.testing.assert_allclose(Zb, L.T @ Fb, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(F, L @ Z)


def test_longdouble_forward_mode_matches_reverse_and_central_differences():
    X, a, ell, Z, Fb = _problem(30, 2, 2, 2, seed=3)
    g_ld = vr.vjp_forward_longdouble(X, a, ell, Z, Fb, 1e-6).astype(float)
    _, _, g = vr.vjp_reverse(X, a, ell, Z, Fb, 1e-6)
    np.testing.assert_allclose(g, g_ld, rtol=1e-9, atol=1e-9 * np.abs(g_ld).max())
    cd = vr.central_diff(_sum_fbar_f(X, 2, Z, Fb, 1e-6), np.concatenate([[a], ell]))
    np.testing.assert_allclose(g_ld, cd, rtol=1e-6, atol=1e-6 * np.abs(cd).max())


def test_suffix_sum_form_of_V():
    X, a, ell, Z, Fb = _problem(37, 1, 1, 3, seed=5)
    K, _, _ = vr.se_cov(X, a, ell, 1e-6)
    L = np.linalg.cholesky(K)
    U = np.linalg.inv(L).T
    W = L.T @ Fb
    want = U @ vr.phi(W @ Z.T)
    np.testing.assert_allclose(vr.suffix_V(np.triu(U), W, Z), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_reference_configuration_longdouble_vs_float64():
    """x = linspace(0, 10, 100), alpha = 1, jitter 1e-10 (test_interpolate.R:31-36 / models/exact_gp.stan): cond(K) ~ 1e10,
    float64 reverse mode lands within 1e-4 of the longdouble forward mode."""
    x = np.linspace(0, 10, 100).reshape(-1, 1)
    rng = np.random.default_rng(11)
    z = rng.standard_normal((100, 1)); fb = rng.standard_normal((100, 1))
    for l in (0.5, 1.0):
        g_ld = vr.vjp_forward_longdouble(x, 1.0, [l], z, fb, 1e-10).astype(float)
        _, _, g = vr.vjp_reverse(x, 1.0, [l], z, fb, 1e-10)
        assert np.all(np.abs(g - g_ld) <= 1e-4 * np.abs(g_ld).max()), (l, g, g_ld)


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    from gp_amd import _lib
    for name in ("gpmi_exact_gp_f_vjp", "gpmi_exact_gp_f_vjp_dev", "gpmi_trmv_lower_t"):
        assert re.search(r"GPMI_API int %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS, name
    if os.path.exists(_lib.LIB_PATH):
        import subprocess
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        for name in ("gpmi_exact_gp_f_vjp", "gpmi_exact_gp_f_vjp_dev", "gpmi_trmv_lower_t"):
            assert re.search(r"\b%s\b" % name, syms), name
    assert 'exact_gp_f_vjp <- function(' in open(os.path.join(ROOT, "r", "gpmi.R")).read()
    from gp_amd import stan_models
    assert callable(stan_models.exact_gp_log_prob_grad)
