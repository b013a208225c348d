"""CPU: the yardsticks of gpmi_latent_gp_lp_grad (tests/latent_lik_reference.py) pinned by central differences, the tie between
the GPU parity test's tolerances and the reference's own error, the resource usage of the chain's head kernels, and the new entry points'
presence in the header, the binding list, the built library and the R wrapper."""
import json
import os
import re

import numpy as np
import pytest

from kernel_resources import resource_usage
import latent_lik_reference as lr
import vjp_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def westbrook():
    with open(os.path.join(ROOT, "tests", "golden", "westbrook.json")) as f:
        w = json.load(f)
    return np.asarray(w["x"], float), np.asarray(w["made"], float)


def test_westbrook_fixture():
    x, y = westbrook()
    assert x.size == 1438 and y.size == 1438
    assert set(np.unique(y)) == {0.0, 1.0} and int(y.sum()) == 613
    assert np.all(np.abs(x) <= 0.5)


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("m", [1, 5])
def test_head_adjoints_match_central_differences(family, m):
    rng = np.random.default_rng(3 + m)
    n, k = 17, lr.K_OF[family]
    F = rng.standard_normal((n, k)) * (0.5 if family == "normal_logsd" else 2.0)
    Y = (rng.uniform(size=(n, m)) < 0.5).astype(float) if family == "bernoulli_logit" else rng.standard_normal((n, m))
    sigma = 0.8 if family == "normal" else None
    lik, ds, Fb, asum = lr.head(family, F, Y, sigma)
    assert Fb.shape == (n, k) and asum >= abs(lik)
    cd = vr.central_diff(lambda f: lr.lik_of_F(family, f.reshape(n, k, order="F"), Y, sigma), F.ravel(order="F"))
    np.testing.assert_allclose(Fb.ravel(order="F"), cd, rtol=1e-7, atol=1e-7 * np.abs(cd).max())
    if family == "normal":
        cds = vr.central_diff(lambda s: lr.lik_of_F(family, F, Y, s[0]), np.array([sigma]))
        np.testing.assert_allclose(ds, cds[0], rtol=1e-7)
    else:
        assert ds == 0.0
    # float64 against longdouble: the head itself is accurate to a few ulp of the sum of its absolute terms
    likl, dsl, Fbl, _ = lr.head(family, F, Y, sigma, dtype=np.longdouble)
    assert abs(float(likl) - lik) <= 1e-14 * asum
    assert lr.rel(Fb, Fbl.astype(float)) <= 1e-14


def test_bernoulli_head_is_finite_for_large_latents():
    F = np.array([[-800.0], [-40.0], [0.0], [40.0], [800.0]])
    Y = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]])
    lik, _, Fb, _ = lr.head("bernoulli_logit", F, Y)
    assert np.isfinite(lik) and np.all(np.isfinite(Fb)) and np.all(np.abs(Fb) <= 2.0)
    assert Fb[0, 0] == 1.0 and Fb[4, 0] == 0.0


def _fd_model(lp, theta, grad, rtol=2e-6):
    cd = vr.central_diff(lp, theta, h_rel=1e-6)
    np.testing.assert_allclose(grad, cd, rtol=rtol, atol=rtol * np.abs(cd).max())


def test_westbrook_exact_model_gradient_by_central_differences():
    x, y = westbrook()
    idx = np.sort(np.random.default_rng(5).choice(x.size, 30, replace=False))
    x, y = x[idx], y[idx]
    z = np.random.default_rng(6).standard_normal(30)
    lp, g = lr.westbrook_exact_lp_grad(x, y, z, 1.1, 0.2, jitter=1e-6)
    _fd_model(lambda t: lr.westbrook_exact_lp(x, y, t[:30], t[30], t[31], jitter=1e-6), np.concatenate([z, [1.1, 0.2]]), g)
    assert np.isfinite(lp)


def test_heteroscedastic_model_gradient_by_central_differences():
    rng = np.random.default_rng(7)
    n, M = 10, 5                                   # the size heteroscedastic.R runs
    x = np.linspace(0.0, 3.0, n) + 0.05 * rng.standard_normal(n)     # spaced: the model's jitter is 1e-9
    Y = rng.standard_normal((n, M))
    z1 = rng.standard_normal(n); z2 = 0.3 * rng.standard_normal(n)
    lp, g = lr.heteroscedastic_lp_grad(x, Y, 0.5, 1.0, z1, z2)
    _fd_model(lambda t: lr.heteroscedastic_lp(x, Y, t[0], t[1], t[2:2 + n], t[2 + n:]), np.concatenate([[0.5, 1.0], z1, z2]), g)


def test_fit_full_gp_model_gradient_by_central_differences():
    rng = np.random.default_rng(8)
    n = 20
    x = np.linspace(0.0, 10.0, n)
    y = np.sin(x) + 0.1 * rng.standard_normal(n)
    zn = rng.standard_normal(n)
    lp, g = lr.fit_full_gp_lp_grad(x, y, 0.6, 1.2, 0.4, zn)
    _fd_model(lambda t: lr.fit_full_gp_lp(x, y, t[0], t[1], t[2], t[3:]), np.concatenate([[0.6, 1.2, 0.4], zn]), g)


def _d_ref(family, X, alpha, ell, Z, Y, sigma, jitter):
    """Disagreement of float64 reverse mode and longdouble forward mode on the same head adjoint."""
    r = lr.lp_grad_reference(family, X, alpha, ell, Z, Y, sigma, jitter)
    gl = vr.vjp_forward_longdouble(X, alpha, ell, Z, r["Fbar"], jitter)
    return lr.rel(r["grad"], gl.astype(float))


def test_gpu_tolerances_follow_from_the_reference():
    """For every configuration of the GPU parity test: 10 d_ref <= the gradient tolerance that test uses, d_ref the disagreement
    between vjp_reverse (float64) and vjp_forward_longdouble.  Full size up to n = 300; above, a seeded 300-point subsample (the
    longdouble loops are cubic in Python)."""
    worst = 0.0
    for family, n, D, ard, m in lr.parity_cases():
        X, a, ell, Z, Y, sg = lr.parity_case(family, n, D, ard, m)
        if n > 300:
            idx = np.sort(np.random.default_rng(n).choice(n, 300, replace=False))
            X, Z, Y = X[idx], Z[idx], Y[idx]
        d = _d_ref(family, X, a, ell, Z, Y, sg, lr.PARITY_JITTER)
        worst = max(worst, d)
        assert 10.0 * d <= lr.GRAD_TOL, (family, n, D, ard, m, d)
    print("worst d_ref over the parity cases: %.2e" % worst)


@pytest.mark.parametrize("l", [0.1, 0.3])
def test_westbrook_tolerance_follows_from_the_reference(l):
    """The Westbrook fixture at jitter 1e-6 (the GPU test's setting), a seeded 200-point subsample."""
    x, y = westbrook()
    idx = np.sort(np.random.default_rng(11).choice(x.size, 200, replace=False))
    z = np.random.default_rng(12).standard_normal(200)
    d = _d_ref("bernoulli_logit", x[idx].reshape(-1, 1), 1.0, [l], z.reshape(-1, 1), y[idx].reshape(-1, 1), None, 1e-6)
    print("westbrook subsample l=%g d_ref %.2e" % (l, d))
    assert 10.0 * d <= lr.GRAD_TOL, d


def test_chain_head_kernels_do_not_spill():
    """The head kernels of the blocked chain keep their state in registers and LDS: 0 VGPRs spilled, 0 bytes of scratch."""
    from gp_amd import _build
    kernels = resource_usage(os.path.join(_build.CSRC, "latent_kernels.hip"), "latent_kernels.o")
    for must in ("k_latent_head", "k_latent_head_sum"):
        assert any(must in k for k in kernels), (must, list(kernels))
    for k, v in kernels.items():
        assert v.get("VGPRs Spill") == 0, (k, v)
        assert v.get("ScratchSize [bytes/lane]") == 0, (k, v)


def test_entry_points_are_declared_bound_and_built():
    import ctypes
    from gp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"#define GPMI_VERSION 302\b", hdr)
    assert re.search(r"GPMI_LIK_NORMAL = 0, GPMI_LIK_BERNOULLI_LOGIT = 1, GPMI_LIK_NORMAL_LOGSD = 2", hdr)
    for name in ("gpmi_latent_gp_lp_grad", "gpmi_latent_gp_lp_grad_dev"):
        assert re.search(r"GPMI_API int %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS
    assert _lib.LIK_FAMILIES == {"normal": 0, "bernoulli_logit": 1, "normal_logsd": 2}
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in ("gpmi_latent_gp_lp_grad", "gpmi_latent_gp_lp_grad_dev"):
            getattr(lib, name)
    assert "latent_gp_lp_grad <- function(" in open(os.path.join(ROOT, "r", "gpmi.R")).read()
    assert "gpmi_R_latent_gp_lp_grad" in open(os.path.join(ROOT, "r", "gpmi_shim.c")).read()
    from gp_amd import stan_models
    for f in ("westbrook_exact_log_prob_grad", "heteroscedastic_log_prob_grad", "fit_full_gp_log_prob_grad"):
        assert callable(getattr(stan_models, f))
