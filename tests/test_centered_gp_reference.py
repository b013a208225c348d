"""CPU: the yardsticks of gpmi_centered_gp_lp_grad (tests/centered_gp_reference.py) pinned by central differences, the
condition on the parity inputs that the GPU test's bounds rest on (cond_2(Sigma) and the float64 reference's own error against
long double), and the new entry points' presence in the header, the binding list, the built library and the R wrapper."""
import os
import re
import subprocess

import numpy as np
import pytest

import centered_gp_reference as cr
import vjp_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(family, n, D, n_ell, k, m=3, seed=0):
    rng = np.random.default_rng(50 * n + 7 * D + n_ell + k + seed)
    ell = 0.6 + 0.4 * rng.random(n_ell)
    X = rng.random((n, D)) * (float(ell.mean()) * n ** (1.0 / D))
    k = cr.k_of(family, k)
    K, _, _ = vr.se_cov(X, 1.3, ell, 1e-6)
    F = np.linalg.cholesky(K) @ rng.standard_normal((n, k))
    if family == "normal_logsd":
        F[:, 1] *= 0.5
    Y = None if family == "none" else ((rng.uniform(size=(n, m)) < 0.4).astype(float) if family == "bernoulli_logit"
                                       else rng.standard_normal((n, m)))
    return X, 1.3, ell, F, Y, (0.7 if family == "normal" else None)


@pytest.mark.parametrize("family,n,D,n_ell,k", [("none", 12, 1, 1, 1), ("none", 30, 2, 2, 3), ("none", 40, 3, 1, 8), ("normal", 25, 2, 1, 1),
                                                ("bernoulli_logit", 40, 1, 1, 1), ("normal_logsd", 10, 1, 1, 2),
                                                ("normal_logsd", 33, 3, 3, 2)])
def test_reference_gradients_match_central_differences(family, n, D, n_ell, k):
    """Fgrad and grad of the float64 reference against central differences of out[0]: 1e-6 relative at n <= 40, the bound of
    test_exact_gp_vjp_reference.py::test_reverse_mode_matches_central_differences."""
    X, a, ell, F, Y, sg = _problem(family, n, D, n_ell, k)
    k = F.shape[1]
    r = cr.centered_reference(X, a, ell, F, family, Y, sg, 1e-6)
    assert r["Fgrad"].shape == (n, k) and r["grad"].shape == (1 + n_ell,)
    assert abs(float(r["prior"]) - (-0.5 * float(r["quad"]) - k * float(r["sum_log_diag"]))) <= 1e-13 * abs(float(r["prior"]))
    cd_t = vr.central_diff(lambda t: cr.prior_lp(X, t[0], t[1:], F, family, Y, sg, 1e-6), np.concatenate([[a], ell]))
    np.testing.assert_allclose(r["grad"], cd_t, rtol=1e-6, atol=1e-6 * np.abs(cd_t).max())
    cd_f = vr.central_diff(lambda f: cr.prior_lp(X, a, ell, f.reshape(n, k, order="F"), family, Y, sg, 1e-6), F.ravel(order="F"))
    np.testing.assert_allclose(r["Fgrad"].ravel(order="F"), cd_f, rtol=1e-6, atol=1e-6 * np.abs(cd_f).max())
    if family == "normal":
        cd_s = vr.central_diff(lambda s: cr.prior_lp(X, a, ell, F, family, Y, s[0], 1e-6), np.array([sg]))
        np.testing.assert_allclose(r["dlik_dsigma"], cd_s[0], rtol=1e-6)
    # the long-double loops state the same function
    rl = cr.centered_reference(X, a, ell, F, family, Y, sg, 1e-6, dtype=np.longdouble)
    e = cr.reference_errors(r, rl)
    assert max(e["sum_log_diag"], e["quad"], e["prior"], e["Fgrad"], e["grad"]) <= 1e-9, e


def test_model_gradient_matches_central_differences():
    rng = np.random.default_rng(7)
    n, M = 10, 5                                   # the size heteroscedastic.R runs
    x = np.linspace(0.0, 3.0, n) + 0.05 * rng.standard_normal(n)     # spaced: the model's jitter is 1e-9
    Y = rng.standard_normal((n, M))
    mu = rng.standard_normal(n); s = 0.2 + rng.random(n)             # vector<lower=0> sigma_log
    lp, g = cr.heteroscedastic_centered_lp_grad(x, Y, 0.5, 1.0, mu, s)
    assert np.isfinite(lp) and g.shape == (2 + 2 * n,)
    cd = vr.central_diff(lambda t: float(cr.heteroscedastic_centered_lp(x, Y, t[0], t[1], t[2:2 + n], t[2 + n:])),
                         np.concatenate([[0.5, 1.0], mu, s]), h_rel=1e-6)
    np.testing.assert_allclose(g, cd, rtol=2e-6, atol=2e-6 * np.abs(cd).max())


@pytest.mark.parametrize("n", [10, 100])
def test_model_cases_reference_error(n):
    """The model-level GPU test compares at the model's own jitter 1e-9, where cond_2(Sigma) is far higher than on the parity
    inputs; its bound is 10 cond eps for that case's cond, and here the float64 reference stays under 1 cond eps."""
    x, Y, l, sf, mu, s = cr.model_case(n)
    lp, g = cr.heteroscedastic_centered_lp_grad(x, Y, l, sf, mu, s)
    e_lp, e_g, cond = cr.model_errors(lp, g, x, Y, l, sf, mu, s)
    print("model N=%d: cond %.1e, float64 vs long double in cond eps: lp %.3f gradient %.3f" % (n, cond, e_lp / (cond * cr.EPS),
                                                                                             e_g / (cond * cr.EPS)))
    assert e_lp <= cond * cr.EPS and e_g <= cond * cr.EPS


def test_parity_cases_cover_what_the_issue_asks():
    cases = cr.parity_cases()
    assert len(set(cases)) == len(cases)
    for family in cr.FAMILIES:
        mine = [c for c in cases if c[0] == family]
        assert {c[1] for c in mine} == set(cr.PARITY_SIZES)
        assert {c[2] for c in mine} == {1, 2, 3} and {c[3] for c in mine} == {False, True} and {c[4] for c in mine} == {1, 5}
        for lo, hi in ((1, 256), (257, 10 ** 6)):     # both paths
            assert any(lo <= c[1] <= hi for c in mine)
    assert {c[5] for c in cases if c[0] == "none"} == set(cr.NONE_K)
    for path in ((1, 256), (257, 10 ** 6)):
        assert {c[5] for c in cases if c[0] == "none" and path[0] <= c[1] <= path[1]} == set(cr.NONE_K)


@pytest.mark.parametrize("case", cr.parity_cases(), ids=lambda c: "%s-n%d-D%d-ard%d-m%d-k%d" % c)
def test_parity_inputs_are_well_conditioned_and_the_reference_is_good(case):
    """A condition on the inputs of the GPU parity test, not a measurement: cond_2(Sigma) <= 2e7 and the float64 reference's own
    error against long double <= 1 cond_2(Sigma) eps -- for out[2], out[3] and prior (relative), Fgrad (max norm relative to
    max|Fgrad|) and grad (max norm relative to max|grad|).  The GPU test allows the device ten times that."""
    inp, ref, cond = cr.parity_reference(case)
    X, a, ell, F, Y, sg = inp
    assert cond <= cr.COND_MAX, cond
    e = cr.reference_errors(cr.centered_reference(X, a, ell, F, case[0], Y, sg, cr.PARITY_JITTER), ref)
    ce = cond * cr.EPS
    print("%s: cond %.1e, float64 vs long double in cond eps: sum_log %.3f quad %.3f prior %.3f Fgrad %.3f grad %.3f" % (
        case, cond, e["sum_log_diag"] / ce, e["quad"] / ce, e["prior"] / ce, e["Fgrad"] / ce, e["grad"] / ce))
    for key in ("sum_log_diag", "quad", "prior", "Fgrad", "grad"):
        assert e[key] <= ce, (key, e[key] / ce)


def test_entry_points_are_declared_bound_and_built():
    from gp_amd import _lib, stan_models
    hdr = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"#define GPMI_VERSION 302\b", hdr)
    assert re.search(r"GPMI_LIK_NONE = 3\b", hdr)
    names = ("gpmi_centered_gp_lp_grad", "gpmi_centered_gp_lp_grad_dev")
    for name in names:
        assert re.search(r"GPMI_API int %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS, name
    assert _lib.lik_family("none") == 3
    if os.path.exists(_lib.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        for name in names:
            assert re.search(r"\b%s\b" % name, syms), name
    assert "centered_gp_lp_grad <- function(" in open(os.path.join(ROOT, "r", "gpmi.R")).read()
    assert "gpmi_R_centered_gp_lp_grad" in open(os.path.join(ROOT, "r", "gpmi_shim.c")).read()
    assert callable(stan_models.heteroscedastic_centered_log_prob_grad)
    assert callable(_lib.Context.centered_gp_lp_grad) and callable(_lib.Context.centered_gp_lp_grad_dev)
