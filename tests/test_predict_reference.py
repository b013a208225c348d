"""CPU: the yardstick of gpmi_gp_predict / gpmi_seq_marginals (tests/predict_reference.py) -- the tie between the GPU parity
tests' two tolerances and the reference's own float64-vs-longdouble error, two identities that pin its formulas, and the new entry
points' presence in the header, the binding list and the host layers."""
import os
import re

import numpy as np
import pytest

import predict_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSUB = 300   # the longdouble reference is a Python loop: larger cases are judged on a seeded subsample of this size


def _case_inputs(n, D, m):
    X, y, Xs = pr.inputs(n, D, m)
    if n > NSUB:
        idx = np.sort(np.random.default_rng(n).choice(n, NSUB, replace=False))
        X, y = np.asfortranarray(X[idx]), y[idx]
    if m > 128:
        Xs = np.asfortranarray(Xs[:128])
    return X, y, Xs


@pytest.mark.parametrize("case", pr.parity_cases(), ids=lambda c: c[0])
def test_tolerances_stand_on_the_reference_own_error(case):
    """10 x the float64-vs-longdouble disagreement of the reference stays below MEAN_TOL / VAR_TOL on every parity case."""
    name, n, D, m, alpha, ell, sigma, jitter = case
    X, y, Xs = _case_inputs(n, D, m)
    mf, vf = pr.predict(X, y, Xs, alpha, ell, sigma, jitter, float)
    ml, vl = pr.predict(X, y, Xs, alpha, ell, sigma, jitter, np.longdouble)
    em = pr.max_rel(mf, ml.astype(float))
    ev = float(np.max(np.abs(vf - vl.astype(float)))) / alpha ** 2
    print("%s: mean %.2e var/alpha^2 %.2e" % (name, em, ev))
    assert 10 * em < pr.MEAN_TOL
    assert 10 * ev < pr.VAR_TOL
    assert np.all(vl > 0) and np.all(vl <= alpha ** 2)


def _sampler_inputs():
    """A sampler in the manner of tests/test_gpu_seq.py's ARD scenario: a jittered 7 x 7 x 6 grid of unit spacing under
    length-scales below one (K~ = K_XX + 1e-6 I stays well conditioned), Kn a noise floor plus a smooth low-rank part."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    X = np.asfortranarray(g + rng.uniform(-0.15, 0.15, g.shape))
    n = X.shape[0]
    A = rng.standard_normal((n, 8))
    Kn = 0.05 * np.eye(n) + 0.01 * (A @ A.T)
    mn = np.sin(X.sum(axis=1))
    Xs = np.asfortranarray(rng.uniform(0, 6, size=(64, 3)))
    return X, mn, Kn, Xs


def test_seq_marginals_tolerance_stands_on_the_reference_own_error():
    X, mn, Kn, Xs = _sampler_inputs()
    alpha, ell = 0.9, (0.7, 0.9, 0.6)
    mf, vf = pr.seq_marginals(X, mn, Kn, alpha, ell, 1e-6, Xs, float)
    ml, vl = pr.seq_marginals(X, mn, Kn, alpha, ell, 1e-6, Xs, np.longdouble)
    em = float(np.max(np.abs(mf - ml.astype(float)) / np.maximum(1.0, np.abs(ml.astype(float)))))
    ev = float(np.max(np.abs(vf - vl.astype(float)) / np.maximum(1.0, np.abs(vl.astype(float)))))
    print("seq_marginals: mean %.2e var %.2e" % (em, ev))
    # the GPU test holds gpmi_seq_marginals to 1e-8 max(1, |.|), the sampler's own tolerance
    assert 10 * em < 1e-8 and 10 * ev < 1e-8


def test_predict_is_mean_and_diagonal_of_the_full_posterior_1d():
    X, y, Xs = pr.inputs(60, 1, 25)
    alpha, ell, sigma, jitter = 1.3, (0.25,), 0.1, 1e-6
    mean, var = pr.predict(X, y, Xs, alpha, ell, sigma, jitter)
    S = pr.se_cov(X, X, alpha, ell) + (sigma ** 2 + jitter) * np.eye(60)
    Ks = pr.se_cov(Xs, X, alpha, ell)
    full = pr.se_cov(Xs, Xs, alpha, ell) - Ks @ np.linalg.solve(S, Ks.T)
    np.testing.assert_allclose(mean, Ks @ np.linalg.solve(S, y), rtol=0, atol=1e-10 * np.max(np.abs(mean)))
    np.testing.assert_allclose(var, np.diag(full), rtol=0, atol=1e-10 * alpha ** 2)


def test_seq_marginals_without_kn_is_predict():
    """Kn = 0 and mn = y: the sampler's marginals are predict's moments with sigma^2 + jitter folded into the sampler's jitter,
    up to the `+ jitter` on the variance."""
    X, y, Xs = pr.inputs(80, 2, 30)
    alpha, ell, sigma, jitter = 0.9, (0.3, 0.6), 0.1, 1e-6
    jit = sigma ** 2 + jitter
    ms, vs = pr.seq_marginals(X, y, np.zeros((80, 80)), alpha, ell, jit, Xs)
    mp, vp = pr.predict(X, y, Xs, alpha, ell, sigma, jitter)
    np.testing.assert_allclose(ms, mp, rtol=0, atol=1e-13 * np.max(np.abs(mp)))
    np.testing.assert_allclose(vs - jit, vp, rtol=0, atol=1e-13)


def test_lapack_form_agrees_with_the_loops():
    X, y, Xs = pr.inputs(200, 3, 50)
    a = pr.predict(X, y, Xs, 1.0, pr.ARD3, 0.1, 1e-6)
    b = pr.predict_lapack(X, y, Xs, 1.0, pr.ARD3, 0.1, 1e-6)
    assert pr.max_rel(a[0], b[0]) < 1e-12 and np.max(np.abs(a[1] - b[1])) < 1e-12


def test_entry_points_are_bound():
    """The three names are in the header and the binding list, and the host layers expose them."""
    names = ("gpmi_gp_predict", "gpmi_gp_predict_dev", "gpmi_seq_marginals")
    hdr = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    from gp_amd import _lib, ode_gp
    for nm in names:
        assert re.search(r"GPMI_API int %s\(" % nm, hdr), nm
        assert nm in _lib.SYMBOLS, nm
    assert callable(_lib.Context.gp_predict) and callable(_lib.Context.gp_predict_dev)
    assert callable(_lib.SeqSampler.marginals)
    assert callable(ode_gp.p_fXs)
    rsrc = open(os.path.join(ROOT, "r", "gpmi.R")).read()
    shim = open(os.path.join(ROOT, "r", "gpmi_shim.c")).read()
    for fn, call in (("gp_predict", "gpmi_R_gp_predict"), ("p_dotXnS_marginals", "gpmi_R_seq_marginals")):
        assert re.search(r"^%s <- function" % fn, rsrc, flags=re.M), fn
        assert '.Call("%s"' % call in rsrc and re.search(r"^SEXP %s\(" % call, shim, flags=re.M), call
