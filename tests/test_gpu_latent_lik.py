"""GPU: gpmi_latent_gp_lp_grad[_dev] -- forward product, likelihood head, its adjoint and the reverse sweep with one
factorisation -- against the float64 heads and models of tests/latent_lik_reference.py, gpmi_exact_gp_f / gpmi_exact_gp_f_vjp,
and itself across paths (one workgroup / blocked chain), calls and entry points; the model-level functions of
gp_amd.stan_models on top of it.  The tolerances of the parity test are tied to the reference's own error by
tests/test_latent_lik_reference.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import latent_lik_reference as lr
import vjp_reference as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_TOL = 1e-11    # of the sum of absolute terms: a fixed-order sum of <= n m terms of a few ulp each (n m eps = 1.3e-12 at most)
KEYS = ("F", "Fbar", "Zbar", "grad")


@pytest.fixture(scope="module")
def chain_ctx():
    """A second context whose VJP always takes the blocked chain."""
    import gp_amd
    c = gp_amd.Context(0)
    c.set_option("small_vjp", 0)
    yield c
    c.close()


def westbrook():
    with open(os.path.join(ROOT, "tests", "golden", "westbrook.json")) as f:
        w = json.load(f)
    return np.asarray(w["x"], float), np.asarray(w["made"], float)


def _call(c, family, case, **kw):
    X, a, ell, Z, Y, sg = case
    return c.latent_gp_lp_grad(X, a, ell, Z, family, Y, sg, lr.PARITY_JITTER, want_f=True, want_fbar=True, **kw)


def _same(r1, r2, keys=KEYS):
    assert r1["lik"] == r2["lik"] and r1["dlik_dsigma"] == r2["dlik_dsigma"]
    for key in keys:
        np.testing.assert_array_equal(r1[key], r2[key])


@pytest.mark.parametrize("family,n,D,ard,m", lr.parity_cases())
def test_parity(ctx, family, n, D, ard, m):
    case = lr.parity_case(family, n, D, ard, m)
    X, a, ell, Z, Y, sg = case
    k = lr.K_OF[family]
    r = _call(ctx, family, case)
    assert r["info"] == 0 and r["F"].shape == (n, k) and r["Fbar"].shape == (n, k) and r["Zbar"].shape == (n, k)
    assert r["grad"].shape == (1 + len(ell),)
    for c in range(k):   # every column is the value call's, bit for bit
        np.testing.assert_array_equal(r["F"][:, c], ctx.exact_gp_f(X, a, ell, Z[:, c], lr.PARITY_JITTER))
    # the head, in float64 on the F the call returned
    lik, ds, Fb, asum = lr.head(family, r["F"], Y, sg)
    fb_abs, ds_abs = lr.head_abs(family, r["F"], Y, sg)
    e_lik = abs(r["lik"] - lik) / asum
    e_ds = abs(r["dlik_dsigma"] - ds) / ds_abs if ds_abs else abs(r["dlik_dsigma"])
    e_fb = float(np.max(np.abs(r["Fbar"] - Fb) / fb_abs))
    # the sweep, against float64 reverse mode on the reference's own F and head adjoint
    ref = lr.lp_grad_reference(family, X, a, ell, Z, Y, sg, lr.PARITY_JITTER)
    e_zb, e_g = lr.rel(r["Zbar"], ref["Zbar"]), lr.rel(r["grad"], ref["grad"])
    print("%s n=%d D=%d ard=%d m=%d: lik %.1e dsig %.1e Fbar %.1e Zbar %.1e grad %.1e" % (family, n, D, ard, m, e_lik, e_ds, e_fb, e_zb, e_g))
    assert e_lik <= HEAD_TOL and e_ds <= HEAD_TOL and e_fb <= HEAD_TOL
    assert e_zb <= lr.ZBAR_TOL and e_g <= lr.GRAD_TOL
    if family != "normal":
        assert r["dlik_dsigma"] == 0.0


@pytest.mark.parametrize("family,n", [(f, n) for f in lr.FAMILIES for n in (100, 256, 300, 700)])
def test_sweep_is_the_plain_vjp_on_the_returned_fbar(ctx, family, n):
    """Feeding the returned Fbar to gpmi_exact_gp_f_vjp on the same path reproduces Zbar and grad bit for bit: on the chain the
    launches are the same, on the one-workgroup path the two kernels are instances of one body."""
    case = lr.parity_case(family, n, 2, True, 5)
    X, a, ell, Z, Y, sg = case
    r = _call(ctx, family, case)
    F, Zb, g = ctx.exact_gp_f_vjp(X, a, ell, Z, r["Fbar"], lr.PARITY_JITTER)
    np.testing.assert_array_equal(F, r["F"])
    np.testing.assert_array_equal(Zb, r["Zbar"])
    np.testing.assert_array_equal(g, r["grad"])


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("n", [100, 256])
def test_one_workgroup_and_chain_agree(ctx, chain_ctx, family, n):
    """The bounds and the problem layout of tests/test_gpu_exact_gp_vjp.py::test_one_workgroup_and_chain_agree (see
    latent_lik_reference.path_case for why the layout belongs to the bounds)."""
    case = lr.path_case(family, n)
    r1 = _call(ctx, family, case)
    r2 = _call(chain_ctx, family, case)
    asum = lr.head(family, r1["F"], case[4], case[5])[3]
    e = (abs(r1["lik"] - r2["lik"]) / asum, lr.rel(r2["Zbar"], r1["Zbar"]), lr.rel(r2["grad"], r1["grad"]))
    print("%s n=%d one workgroup vs chain: lik %.1e Zbar %.1e grad %.1e" % ((family, n) + e))
    assert e[0] <= 1e-12 and e[1] <= 1e-12 and e[2] <= 1e-11, e


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("n", [100, 700])
def test_repeated_calls_bit_identical(ctx, chain_ctx, family, n):
    case = lr.parity_case(family, n, 1, False, 5)
    for c in (ctx, chain_ctx):
        r1 = _call(c, family, case)
        other = lr.parity_case(family, n, 1, False, 5, seed=1)
        _call(c, family, other)                      # something else in between: nothing of it may linger
        _same(r1, _call(c, family, case))


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("n", [100, 700])
def test_dev_equals_host(ctx, family, n):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    m, D = 5, 2
    case = lr.parity_case(family, n, D, False, m)
    X, a, ell, Z, Y, sg = case
    k = lr.K_OF[family]
    r = _call(ctx, family, case)
    up = lambda A: torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)      # (cols, n) row-major == n x cols column-major
    dX, dZ, dY = up(X), up(Z), up(Y)
    for with_opt in (True, False):
        dF = torch.zeros((k, n), dtype=torch.float64, device=dev); dFb = torch.zeros_like(dF); dZb = torch.zeros_like(dF)
        dg = torch.zeros(1 + len(ell), dtype=torch.float64, device=dev); dout = torch.zeros(2, dtype=torch.float64, device=dev)
        info = torch.full((1,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.latent_gp_lp_grad_dev(dX.data_ptr(), n, n, D, a, ell, lr.PARITY_JITTER, dZ.data_ptr(), k, n, family, dY.data_ptr(), m, n, sg,
                                  dout.data_ptr(), dF.data_ptr() if with_opt else None, n, dFb.data_ptr() if with_opt else None, n,
                                  dZb.data_ptr(), n, dg.data_ptr(), info.data_ptr())
        ctx.sync()
        assert int(info.item()) == 0
        o = dout.cpu().numpy()
        assert o[0] == r["lik"] and o[1] == r["dlik_dsigma"]
        np.testing.assert_array_equal(dZb.cpu().numpy().T, r["Zbar"])
        np.testing.assert_array_equal(dg.cpu().numpy(), r["grad"])
        if with_opt:
            np.testing.assert_array_equal(dF.cpu().numpy().T, r["F"])
            np.testing.assert_array_equal(dFb.cpu().numpy().T, r["Fbar"])
    # ... and the host form without F and Fbar
    X, a, ell, Z, Y, sg = case
    r0 = ctx.latent_gp_lp_grad(X, a, ell, Z, family, Y, sg, lr.PARITY_JITTER, want_f=False, want_fbar=False)
    assert r0["F"] is None and r0["Fbar"] is None
    _same(r, r0, keys=("Zbar", "grad"))


@pytest.mark.parametrize("n", [100, 700])
def test_bernoulli_stays_finite_for_huge_latents(ctx, n):
    m = 5
    X, a, ell, Z, Y, _ = lr.parity_case("bernoulli_logit", n, 1, False, m)
    f0 = ctx.exact_gp_f(X, a, ell, Z[:, 0], lr.PARITY_JITTER)
    Z = Z * (900.0 / np.max(np.abs(f0)))
    r = ctx.latent_gp_lp_grad(X, a, ell, Z, "bernoulli_logit", Y, None, lr.PARITY_JITTER, want_f=True, want_fbar=True)
    assert np.max(np.abs(r["F"])) > 700.0
    assert math.isfinite(r["lik"]) and np.all(np.isfinite(r["Fbar"])) and np.all(np.isfinite(r["Zbar"])) and np.all(np.isfinite(r["grad"]))
    assert np.all(np.abs(r["Fbar"]) <= m)
    lik, _, Fb, asum = lr.head("bernoulli_logit", r["F"], Y)
    assert abs(r["lik"] - lik) <= HEAD_TOL * asum
    assert np.max(np.abs(r["Fbar"] - Fb)) <= HEAD_TOL * 2 * m


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("n", [50, 300])
def test_not_positive_definite(ctx, family, n):
    from gp_amd._lib import NotPositiveDefinite
    k = lr.K_OF[family]
    X = np.ones((n, 1)); Z = np.ones((n, k)); Y = np.ones((n, 2))
    sg = 1.0 if family == "normal" else None
    with pytest.raises(NotPositiveDefinite):
        ctx.latent_gp_lp_grad(X, 1.0, [1.0], Z, family, Y, sg, 0.0)
    r = ctx.latent_gp_lp_grad(X, 1.0, [1.0], Z, family, Y, sg, 0.0, want_f=True, want_fbar=True, raise_not_pd=False)
    assert 1 < r["info"] <= n
    assert math.isnan(r["lik"]) and math.isnan(r["dlik_dsigma"])
    for key in KEYS:
        assert np.all(np.isnan(r[key])), key
    # the context is usable afterwards
    case = lr.parity_case(family, n, 1, False, 1)
    assert _call(ctx, family, case)["info"] == 0


def test_bad_arguments(ctx):
    from gp_amd._lib import _p
    n = 10
    X = np.asfortranarray(np.linspace(0, 3, n).reshape(-1, 1)); Z = np.ones((n, 2), order="F"); Y = np.ones((n, 3), order="F")
    Zb = np.zeros((n, 2), order="F"); g = np.zeros(2); e = np.ones(1); out = np.zeros(2)
    lib, h = ctx._lib, ctx._h
    d = C.c_double

    def call(family=0, k=1, m=3, ldy=n, sigma=1.0, Yp=Y, n_=n, ldz=n, ldzb=n, alpha=1.0):
        return lib.gpmi_latent_gp_lp_grad(h, _p(X), n_, n, 1, d(alpha), _p(e), 1, d(1e-6), _p(Z), k, ldz, family, _p(Yp), m, ldy, d(sigma),
                                          _p(out), None, n, None, n, _p(Zb), ldzb, _p(g))
    assert call() == 0 and call(family=1) == 0 and call(family=2, k=2) == 0
    Yhalf = Y.copy(order="F"); Yhalf[3, 1] = 0.5
    for kw in ({"k": 2}, {"k": 0}, {"family": 1, "k": 2}, {"family": 2, "k": 1}, {"family": 2, "k": 3}, {"m": 0}, {"ldy": n - 1},
               {"sigma": 0.0}, {"sigma": -1.0}, {"sigma": math.nan}, {"family": 3}, {"family": -1}, {"family": 1, "Yp": Yhalf},
               {"n_": 0}, {"ldz": n - 1}, {"ldzb": n - 1}, {"alpha": 0.0}):
        assert call(**kw) == -1, kw
    assert call(family=2, k=2, sigma=-1.0) == 0 and call(family=1, sigma=0.0) == 0      # sigma is ignored there
    assert call(family=0, Yp=Yhalf) == 0
    assert lib.gpmi_latent_gp_lp_grad(h, _p(X), n, n, 1, d(1.0), _p(e), 1, d(1e-6), _p(Z), 1, n, 0, None, 3, n, d(1.0), _p(out), None, n,
                                      None, n, _p(Zb), n, _p(g)) == -1
    with pytest.raises(Exception):
        ctx.latent_gp_lp_grad(X, 1.0, e, Z[:, 0], "poisson", Y, 1.0)


@pytest.mark.parametrize("l", [0.1, 0.3])
def test_westbrook_fixture_against_the_reference_model(ctx, l):
    """The whole fixture (N = 1438, the blocked chain), sigma = 1, jitter 1e-6 (the reference's own error at the model's 1e-12 is
    1e-5: see the issue's numbers in DESIGN.md)."""
    from gp_amd import stan_models
    x, y = westbrook()
    n = x.size
    z = np.random.default_rng(int(100 * l)).standard_normal(n)
    lp, g = stan_models.westbrook_exact_log_prob_grad(x, y, z, 1.0, l, ctx=ctx, jitter=1e-6)
    want, gw = lr.westbrook_exact_lp_grad(x, y, z, 1.0, l, jitter=1e-6)
    e_lp = abs(lp - want) / abs(want)
    e_z = np.max(np.abs(g[:n] - gw[:n])) / np.max(np.abs(gw[:n] + z))      # relative to Zbar, as the parity test
    e_t = lr.rel(g[n:] , gw[n:])
    print("westbrook l=%g: lp %.1e z-gradient %.1e (sigma, l)-gradient %.1e" % (l, e_lp, e_z, e_t))
    assert e_lp <= 1e-9 and e_z <= lr.ZBAR_TOL and e_t <= lr.GRAD_TOL


def test_westbrook_at_the_models_own_jitter(ctx):
    """jitter 1e-12, cond(K) about 6e13: either the proposal is rejected, (-inf, NaN), or the result is finite and Zbar is
    tril(L)^T Fbar for the device's own factor L.  No accuracy claim against longdouble here."""
    from gp_amd import stan_models
    x, y = westbrook()
    n = x.size
    z = np.random.default_rng(3).standard_normal(n)
    lp, g = stan_models.westbrook_exact_log_prob_grad(x, y, z, 1.0, 0.1, ctx=ctx)
    if lp == -math.inf:
        assert np.all(np.isnan(g))
        print("westbrook at jitter 1e-12: not positive definite on the device")
        return
    assert math.isfinite(lp) and np.all(np.isfinite(g))
    r = ctx.latent_gp_lp_grad(x, 1.0, [0.1], z, "bernoulli_logit", y, None, 1e-12, want_f=True, want_fbar=True)
    Ld = np.tril(ctx.potrf(ctx.se_cov(x.reshape(-1, 1), None, 1.0, [0.1], diag_add=1e-12)))
    e = lr.rel(r["Zbar"], Ld.T @ r["Fbar"])
    print("westbrook at jitter 1e-12: finite, Zbar vs tril(L_dev)^T Fbar %.1e" % e)
    assert e <= 1e-12


def _cd_check(fun, theta, got, rtol=1e-6):
    cd = vr.central_diff(fun, theta, h_rel=1e-6)
    np.testing.assert_allclose(got, cd, rtol=rtol, atol=rtol * np.abs(cd).max())


# N = 100 on linspace(0, 10) with l = 0.15: cond(K) = 2.6e4, so that float64 references are good to 1e-11 and the 1e-9 bound on
# lp__ (that of test_exact_gp_log_prob_grad) tests the library, not LAPACK's factor
def test_heteroscedastic_log_prob_grad(ctx):
    from gp_amd import stan_models
    rng = np.random.default_rng(21)
    n, M = 100, 5
    x = np.linspace(0, 10, n)
    Y = np.sin(x)[:, None] + 0.3 * rng.standard_normal((n, M))
    z1 = rng.standard_normal(n); z2 = 0.3 * rng.standard_normal(n)
    l, sf = 0.15, 1.1
    lp, g = stan_models.heteroscedastic_log_prob_grad(x, Y, l, sf, z1, z2, ctx=ctx)
    want, gw = lr.heteroscedastic_lp_grad(x, Y, l, sf, z1, z2)
    assert abs(lp - want) <= 1e-9 * abs(want)
    assert g.shape == (2 + 2 * n,) and lr.rel(g, gw) <= lr.GRAD_TOL

    def at(t):
        a = z1.copy(); b = z2.copy(); a[[0, 57]] = t[2:4]; b[[3, 99]] = t[4:]
        return stan_models.heteroscedastic_log_prob_grad(x, Y, t[0], t[1], a, b, ctx=ctx)[0]
    _cd_check(at, np.array([l, sf, z1[0], z1[57], z2[3], z2[99]]), np.array([g[0], g[1], g[2], g[59], g[2 + n + 3], g[2 + n + 99]]))


def test_fit_full_gp_log_prob_grad(ctx):
    from gp_amd import stan_models
    rng = np.random.default_rng(22)
    n = 100
    x = np.linspace(0, 10, n)
    y = np.sin(x) + 0.1 * rng.standard_normal(n)
    zn = rng.standard_normal(n)
    l, al, sg = 0.15, 1.2, 0.4
    lp, g = stan_models.fit_full_gp_log_prob_grad(x, y, l, al, sg, zn, ctx=ctx)
    want, gw = lr.fit_full_gp_lp_grad(x, y, l, al, sg, zn)
    assert abs(lp - want) <= 1e-9 * abs(want)
    assert g.shape == (3 + n,) and lr.rel(g, gw) <= lr.GRAD_TOL

    def at(t):
        a = zn.copy(); a[[0, 41, 99]] = t[3:]
        return stan_models.fit_full_gp_log_prob_grad(x, y, t[0], t[1], t[2], a, ctx=ctx)[0]
    _cd_check(at, np.array([l, al, sg, zn[0], zn[41], zn[99]]), np.array([g[0], g[1], g[2], g[3], g[44], g[102]]))


def test_exact_gp_log_prob_grad_fused(ctx):
    from gp_amd import stan_models
    rng = np.random.default_rng(23)
    n = 100
    x = np.linspace(0, 10, n)
    y = np.sin(x) + 0.1 * rng.standard_normal(n)
    z = rng.standard_normal(n)
    l, s = 0.15, 0.3
    lp, g = stan_models.exact_gp_log_prob_grad(x, y, l, s, z, ctx=ctx, fused=True)
    lp0, g0 = stan_models.exact_gp_log_prob_grad(x, y, l, s, z, ctx=ctx)
    want = vr.exact_gp_lp(x, y, l, s, z)
    assert abs(lp - want) <= 1e-9 * abs(want) and abs(lp - lp0) <= 1e-9 * abs(lp0)
    assert g.shape == (2 + n,) and lr.rel(g, g0) <= lr.GRAD_TOL

    def at(t):
        zz = z.copy(); zz[[0, 7, 99]] = t[2:]
        return stan_models.exact_gp_log_prob_grad(x, y, t[0], t[1], zz, ctx=ctx, fused=True)[0]
    _cd_check(at, np.array([l, s, z[0], z[7], z[99]]), np.array([g[0], g[1], g[2], g[9], g[101]]))


def test_rejected_proposal(ctx):
    """Not positive definite (duplicate points, no jitter): (-inf, NaN), as exact_gp_log_prob_grad."""
    from gp_amd import stan_models
    n = 40
    lp, g = stan_models.westbrook_exact_log_prob_grad(np.ones(n), np.ones(n), np.ones(n), 1.0, 0.1, ctx=ctx, jitter=0.0)
    assert lp == -math.inf and g.shape == (n + 2,) and np.all(np.isnan(g))
