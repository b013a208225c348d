"""GPU: the vector-Jacobian product of the latent exact GP's transform (gpmi_exact_gp_f_vjp[_dev], gpmi_trmv_lower_t) against
the CPU references of tests/vjp_reference.py, central differences of gpmi_exact_gp_f, the library's forward-mode tangent
(gpmi_rbf_cov_chol), and itself across paths (one workgroup / blocked chain), calls and entry points."""
import ctypes as C
import math

import numpy as np
import pytest

import vjp_reference as vr

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 1), (30, 1, 1, 1), (100, 3, 3, 2), (256, 2, 1, 2), (257, 2, 2, 1), (700, 1, 1, 3), (1500, 9, 9, 1),
         (4096, 3, 1, 1)]


@pytest.fixture(scope="module")
def chain_ctx():
    """A second context whose VJP always takes the blocked chain."""
    import gp_amd
    c = gp_amd.Context(0)
    c.set_option("small_vjp", 0)
    yield c
    c.close()


def _problem(n, D, n_ell, k, seed):
    rng = np.random.default_rng(seed)
    ell = 0.6 + 0.4 * rng.random(n_ell)
    X = rng.random((n, D)) * (ell.mean() * n ** (1.0 / D))     # about one point per length-scale
    return X, 1.3, ell, rng.standard_normal((n, k)), rng.standard_normal((n, k))


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("n,D,n_ell,k", CASES)
def test_parity_well_conditioned(ctx, n, D, n_ell, k):
    X, a, ell, Z, Fb = _problem(n, D, n_ell, k, seed=n + 7 * D)
    jit = 1e-6
    F, Zb, g = ctx.exact_gp_f_vjp(X, a, ell, Z, Fb, jit)
    assert F.shape == (n, k) and Zb.shape == (n, k) and g.shape == (1 + n_ell,)
    for c in range(k):   # every column is the value call's, bit for bit
        np.testing.assert_array_equal(F[:, c], ctx.exact_gp_f(X, a, ell, Z[:, c], jit))
    Fr, Zr, gr = vr.vjp_reverse(X, a, ell, Z, Fb, jit)
    # Zbar against L^T Fbar with the library's own factor (LAPACK's differs from it by rounding amplified by cond(K))
    Lg = ctx.potrf(ctx.se_cov(X, None, a, ell, diag_add=jit))
    assert _rel(Zb, np.tril(Lg).T @ Fb) <= 1e-12
    assert _rel(Zb, Zr) <= 1e-9
    if n == 1:
        s = math.sqrt(a * a + jit)
        np.testing.assert_allclose(g[0], Fb[0] @ Z[0] * a / s, rtol=1e-14)
        assert g[1] == 0.0
        return
    assert _rel(g, gr) <= 1e-8, (g, gr)

    def fun(theta):
        return sum(float(Fb[:, c] @ ctx.exact_gp_f(X, theta[0], theta[1:], Z[:, c], jit)) for c in range(k))
    cd = vr.central_diff(fun, np.concatenate([[a], ell]), h_rel=1e-5)
    assert _rel(g, cd) <= 1e-6, (g, cd)


@pytest.mark.parametrize("l", [0.5, 1.0, 1.6])
def test_reference_configuration(ctx, l):
    """x = linspace(0, 10, 100), alpha = 1, jitter 1e-10 (test_interpolate.R:31-36 runs models/exact_gp.stan there), cond(K) ~ 1e11.
    The device's factor differs from the exact one by rounding amplified by cond(K), and theta_bar inherits that: float64 reverse
    mode on the device's own L lands where the library does (checked to 1e-5), the longdouble forward mode -- and the library's
    independent forward-mode tangent, gpmi_rbf_cov_chol -- within 1e-3 (measured: 2.2e-4 at l = 0.5, <= 7e-5 at 1.0 and 1.6)."""
    x = np.linspace(0, 10, 100)
    rng = np.random.default_rng(int(10 * l))
    z = rng.standard_normal(100); u = rng.standard_normal(100)
    f, zb, g = ctx.exact_gp_f_vjp(x, 1.0, [l], z, u, 1e-10)
    np.testing.assert_array_equal(f, ctx.exact_gp_f(x, 1.0, [l], z, 1e-10))
    Lg = np.tril(ctx.potrf(ctx.se_cov(x, None, 1.0, [l], diag_add=1e-10)))
    U = np.linalg.inv(Lg).T
    S = U @ vr.phi((Lg.T @ u)[:, None] @ z[None, :]) @ U.T
    gd = np.array([np.sum(0.5 * (S + S.T) * dk) for dk in vr.dK_dtheta(x.reshape(-1, 1), 1.0, [l], 1)])
    assert np.all(np.abs(g - gd) <= 1e-5 * np.abs(gd)), (g, gd)
    g_ld = vr.vjp_forward_longdouble(x.reshape(-1, 1), 1.0, [l], z, u, 1e-10).astype(float)
    assert np.all(np.abs(g - g_ld) <= 1e-3 * np.abs(g_ld)), (g, g_ld)
    L, dL = ctx.rbf_cov_chol(x, l)
    fwd = float(u @ (dL @ z))
    assert abs(g[1] - fwd) <= 1e-3 * abs(fwd), (g[1], fwd)


@pytest.mark.parametrize("n", [100, 256])
def test_one_workgroup_and_chain_agree(ctx, chain_ctx, n):
    X, a, ell, Z, Fb = _problem(n, 2, 2, 2, seed=n)
    F1, Z1, g1 = ctx.exact_gp_f_vjp(X, a, ell, Z, Fb, 1e-6)
    F2, Z2, g2 = chain_ctx.exact_gp_f_vjp(X, a, ell, Z, Fb, 1e-6)
    # F and Zbar to 1e-12; theta_bar is a sum with cancellation formed in a different order (register tiles against
    # 64 x 64 tile sums): measured 2.2e-12 at n = 100
    assert _rel(F2, F1) <= 1e-12 and _rel(Z2, Z1) <= 1e-12 and _rel(g2, g1) <= 1e-11, (g1, g2)


@pytest.mark.parametrize("n", [100, 700])
def test_repeated_calls_bit_identical(ctx, chain_ctx, n):
    X, a, ell, Z, Fb = _problem(n, 3, 1, 2, seed=5)
    for c in (ctx, chain_ctx):
        r1 = c.exact_gp_f_vjp(X, a, ell, Z, Fb, 1e-6)
        r2 = c.exact_gp_f_vjp(X, a, ell, Z, Fb, 1e-6)
        for p, q in zip(r1, r2):
            np.testing.assert_array_equal(p, q)


@pytest.mark.parametrize("n,k", [(100, 2), (700, 1)])
def test_dev_equals_host(ctx, n, k):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    X, a, ell, Z, Fb = _problem(n, 2, 1, k, seed=9)
    F, Zb, g = ctx.exact_gp_f_vjp(X, a, ell, Z, Fb, 1e-6)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)      # (D, n) row-major == n x D column-major
    dZ = torch.from_numpy(np.ascontiguousarray(Z.T)).to(dev)
    dFb = torch.from_numpy(np.ascontiguousarray(Fb.T)).to(dev)
    dF = torch.zeros((k, n), dtype=torch.float64, device=dev); dZb = torch.zeros_like(dF)
    dg = torch.zeros(2, dtype=torch.float64, device=dev); info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.exact_gp_f_vjp_dev(dX.data_ptr(), n, n, 2, a, ell, 1e-6, dZ.data_ptr(), k, n, dFb.data_ptr(), n, dF.data_ptr(), n,
                           dZb.data_ptr(), n, dg.data_ptr(), info.data_ptr())
    ctx.sync()
    assert int(info.item()) == 0
    np.testing.assert_array_equal(dF.cpu().numpy().T, F)
    np.testing.assert_array_equal(dZb.cpu().numpy().T, Zb)
    np.testing.assert_array_equal(dg.cpu().numpy(), g)
    # F is optional
    dZb2 = torch.zeros_like(dF)
    ctx.exact_gp_f_vjp_dev(dX.data_ptr(), n, n, 2, a, ell, 1e-6, dZ.data_ptr(), k, n, dFb.data_ptr(), n, None, n,
                           dZb2.data_ptr(), n, dg.data_ptr(), info.data_ptr())
    ctx.sync()
    np.testing.assert_array_equal(dZb2.cpu().numpy().T, Zb)


@pytest.mark.parametrize("n", [1, 100, 1000, 5000])
def test_trmv_lower_t(ctx, n):
    rng = np.random.default_rng(n)
    L = np.tril(rng.standard_normal((n, n))) + n * np.eye(n)
    u = rng.standard_normal(n)
    w = ctx.trmv_lower_t(L, u)
    want = L.T @ u
    assert _rel(w, want) <= 1e-12
    np.testing.assert_array_equal(ctx.trmv_lower_t(L, u), w)


@pytest.mark.parametrize("n", [50, 300])
def test_not_positive_definite(ctx, n):
    from gp_amd._lib import NotPositiveDefinite, _p
    X = np.ones((n, 1))
    Z = np.ones((n, 1)); Fb = np.ones((n, 1))
    with pytest.raises(NotPositiveDefinite):
        ctx.exact_gp_f_vjp(X, 1.0, [1.0], Z, Fb, 0.0)
    F = np.zeros((n, 1), order="F"); Zb = np.zeros((n, 1), order="F"); g = np.zeros(2)
    Xf = np.asfortranarray(X); Zf = np.asfortranarray(Z); Fbf = np.asfortranarray(Fb)
    rc = ctx._lib.gpmi_exact_gp_f_vjp(ctx._h, _p(Xf), n, n, 1, C.c_double(1.0), _p(np.ones(1)), 1, C.c_double(0.0), _p(Zf), 1, n,
                                      _p(Fbf), n, _p(F), n, _p(Zb), n, _p(g))
    assert rc > 0
    assert np.all(np.isnan(F)) and np.all(np.isnan(Zb)) and np.all(np.isnan(g))
    # the context is usable afterwards
    Xg, a, ell, Zg, Fbg = _problem(n, 1, 1, 1, seed=1)
    ctx.exact_gp_f_vjp(Xg, a, ell, Zg, Fbg, 1e-6)


def test_bad_arguments(ctx):
    from gp_amd._lib import _p
    n = 10
    X = np.asfortranarray(np.linspace(0, 3, n).reshape(-1, 1)); Z = np.ones((n, 1), order="F"); F = np.zeros((n, 1), order="F")
    g = np.zeros(2); e = np.ones(1)
    lib, h = ctx._lib, ctx._h
    d = C.c_double

    def call(n_=n, ldx=n, D=1, alpha=1.0, ell=e, n_ell=1, k=1, ldz=n, ldfb=n, ldzb=n, Zp=Z):
        return lib.gpmi_exact_gp_f_vjp(h, _p(X), n_, ldx, D, d(alpha), _p(ell), n_ell, d(1e-6), _p(Zp), k, ldz, _p(Z), ldfb, None, n,
                                       _p(F), ldzb, _p(g))
    assert call() == 0
    for kw in ({"n_": 0}, {"ldx": n - 1}, {"D": 0}, {"D": 65}, {"alpha": 0.0}, {"alpha": -1.0}, {"n_ell": 2}, {"k": 0},
               {"ldz": n - 1}, {"ldfb": n - 1}, {"ldzb": n - 1}, {"ell": np.array([-1.0])}):
        assert call(**kw) == -1, kw
    assert lib.gpmi_exact_gp_f_vjp(h, None, n, n, 1, d(1.0), _p(e), 1, d(0.0), _p(Z), 1, n, _p(Z), n, None, n, _p(F), n, _p(g)) == -1
    assert lib.gpmi_trmv_lower_t(h, None, n, n, _p(e), _p(g)) == -1
    assert lib.gpmi_trmv_lower_t(h, _p(X), n, n - 1, _p(Z), _p(F)) == -1
    assert lib.gpmi_set_option(h, b"small_vjp", 257) == -1


def test_exact_gp_log_prob_grad(ctx):
    from gp_amd import stan_models
    rng = np.random.default_rng(4)
    x = np.linspace(0, 10, 20)
    y = np.sin(x) + 0.1 * rng.standard_normal(20)
    z = rng.standard_normal(20)
    l, s = 0.6, 0.3
    lp, g = stan_models.exact_gp_log_prob_grad(x, y, l, s, z, ctx=ctx)
    want = vr.exact_gp_lp(x, y, l, s, z)
    assert abs(lp - want) <= 1e-9 * abs(want)
    assert g.shape == (22,)

    def at(theta):
        zz = z.copy(); zz[[0, 7, 19]] = theta[2:]
        return stan_models.exact_gp_log_prob_grad(x, y, theta[0], theta[1], zz, ctx=ctx)[0]
    cd = vr.central_diff(at, np.array([l, s, z[0], z[7], z[19]]), h_rel=1e-6)
    got = np.array([g[0], g[1], g[2], g[9], g[21]])
    np.testing.assert_allclose(got, cd, rtol=1e-6, atol=1e-6 * np.abs(cd).max())
