"""GPU: gpmi_gp_predict_joint / gpmi_gp_predict_joint_dev (the joint posterior at new D-dimensional inputs: mean, covariance and
draws mean + chol(C) Z) against the numpy yardstick tests/predict_joint_reference.py, numpy's LAPACK at the mid size, and
gpmi_gp_predict on the same context.

Tolerances: the mean predict_reference.MEAN_TOL relative in the max norm, the covariance VAR_TOL alpha^2 absolute in the max
norm (tied to the yardstick's own error by tests/test_predict_joint_reference.py).  The factor and the draws are held to textbook
componentwise backward bounds with eps = 2^-52 (stated at each test); nothing there is measured."""
import ctypes as C
import functools

import numpy as np
import pytest

import predict_joint_reference as pj
import predict_reference as pr

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
SENT = -7.25


@pytest.fixture(scope="module")
def octx():
    """A context of this module's own for the runs that change options (the session context keeps its defaults)."""
    import gp_amd
    c = gp_amd.Context(0)
    yield c
    c.close()


def _route(ctx, octx, route):
    """default: the session context as it is; chain: small_pj = 0; wg: the one-workgroup kernel up to 600 rows."""
    if route == "default":
        return ctx
    octx.set_option("small_pj", 0 if route == "chain" else 600)
    return octx


@functools.lru_cache(maxsize=None)
def _case(name):
    _, n, D, m, alpha, ell, sigma = pj.case(name)
    X, y, Xs = pr.inputs(n, D, m)
    want = pj.joint(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER, float)
    return X, y, Xs, alpha, ell, sigma, want


def _call(c, name, Z=None, want_cov=True, post_jitter=pj.POST_JITTER):
    X, y, Xs, alpha, ell, sigma, _ = _case(name)
    return c.gp_predict_joint(X, y, alpha, ell, sigma, pj.JITTER, Xs, post_jitter=post_jitter, Z=Z, want_cov=want_cov)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [(c[0], r) for c in pj.cases() for r in ("default", "chain")] + [("n300_d3", "wg")])
def test_parity_with_the_reference(ctx, octx, name, route):
    X, y, Xs, alpha, ell, sigma, want = _case(name)
    c = _route(ctx, octx, route)
    got = _call(c, name)
    em = pr.max_rel(got["mean"], want[0])
    ec = float(np.max(np.abs(got["cov"] - want[1]))) / alpha ** 2
    print("%s [%s]: mean %.2e cov/alpha^2 %.2e" % (name, route, em, ec))
    assert got["info"] == 0 and got["draws"] is None
    assert em <= pr.MEAN_TOL
    assert ec <= pr.VAR_TOL
    assert np.array_equal(got["cov"], got["cov"].T)
    point = c.gp_predict(X, y, alpha, ell, sigma, pj.JITTER, Xs)
    ep = pr.max_rel(got["mean"], point["mean"])
    ev = float(np.max(np.abs(np.diag(got["cov"]) - pj.POST_JITTER - point["var"]))) / alpha ** 2
    print("   against gpmi_gp_predict: mean %.2e var/alpha^2 %.2e" % (ep, ev))
    assert point["info"] == 0
    assert ep <= pr.MEAN_TOL and ev <= pr.VAR_TOL


# ---- 2. the factor -----------------------------------------------------------------------------------------------------------
_FACTOR = {}


def _factor(ctx, octx, name, route):
    """(Lc, result of the Z = I call with the case's y) once per (case, route).  The factor does not depend on y, so Lc is read
    EXACTLY from a second Z = I call with y = 0 (mean = 0, draws = Lc): draws - mean of the first call is fl(mean + Lc) - mean,
    whose error eps |mean + Lc| / 2 is absolute in |mean| and not relative to the entries of Lc -- with it the componentwise
    bound below asks more than a correctly rounded result can give (measured on n21_d3: 1.25 x the bound through draws - mean, 0.054 x for
    the same factor read exactly)."""
    if (name, route) not in _FACTOR:
        X, y, Xs, alpha, ell, sigma, _ = _case(name)
        m = Xs.shape[0]
        c = _route(ctx, octx, route)
        got = _call(c, name, Z=np.eye(m))
        zero = c.gp_predict_joint(X, np.zeros_like(y), alpha, ell, sigma, pj.JITTER, Xs, post_jitter=pj.POST_JITTER, Z=np.eye(m))
        assert zero["info"] == 0 and np.all(zero["mean"] == 0.0)
        np.testing.assert_array_equal(zero["cov"], got["cov"])
        _FACTOR[(name, route)] = (zero["draws"], got)
    return _FACTOR[(name, route)]


@pytest.mark.parametrize("route", ["wg", "chain"])
@pytest.mark.parametrize("name", ["n21_d3", "n300_d3"])
def test_draws_of_the_identity_are_the_cholesky_factor(ctx, octx, name, route):
    """Z = I_m: draws = mean + Lc to the bit (one product with an exact one, exact zeros, one addition), Lc is lower triangular
    with a positive diagonal and |Lc Lc^T - cov| <= 2 (m + 1) eps |Lc| |Lc|^T componentwise -- the backward bound of a Cholesky
    factorisation of order m, (m + 1) eps |L| |L|^T, times 2."""
    Lc, got = _factor(ctx, octx, name, route)
    m = Lc.shape[0]
    assert got["info"] == 0
    np.testing.assert_array_equal(got["draws"], got["mean"][:, None] + Lc)
    assert np.all(np.triu(Lc, 1) == 0.0)
    assert np.all(np.diag(Lc) > 0.0)
    Ll = Lc.astype(np.longdouble)
    res = np.abs((Ll @ Ll.T).astype(float) - got["cov"])
    bound = 2 * (m + 1) * EPS * (np.abs(Lc) @ np.abs(Lc).T)
    print("%s [%s]: max |Lc Lc^T - cov| / bound %.3f" % (name, route, float(np.max(res / bound))))
    assert np.all(res <= bound)


# ---- 3. the product kernel's edges -------------------------------------------------------------------------------------------
def _raw(c, X, y, alpha, ell, sigma, jitter, Xs, post_jitter, mean, cov, Z, B, draws, n=None, m=None, D=None, ldx=None, ldxs=None,
         ldc=None, ldz=None, ldd=None, n_ell=None):
    """gpmi_gp_predict_joint with every argument as given (no checks of the Python layer in front); None: NULL."""
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ell = np.ascontiguousarray(np.asarray(ell, float).ravel())
    return c._lib.gpmi_gp_predict_joint(
        c._h, p(X), int(X.shape[0] if n is None else n), int(X.shape[0] if ldx is None else ldx), int(X.shape[1] if D is None else D),
        p(y), C.c_double(alpha), p(ell), int(ell.size if n_ell is None else n_ell), C.c_double(sigma), C.c_double(jitter), p(Xs),
        int(Xs.shape[0] if m is None else m), int(Xs.shape[0] if ldxs is None else ldxs), C.c_double(post_jitter), p(mean), p(cov),
        int(Xs.shape[0] if ldc is None else ldc), p(Z), int(B), int(Xs.shape[0] if ldz is None else ldz), p(draws),
        int(Xs.shape[0] if ldd is None else ldd))


_EDGE_DRAWS = {}
EDGE_B = (1, 5, 16, 17, 33)


@pytest.mark.parametrize("B", EDGE_B)
def test_product_kernel_edges(ctx, octx, B):
    """Chain route, m = 259 (ragged against 16, three 128-row blocks), padded leading dimensions with sentinels, and every draw
    within 2 (m + 2) eps (|Lc| |Z| + |mean|) of the long-double mean + Lc Z: (m + 1) eps |Lc| |Z| for a sum of m products in
    any order, one eps for the addition of the mean, times 2; Lc is the factor of test 2."""
    name = "n300_d3"
    X, y, Xs, alpha, ell, sigma, _ = _case(name)
    Lc, ref = _factor(ctx, octx, name, "chain")
    c = _route(ctx, octx, "chain")
    m = Xs.shape[0]
    Zall = np.random.default_rng(259).standard_normal((m, max(EDGE_B)))
    ldz, ldd, ldc = m + 3, m + 5, m + 1
    Z = np.full((ldz, B), SENT, order="F"); Z[:m] = Zall[:, :B]
    draws = np.full((ldd, B), SENT, order="F")
    cov = np.full((ldc, m), SENT, order="F")
    mean = np.full(m + 1, SENT)
    rc = _raw(c, X, y, alpha, ell, sigma, pj.JITTER, Xs, pj.POST_JITTER, mean, cov, Z, B, draws, ldc=ldc, ldz=ldz, ldd=ldd)
    assert rc == 0
    assert mean[m] == SENT and np.all(cov[m:] == SENT) and np.all(draws[m:] == SENT) and np.all(Z[m:] == SENT)
    np.testing.assert_array_equal(mean[:m], ref["mean"])
    np.testing.assert_array_equal(cov[:m], ref["cov"])
    want = ref["mean"].astype(np.longdouble)[:, None] + Lc.astype(np.longdouble) @ Zall[:, :B].astype(np.longdouble)
    bound = 2 * (m + 2) * EPS * (np.abs(Lc) @ np.abs(Zall[:, :B]) + np.abs(ref["mean"])[:, None])
    err = np.abs((draws[:m].astype(np.longdouble) - want).astype(float))
    print("B = %d: max error / bound %.3f" % (B, float(np.max(err / bound))))
    assert np.all(err <= bound)
    _EDGE_DRAWS[B] = draws[:m].copy()
    for other, d in _EDGE_DRAWS.items():   # column b has the same bits whatever B is
        k = min(other, B)
        np.testing.assert_array_equal(d[:, :k], draws[:m, :k])


def test_columns_do_not_depend_on_their_neighbours(ctx, octx):
    """The same column of Z beside other columns, on both routes: identical bits."""
    for name, route in (("n21_d3", "default"), ("n300_d3", "chain"), ("n300_d3", "wg")):
        c = _route(ctx, octx, route)
        m = _case(name)[2].shape[0]
        rng = np.random.default_rng(3)
        Z = rng.standard_normal((m, 19))
        a = _call(c, name, Z=Z)
        Z2 = rng.standard_normal((m, 40)); Z2[:, 37] = Z[:, 4]
        b = _call(c, name, Z=Z2)
        one = _call(c, name, Z=Z[:, 4:5])
        np.testing.assert_array_equal(a["draws"][:, 4], b["draws"][:, 37])
        np.testing.assert_array_equal(a["draws"][:, 4], one["draws"][:, 0])


# ---- 4. determinism and entry points -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(21, 41), (700, 300)])
def test_repeated_calls_and_optional_outputs(ctx, n, m):
    X, y, Xs = pr.inputs(n, 3, m)
    Z = np.random.default_rng(n).standard_normal((m, 7))
    args = (X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs)
    a = ctx.gp_predict_joint(*args, post_jitter=1e-6, Z=Z)
    b = ctx.gp_predict_joint(*args, post_jitter=1e-6, Z=Z)
    assert a["info"] == 0 and b["info"] == 0
    for k in ("mean", "cov", "draws"):
        np.testing.assert_array_equal(a[k], b[k])
    nocov = ctx.gp_predict_joint(*args, post_jitter=1e-6, Z=Z, want_cov=False)
    assert nocov["cov"] is None and nocov["info"] == 0
    np.testing.assert_array_equal(nocov["mean"], a["mean"])
    np.testing.assert_array_equal(nocov["draws"], a["draws"])
    nodraws = ctx.gp_predict_joint(*args, post_jitter=1e-6)
    assert nodraws["draws"] is None and nodraws["info"] == 0
    np.testing.assert_array_equal(nodraws["mean"], a["mean"])
    np.testing.assert_array_equal(nodraws["cov"], a["cov"])


@pytest.mark.parametrize("n,m,want_cov", [(21, 41, True), (21, 41, False), (700, 300, True), (700, 300, False)])
def test_dev_equals_host(ctx, n, m, want_cov):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    X, y, Xs = pr.inputs(n, 3, m)
    B = 5
    Z = np.asfortranarray(np.random.default_rng(m).standard_normal((m, B)))
    host = ctx.gp_predict_joint(X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs, post_jitter=1e-6, Z=Z)
    ldc, ldz, ldd = m + 2, m + 1, m + 3
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)      # (D, n) row-major == n x D column-major
    dXs = torch.from_numpy(np.ascontiguousarray(Xs.T)).to(dev)
    dy = torch.from_numpy(y).to(dev)
    Zp = np.full((B, ldz), SENT); Zp[:, :m] = Z.T
    dZ = torch.from_numpy(Zp).to(dev)
    dmean = torch.full((m + 1,), SENT, dtype=torch.float64, device=dev)
    dcov = torch.full((m, ldc), SENT, dtype=torch.float64, device=dev)
    ddraws = torch.full((B, ldd), SENT, dtype=torch.float64, device=dev)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.gp_predict_joint_dev(dX.data_ptr(), n, n, 3, dy.data_ptr(), 1.0, pr.ARD3, 0.1, 1e-6, dXs.data_ptr(), m, m, 1e-6,
                             dmean.data_ptr(), dcov.data_ptr() if want_cov else None, ldc, dZ.data_ptr(), B, ldz, ddraws.data_ptr(),
                             ldd, info.data_ptr())
    ctx.sync()
    assert int(info.item()) == 0
    mean = dmean.cpu().numpy(); cov = dcov.cpu().numpy().T; draws = ddraws.cpu().numpy().T
    np.testing.assert_array_equal(mean[:m], host["mean"])
    np.testing.assert_array_equal(draws[:m], host["draws"])
    assert mean[m] == SENT and np.all(draws[m:] == SENT)
    if want_cov:
        np.testing.assert_array_equal(cov[:m], host["cov"])
        assert np.all(cov[m:] == SENT)
    else:
        assert np.all(cov == SENT)   # no covariance asked for: the buffer beside the call is not touched


# ---- 5. status ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "chain"])
def test_sigma_not_positive_definite(ctx, octx, route):
    c = _route(ctx, octx, route)
    X, y, Xs = pr.inputs(40, 2, 30)
    X[20:28] = X[19]   # nine copies of one point, no noise, no jitter: singular (the construction of tests/test_gpu_predict.py)
    Z = np.random.default_rng(0).standard_normal((30, 3))
    got = c.gp_predict_joint(X, y, 1.0, (0.3,), 0.0, 0.0, Xs, post_jitter=1e-6, Z=Z)
    assert 1 <= got["info"] <= 40
    assert np.all(np.isnan(got["mean"])) and np.all(np.isnan(got["cov"])) and np.all(np.isnan(got["draws"]))
    ok = c.gp_predict_joint(X, y, 1.0, (0.3,), 0.1, 1e-6, Xs, post_jitter=1e-6, Z=Z)     # the same data with noise: fine
    assert ok["info"] == 0 and np.all(np.isfinite(ok["draws"]))


@pytest.mark.parametrize("route", ["default", "chain"])
def test_covariance_not_positive_definite(ctx, octx, route):
    c = _route(ctx, octx, route)
    n, m, alpha = 40, 30, 1.3
    X, y, Xs = pr.inputs(n, 3, m)
    Z = np.random.default_rng(1).standard_normal((m, 4))
    args = (X, y, alpha, pr.ARD3, 0.1, 1e-6, Xs)
    bad = c.gp_predict_joint(*args, post_jitter=-2 * alpha ** 2, Z=Z)
    ref = c.gp_predict_joint(*args, post_jitter=-2 * alpha ** 2)
    assert ref["info"] == 0   # B = 0: C is not factored
    assert bad["info"] == n + 1
    np.testing.assert_array_equal(bad["mean"], ref["mean"])
    np.testing.assert_array_equal(bad["cov"], ref["cov"])
    assert np.all(np.isfinite(bad["cov"])) and np.all(np.diag(bad["cov"]) < 0)
    assert np.all(np.isnan(bad["draws"]))


def test_bad_arguments_return_earg_and_write_nothing(ctx):
    n, m, D, B = 12, 9, 3, 2
    X, y, Xs = pr.inputs(n, D, m)
    Z = np.asfortranarray(np.random.default_rng(2).standard_normal((m, B)))

    def run(null=(), **kw):
        mean = np.full(m, SENT); cov = np.full((m, m), SENT, order="F"); draws = np.full((m, B), SENT, order="F")
        a = dict(X=X, y=y, alpha=1.0, ell=pr.ARD3, sigma=0.1, jitter=1e-6, Xs=Xs, post_jitter=1e-6, mean=mean, cov=cov, Z=Z, B=B,
                 draws=draws)
        a.update(dict(n=n, m=m, D=D, ldx=n, ldxs=m, ldc=m, ldz=m, ldd=m))   # the sizes do not come from a pointer that may be NULL
        a.update(kw)
        for k in null:
            a[k] = None
        rc = _raw(ctx, a.pop("X"), a.pop("y"), a.pop("alpha"), a.pop("ell"), a.pop("sigma"), a.pop("jitter"), a.pop("Xs"),
                  a.pop("post_jitter"), a.pop("mean"), a.pop("cov"), a.pop("Z"), a.pop("B"), a.pop("draws"), **a)
        assert np.all(mean == SENT) and np.all(cov == SENT) and np.all(draws == SENT), (null, kw)
        return rc

    for kw in (dict(n=0), dict(m=0), dict(B=-1), dict(D=0), dict(D=65), dict(ldx=n - 1), dict(ldxs=m - 1), dict(ldc=m - 1),
               dict(ldz=m - 1), dict(ldd=m - 1), dict(alpha=0.0), dict(alpha=-1.0), dict(ell=(0.3, 0.0, 0.5)), dict(ell=(-0.3,)),
               dict(ell=(0.3, 0.5), n_ell=2), dict(sigma=-0.1)):
        assert run(**kw) == -1, kw
    for null in (("X",), ("y",), ("Xs",), ("mean",), ("Z",), ("draws",)):
        assert run(null=null) == -1, null
    # X is dereferenced only behind the checks; a D = 65 call sees the same 3-column array
    good = ctx.gp_predict_joint(X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs, post_jitter=1e-6, Z=Z)
    assert good["info"] == 0
    # NULL Z / draws are fine when B == 0, and so is a NULL cov
    mean = np.full(m, SENT)
    assert _raw(ctx, X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs, 1e-6, mean, None, None, 0, None) == 0
    np.testing.assert_array_equal(mean, good["mean"])


# ---- 6. mid size against LAPACK ----------------------------------------------------------------------------------------------
def test_mid_size_against_lapack(ctx):
    n, D, m, B = 2048, 3, 1000, 64
    alpha, ell, sigma = 1.0, pr.ARD3, 0.1
    X, y, Xs = pr.inputs(n, D, m)
    want = pj.joint_lapack(X, y, Xs, alpha, ell, sigma, pj.JITTER, pj.POST_JITTER)
    Z = np.random.default_rng(64).standard_normal((m, B))
    got = ctx.gp_predict_joint(X, y, alpha, ell, sigma, pj.JITTER, Xs, post_jitter=pj.POST_JITTER, Z=Z)
    em = pr.max_rel(got["mean"], want[0])
    ec = float(np.max(np.abs(got["cov"] - want[1]))) / alpha ** 2
    print("n = %d m = %d: mean %.2e cov/alpha^2 %.2e" % (n, m, em, ec))
    assert got["info"] == 0
    assert em <= pr.MEAN_TOL and ec <= pr.VAR_TOL
    assert np.array_equal(got["cov"], got["cov"].T)
    fac = ctx.gp_predict_joint(X, np.zeros(n), alpha, ell, sigma, pj.JITTER, Xs, post_jitter=pj.POST_JITTER, Z=np.eye(m), want_cov=False)
    assert fac["info"] == 0 and np.all(fac["mean"] == 0.0)
    Lc = fac["draws"]   # y = 0: the factor itself (see _factor)
    assert np.all(np.triu(Lc, 1) == 0.0) and np.all(np.diag(Lc) > 0.0)
    ref = got["mean"].astype(np.longdouble)[:, None] + Lc.astype(np.longdouble) @ Z.astype(np.longdouble)
    bound = 2 * (m + 2) * EPS * (np.abs(Lc) @ np.abs(Z) + np.abs(got["mean"])[:, None])
    err = np.abs((got["draws"].astype(np.longdouble) - ref).astype(float))
    print("   draws: max error / bound %.3f" % float(np.max(err / bound)))
    assert np.all(err <= bound)
