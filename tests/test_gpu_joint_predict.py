"""GPU: gpmi_joint_predict / gpmi_joint_predict_dev (the posterior of f, f', f'' at new times given stacked observations [y; y']:
mean, covariance and draws mean + chol(C) Z) against the long-double yardstick tests/joint_predict_reference.py and against
gpmi_deriv_cov on the same context.

Tolerances: C_mean eps cond_2(S) for the mean (relative in the max norm per order block) and C_cov eps cond_2(S) for the covariance
(absolute per block (a, b) in units of alpha^2 / l^(a + b)), the constants measured on the reference itself
(joint_predict_reference.constants, printed by tests/test_joint_predict_reference.py).  The factor and the draws are held to
textbook componentwise backward bounds with eps = 2^-52 (stated at each test); nothing there is measured."""
import ctypes as C

import numpy as np
import pytest

import joint_grad_reference as jg
import joint_predict_reference as jp

pytestmark = pytest.mark.gpu

EPS = jp.EPS
SENT = -7.25
ALPHA, SIGMA, JITTER = jg.PARITY_ALPHA, jg.PARITY_SIGMA, jg.PARITY_JITTER
CASE = {c[0]: c for c in jg.PARITY_CASES}
KIND = (("QQ", "QR", "QT"), ("RQ", "RR", "RT"), ("TQ", "TR", "TT"))


@pytest.fixture(scope="module")
def octx():
    """A context of this module's own for the runs that change options (the session context keeps its defaults)."""
    import gp_amd
    c = gp_amd.Context(0)
    yield c
    c.close()


def _route(ctx, octx, route):
    """default: the session context as it is; chain: small_jp = 0; wg: the one-workgroup kernel up to 600 rows."""
    if route == "default":
        return ctx
    octx.set_option("small_jp", 0 if route == "chain" else 600)
    return octx


def _call(c, n, mask, Z=None, want_cov=True, yy=None, pj=None):
    case = CASE[n]
    t, yy0, ts = jp.inputs(case)
    return c.joint_predict(t, yy0 if yy is None else yy, ALPHA, case[1], SIGMA, JITTER, ts, mask,
                           jp.post_jitter(case[1], mask) if pj is None else pj, Z=Z, want_cov=want_cov)


_GOT = {}


def _result(ctx, octx, n, mask, route):
    """The B = 0 result of one (case, orders, route), computed once per session."""
    if (n, mask, route) not in _GOT:
        _GOT[(n, mask, route)] = _call(_route(ctx, octx, route), n, mask)
    return _GOT[(n, mask, route)]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
PARITY = ([(c[0], 7, "default") for c in jg.PARITY_CASES] + [(n, 7, "chain") for n in (65, 129, 350)] + [(129, 7, "wg")]
          + [(n, mask, route) for n in (21, 129) for mask in (2, 5) for route in ("chain", "wg")])


@pytest.mark.parametrize("n,mask,route", PARITY)
def test_parity_with_the_long_double_reference(ctx, octx, n, mask, route):
    case = CASE[n]
    m = jp.case_m(case)
    want_mean, want_cov = jp.reference(case, mask)
    tol_mean, tol_cov = jp.tolerances(case)
    got = _result(ctx, octx, n, mask, route)
    em = jp.mean_error(got["mean"], want_mean, m)
    ec = jp.cov_error(got["cov"], want_cov, jp.scales(case[1], mask, m))
    print("n = %d orders %d [%s]: mean %.2e (tol %.2e) cov %.2e (tol %.2e)" % (n, mask, route, em, tol_mean, ec, tol_cov))
    assert got["info"] == 0 and got["draws"] is None
    assert em <= tol_mean
    assert ec <= tol_cov
    assert np.array_equal(got["cov"], got["cov"].T)


@pytest.mark.parametrize("n,mask,route", [(n, mask, route) for n in (21, 129) for mask in (2, 5) for route in ("chain", "wg")])
def test_sub_blocks_of_all_orders_agree_with_fewer_orders(ctx, octx, n, mask, route):
    """The rows of the requested orders cut out of the orders = 7 result against the orders = 2 / 5 results: the same tolerances
    (the factorisation of S is the same, the Schur complement is formed beside other columns); bits are not compared."""
    case = CASE[n]
    m = jp.case_m(case)
    tol_mean, tol_cov = jp.tolerances(case)
    full = _result(ctx, octx, n, 7, route)
    part = _result(ctx, octx, n, mask, route)
    rows = np.concatenate([np.arange(a * m, (a + 1) * m) for a in jp.orders_of(mask)])
    em = jp.mean_error(full["mean"][rows], part["mean"].astype(jp.LD), m)
    ec = jp.cov_error(full["cov"][np.ix_(rows, rows)], part["cov"].astype(jp.LD), jp.scales(case[1], mask, m))
    print("n = %d orders %d [%s]: mean %.2e cov %.2e" % (n, mask, route, em, ec))
    assert em <= tol_mean and ec <= tol_cov


# ---- 2. the builder pinned to the existing kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["chain", "wg"])
@pytest.mark.parametrize("m", [1, 17, 131])
def test_star_blocks_have_the_bits_of_deriv_cov(ctx, octx, m, route):
    """Training times at least 45 l away from every new time: exp(-45^2 / 2) underflows, Ks is exactly zero, so mean = 0 and C is
    the prior: block (a, b) = gpmi_deriv_cov(kind(a, b), ts, ts) to the bit, plus post_jitter[a] on its diagonal (one addition).
    Fixes signs, argument order, block order and the arithmetic behind the shared exponential (m = 131: three row tiles)."""
    c = _route(ctx, octx, route)
    l, n = 0.5, 5
    rng = np.random.default_rng(m)
    ts = rng.uniform(-1.0, 1.0, m)
    t = 100.0 + rng.uniform(0.0, 1.0, n)
    assert np.min(np.abs(t[:, None] - ts[None, :])) >= 45 * l
    assert np.all(c.deriv_cov("QQ", ts, t, ALPHA, l) == 0.0)
    yy = rng.standard_normal(2 * n)
    pj = np.array([3e-6, 5e-5, 7e-4])
    got = c.joint_predict(t, yy, ALPHA, l, SIGMA, JITTER, ts, 7, pj)
    assert got["info"] == 0
    assert np.all(got["mean"] == 0.0)
    for a in range(3):
        for b in range(3):
            want = c.deriv_cov(KIND[a][b], ts, ts, ALPHA, l)
            if a == b:
                want[np.diag_indices(m)] += pj[a]
            np.testing.assert_array_equal(got["cov"][a * m:(a + 1) * m, b * m:(b + 1) * m], want, err_msg=KIND[a][b])


# ---- 3. the factor -----------------------------------------------------------------------------------------------------------
_FACTOR = {}


def _factor(ctx, octx, n, route):
    """(Lc, result of the Z = I call with the case's yy) once per (case, route), orders = 7.  The factor does not depend on yy, so
    Lc is read EXACTLY from a second Z = I call with yy = 0 (mean = 0, draws = Lc): draws - mean of the first call would be
    fl(mean + Lc) - mean, whose rounding is absolute in |mean| and not relative to the entries of Lc (the reading
    tests/test_gpu_predict_joint.py takes of its factor, for the reason stated there)."""
    if (n, route) not in _FACTOR:
        c = _route(ctx, octx, route)
        pm = 3 * jp.case_m(CASE[n])
        got = _call(c, n, 7, Z=np.eye(pm))
        zero = _call(c, n, 7, Z=np.eye(pm), yy=np.zeros(2 * n))
        assert zero["info"] == 0 and np.all(zero["mean"] == 0.0)
        np.testing.assert_array_equal(zero["cov"], got["cov"])
        _FACTOR[(n, route)] = (zero["draws"], got)
    return _FACTOR[(n, route)]


@pytest.mark.parametrize("route", ["wg", "chain"])
@pytest.mark.parametrize("n", [21, 129])
def test_draws_of_the_identity_are_the_cholesky_factor(ctx, octx, n, route):
    """Z = I: draws = mean + Lc to the bit (one product with an exact one, exact zeros, one addition), Lc is lower triangular with
    a positive diagonal and |Lc Lc^T - cov| <= 2 (pm + 1) eps |Lc| |Lc|^T componentwise -- the backward bound of a Cholesky
    factorisation of order pm, (pm + 1) eps |L| |L|^T, times 2."""
    Lc, got = _factor(ctx, octx, n, route)
    pm = Lc.shape[0]
    assert got["info"] == 0
    np.testing.assert_array_equal(got["cov"], _result(ctx, octx, n, 7, route)["cov"])   # B does not change mean and cov
    np.testing.assert_array_equal(got["draws"], got["mean"][:, None] + Lc)
    assert np.all(np.triu(Lc, 1) == 0.0)
    assert np.all(np.diag(Lc) > 0.0)
    Ll = Lc.astype(jp.LD)
    res = np.abs((Ll @ Ll.T).astype(float) - got["cov"])
    bound = 2 * (pm + 1) * EPS * (np.abs(Lc) @ np.abs(Lc).T)
    print("n = %d [%s]: max |Lc Lc^T - cov| / bound %.3f" % (n, route, float(np.max(res / bound))))
    assert np.all(res <= bound)


# ---- 4. the draws ------------------------------------------------------------------------------------------------------------
def _raw(c, t, yy, alpha, l, sigma, jitter, ts, orders, pj, mean, cov, Z, B, draws, n=None, m=None, ldc=None, ldz=None, ldd=None):
    """gpmi_joint_predict with every argument as given (no checks of the Python layer in front); None: NULL."""
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    pm = bin(orders & 7).count("1") * int(ts.size if m is None else m)
    return c._lib.gpmi_joint_predict(
        c._h, p(t), int(t.size if n is None else n), p(yy), C.c_double(alpha), C.c_double(l), C.c_double(sigma), C.c_double(jitter),
        p(ts), int(ts.size if m is None else m), int(orders), p(pj), p(mean), p(cov), int(pm if ldc is None else ldc), p(Z), int(B),
        int(pm if ldz is None else ldz), p(draws), int(pm if ldd is None else ldd))


_EDGE_DRAWS = {}
EDGE_B = (1, 5, 16, 17, 33)


@pytest.mark.parametrize("route", ["chain", "wg"])
@pytest.mark.parametrize("B", EDGE_B)
def test_draws_against_the_long_double_product(ctx, octx, B, route):
    """The 129-point case, orders = 7 (pm = 258: ragged against 16, three 128-row blocks), padded leading dimensions with
    sentinels, and every draw within 2 (pm + 2) eps (|Lc| |Z| + |mean|) of the long-double mean + Lc Z: (pm + 1) eps |Lc| |Z|
    for a sum of pm products in any order, one eps for the addition of the mean, times 2; Lc is the factor of test 3.  The call
    is made twice (identical bits), and column b has the bits it had with every other B."""
    n = 129
    case = CASE[n]
    t, yy, ts = jp.inputs(case)
    Lc, ref = _factor(ctx, octx, n, route)
    c = _route(ctx, octx, route)
    pm = Lc.shape[0]
    Zall = np.random.default_rng(258).standard_normal((pm, max(EDGE_B)))
    ldz, ldd, ldc = pm + 3, pm + 5, pm + 1
    pj = jp.post_jitter(case[1], 7)
    runs = []
    for _ in range(2):
        Z = np.full((ldz, B), SENT, order="F"); Z[:pm] = Zall[:, :B]
        draws = np.full((ldd, B), SENT, order="F")
        cov = np.full((ldc, pm), SENT, order="F")
        mean = np.full(pm + 1, SENT)
        rc = _raw(c, t, yy, ALPHA, case[1], SIGMA, JITTER, ts, 7, pj, mean, cov, Z, B, draws, ldc=ldc, ldz=ldz, ldd=ldd)
        assert rc == 0
        assert mean[pm] == SENT and np.all(cov[pm:] == SENT) and np.all(draws[pm:] == SENT) and np.all(Z[pm:] == SENT)
        runs.append((mean[:pm].copy(), cov[:pm].copy(), draws[:pm].copy()))
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)
    mean, cov, draws = runs[0]
    np.testing.assert_array_equal(mean, ref["mean"])
    np.testing.assert_array_equal(cov, ref["cov"])
    want = ref["mean"].astype(jp.LD)[:, None] + Lc.astype(jp.LD) @ Zall[:, :B].astype(jp.LD)
    bound = 2 * (pm + 2) * EPS * (np.abs(Lc) @ np.abs(Zall[:, :B]) + np.abs(ref["mean"])[:, None])
    err = np.abs((draws.astype(jp.LD) - want).astype(float))
    print("B = %d [%s]: max error / bound %.3f" % (B, route, float(np.max(err / bound))))
    assert np.all(err <= bound)
    _EDGE_DRAWS[(route, B)] = draws
    for (r, other), d in _EDGE_DRAWS.items():   # column b has the same bits whatever B is
        if r == route:
            k = min(other, B)
            np.testing.assert_array_equal(d[:, :k], draws[:, :k])


# ---- 5. status ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["chain", "wg"])
def test_s_not_positive_definite(ctx, octx, route):
    c = _route(ctx, octx, route)
    n, m = 20, 9
    rng = np.random.default_rng(5)
    t = rng.uniform(-1, 1, n)
    t[10:15] = t[9]   # six copies of one time, no noise, no jitter: S is singular
    ts = rng.uniform(-1, 1, m)
    yy = rng.standard_normal(2 * n)
    Z = rng.standard_normal((3 * m, 3))
    got = c.joint_predict(t, yy, 1.0, 0.4, 0.0, 0.0, ts, 7, (1e-6, 1e-5, 1e-4), Z=Z)
    assert 1 <= got["info"] <= 2 * n
    assert np.all(np.isnan(got["mean"])) and np.all(np.isnan(got["cov"])) and np.all(np.isnan(got["draws"]))


@pytest.mark.parametrize("block", [0, 2])
@pytest.mark.parametrize("route", ["chain", "wg"])
def test_covariance_not_positive_definite(ctx, octx, route, block):
    """A negative post_jitter on one order block of the 21-point case: -1 on f (its posterior variance there is far below 1), and
    on f'' minus (1 + its prior variance 3 alpha^2 / l^4), so that the block's diagonal is negative in either case."""
    n = 21
    c = _route(ctx, octx, route)
    m = jp.case_m(CASE[n])
    pj = jp.post_jitter(CASE[n][1], 7)
    pj[block] = -1.0 if block == 0 else -1.0 - 3 * ALPHA ** 2 / CASE[n][1] ** 4
    Z = np.random.default_rng(1).standard_normal((3 * m, 4))
    bad = _call(c, n, 7, Z=Z, pj=pj)
    ref = _call(c, n, 7, pj=pj)
    assert ref["info"] == 0   # B = 0: C is not factored
    assert 2 * n + 1 <= bad["info"] <= 2 * n + 3 * m
    np.testing.assert_array_equal(bad["mean"], ref["mean"])
    np.testing.assert_array_equal(bad["cov"], ref["cov"])
    assert np.all(np.isfinite(bad["cov"])) and np.all(np.diag(bad["cov"])[block * m:(block + 1) * m] < 0)
    assert np.all(np.isnan(bad["draws"]))


# ---- 6. the device form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,route,want_cov", [(21, "wg", True), (21, "wg", False), (129, "chain", True), (129, "chain", False)])
def test_dev_equals_host(ctx, octx, n, route, want_cov):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    c = _route(ctx, octx, route)
    case = CASE[n]
    t, yy, ts = jp.inputs(case)
    m, B, mask = ts.size, 5, 7
    pm = 3 * m
    pj = jp.post_jitter(case[1], mask)
    Z = np.asfortranarray(np.random.default_rng(m).standard_normal((pm, B)))
    host = _call(c, n, mask, Z=Z)
    ldc, ldz, ldd = pm + 2, pm + 1, pm + 3
    dt, dyy, dts = (torch.from_numpy(a).to(dev) for a in (t, yy, ts))
    Zp = np.full((B, ldz), SENT); Zp[:, :pm] = Z.T
    dZ = torch.from_numpy(Zp).to(dev)
    dmean = torch.full((pm + 1,), SENT, dtype=torch.float64, device=dev)
    dcov = torch.full((pm, ldc), SENT, dtype=torch.float64, device=dev)
    ddraws = torch.full((B, ldd), SENT, dtype=torch.float64, device=dev)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    c.joint_predict_dev(dt.data_ptr(), n, dyy.data_ptr(), ALPHA, case[1], SIGMA, JITTER, dts.data_ptr(), m, mask, pj, dmean.data_ptr(),
                        dcov.data_ptr() if want_cov else None, ldc, dZ.data_ptr(), B, ldz, ddraws.data_ptr(), ldd, info.data_ptr())
    c.sync()
    assert int(info.item()) == 0
    mean = dmean.cpu().numpy(); cov = dcov.cpu().numpy().T; draws = ddraws.cpu().numpy().T
    np.testing.assert_array_equal(mean[:pm], host["mean"])
    np.testing.assert_array_equal(draws[:pm], host["draws"])
    assert mean[pm] == SENT and np.all(draws[pm:] == SENT)
    if want_cov:
        np.testing.assert_array_equal(cov[:pm], host["cov"])
        assert np.all(cov[pm:] == SENT)
    else:
        assert np.all(cov == SENT)   # no covariance asked for: the buffer beside the call is not touched
    # B = 0 with NULL Z / draws
    dmean.fill_(SENT); info.fill_(-7)
    torch.cuda.synchronize(dev)
    c.joint_predict_dev(dt.data_ptr(), n, dyy.data_ptr(), ALPHA, case[1], SIGMA, JITTER, dts.data_ptr(), m, mask, pj, dmean.data_ptr(),
                        None, ldc, None, 0, ldz, None, ldd, info.data_ptr())
    c.sync()
    assert int(info.item()) == 0
    np.testing.assert_array_equal(dmean.cpu().numpy()[:pm], host["mean"])


# ---- 7. bad arguments --------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_earg_and_write_nothing(ctx, octx):
    n, m, B, mask = 12, 9, 2, 7
    pm = 3 * m
    rng = np.random.default_rng(2)
    t, ts, yy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m), rng.standard_normal(2 * n)
    Z = np.asfortranarray(rng.standard_normal((pm, B)))
    pj0 = np.array([1e-6, 1e-5, 1e-4])

    def run(null=(), **kw):
        mean = np.full(pm, SENT); cov = np.full((pm, pm), SENT, order="F"); draws = np.full((pm, B), SENT, order="F")
        a = dict(t=t, yy=yy, alpha=1.0, l=0.5, sigma=0.1, jitter=1e-6, ts=ts, orders=mask, pj=pj0, mean=mean, cov=cov, Z=Z, B=B,
                 draws=draws)
        a.update(dict(n=n, m=m, ldc=pm, ldz=pm, ldd=pm))   # the sizes do not come from a pointer that may be NULL
        a.update(kw)
        for k in null:
            a[k] = None
        rc = _raw(ctx, a.pop("t"), a.pop("yy"), a.pop("alpha"), a.pop("l"), a.pop("sigma"), a.pop("jitter"), a.pop("ts"),
                  a.pop("orders"), a.pop("pj"), a.pop("mean"), a.pop("cov"), a.pop("Z"), a.pop("B"), a.pop("draws"), **a)
        assert np.all(mean == SENT) and np.all(cov == SENT) and np.all(draws == SENT), (null, kw)
        return rc

    for kw in (dict(n=0), dict(m=0), dict(B=-1), dict(orders=0), dict(orders=8), dict(ldc=pm - 1), dict(ldz=pm - 1), dict(ldd=pm - 1),
               dict(alpha=0.0), dict(alpha=-1.0), dict(l=0.0), dict(l=-0.5), dict(l=np.inf), dict(l=np.nan), dict(sigma=-0.1),
               dict(pj=np.array([1e-6, np.inf, 1e-4])), dict(pj=np.array([np.nan, 1e-5, 1e-4]))):
        assert run(**kw) == -1, kw
    for null in (("t",), ("yy",), ("ts",), ("pj",), ("mean",), ("Z",), ("draws",)):
        assert run(null=null) == -1, null
    good = ctx.joint_predict(t, yy, 1.0, 0.5, 0.1, 1e-6, ts, mask, pj0, Z=Z)
    assert good["info"] == 0
    # NULL Z / draws are fine when B == 0, and so is a NULL cov; a negative post_jitter is an argument like any other
    mean = np.full(pm, SENT)
    assert _raw(ctx, t, yy, 1.0, 0.5, 0.1, 1e-6, ts, mask, pj0, mean, None, None, 0, None) == 0
    np.testing.assert_array_equal(mean, good["mean"])
    assert ctx.joint_predict(t, yy, 1.0, 0.5, 0.1, 1e-6, ts, mask, -pj0)["info"] == 0
    for value in (-1, 1025):
        assert octx._lib.gpmi_set_option(octx._h, b"small_jp", value) == -1
    assert octx._lib.gpmi_set_option(octx._h, b"small_jp", 1024) == 0
