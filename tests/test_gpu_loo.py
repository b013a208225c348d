"""GPU: gpmi_logml_loo[_dev], exact leave-one-out cross-validation with gradient, on the two chain routes of
tests/test_gpu_logml_grad_parity.py (`aug`: the augmented factorisation; `chains`: the three chains) -- there is no
one-workgroup form.  Against the long-double reference of tests/loo_reference.py (gradient by R&W (5.13), one product per
hyper-parameter: not the device's identity) within its bounds, no tolerance of this file's own; against gpmi_gp_predict on the
data without the point (no leave-one-out formula at all); and against itself: across routes, calls, forms, NULL outputs and
workspace histories, bit for bit wherever the same kernels run.

The one bound that is not loo_reference's: gpmi_gp_predict's own tolerances (tests/predict_reference.py: MEAN_TOL relative
to the scale of the means, here max|y|; VAR_TOL of the prior variance alpha^2), added to the LOO bound where the two device
results are compared."""
import ctypes as C

import numpy as np
import pytest

import logml_grad_reference as lg
import loo_reference as lr
import predict_reference as pr
from test_gpu_logml_grad_parity import GRID_A, GRID_R, GRID_S, BAD, aug, chains  # noqa: F401  (fixtures: the contexts)

pytestmark = pytest.mark.gpu

EARG = -1
PAD = 1e3   # rows n .. ldx of X when ldx > n: never read into a result
# "chains_ncu8": the three chains with the trailing-update planner made to see 8 compute units ("debug_ncu"), so that the
# symmetric product -M M^T of the gradient (launch_syrk_ppt, the trailing update's launch) and the updates of the factorisation
# take their multi-round paths at NCU8_CASE, n = 705 (21 tiles on 16 workgroup slots); the catalogue itself stops at n = 385
ROUTES = ("aug", "chains", "chains_ncu8")
NCU8_CASE = (705, 2, False, 0.15, "")
PARITY = [(r, c) for r in ROUTES for c in lr.CASES] + [("chains_ncu8", NCU8_CASE)]
KEYS = ("out3", "loo", "mu", "var", "lpd", "grad")


@pytest.fixture(scope="module")
def chains_ncu8():
    from test_gpu_logml_grad_parity import ROUTES as GRAD_ROUTES, _context
    c = _context(dict(GRAD_ROUTES["chains"], debug_ncu=8))
    yield c
    c.close()


@pytest.fixture
def routes(aug, chains, chains_ncu8):  # noqa: F811  (this file's routes: the two chain routes and the debug_ncu one)
    return {"aug": aug, "chains": chains, "chains_ncu8": chains_ncu8}


def _check(tag, got, ref, cond, scale=1.0):
    """Print the worst error / bound per quantity (ARD components one by one inside `grad`) and assert each <= 1."""
    r = lr.ratios(got, ref, cond, scale)
    print("%s: cond %.1e; error / bound: %s" % (tag, cond, ", ".join("%s %.3f" % kv for kv in r.items())))
    for key in ("mu", "var", "lpd", "grad"):
        if got.get(key) is not None:
            assert np.all(np.isfinite(got[key])), (tag, key)
    for key, v in r.items():
        assert v <= 1.0, (tag, key, v)
    return r


def _same(a, b, keys=KEYS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in keys)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _raw_grad(c, X, y, a, ell, s, jit):
    """gpmi_logml_grad without the binding's exception for k > 0: (status, out3, grad)."""
    X = np.asfortranarray(X); y = np.ascontiguousarray(y); ell = np.ascontiguousarray(ell, dtype=float)
    n, D = X.shape
    out, g = np.empty(3), np.empty(2 + ell.size)
    rc = c._lib.gpmi_logml_grad(c._h, _p(X), n, n, D, _p(y), C.c_double(a), _p(ell), ell.size, C.c_double(s), C.c_double(jit),
                                _p(out), _p(g))
    return rc, out, g


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def _loo_dev(c, X, y, a, ell, s, jit, ldx=None, odd=False, want=("mu", "var", "lpd", "grad")):
    """gpmi_logml_loo_dev into sentinel-filled device buffers -> the dict of Context.logml_loo.  ldx > n: the rows below hold PAD;
    odd: X starts one double past the (256-byte aligned) allocation."""
    torch, dev = _torch()
    n, D = X.shape
    ldx = n if ldx is None else ldx
    ell = np.atleast_1d(np.asarray(ell, float))
    Xt = np.full(D * ldx + 1, PAD)
    Xt[int(odd):int(odd) + D * ldx].reshape(D, ldx)[:, :n] = X.T
    dX = torch.from_numpy(Xt).to(dev)
    dy = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    size = {"out3": 3, "loo": 1, "mu": n, "var": n, "lpd": n, "grad": 2 + ell.size}
    d = {k: torch.full((size[k],), -5.0, dtype=torch.float64, device=dev) for k in KEYS}
    di = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ptr = lambda k: d[k].data_ptr() if (k in want or k in ("out3", "loo")) else 0
    torch.cuda.synchronize()
    c.logml_loo_dev(dX.data_ptr() + 8 * int(odd), n, ldx, D, dy.data_ptr(), a, ell, s, jit, ptr("out3"), ptr("loo"), ptr("mu"),
                    ptr("var"), ptr("lpd"), ptr("grad"), di.data_ptr())
    c.sync()
    out = {k: d[k].cpu().numpy() for k in KEYS}
    for k in ("mu", "var", "lpd", "grad"):
        if k not in want:
            assert np.all(out[k] == -5.0), k      # a NULL output's neighbour buffers are not written either
            out[k] = None
    out["loo"] = float(out["loo"][0])
    out["info"] = int(di.cpu()[0])
    return out


# ---- 1. parity with long double -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,case", PARITY, ids=["%s-%s" % (r, lg.case_id(c)) for r, c in PARITY])
def test_parity_with_long_double(routes, route, case):
    c = routes[route]
    (X, y, a, ell, s, jit), ref, cond = lr.parity_reference(case)
    got = c.logml_loo(X, y, a, ell, s, jit)
    assert got["info"] == 0 and got["grad"].shape == (2 + ell.size,) and got["mu"].shape == (case[0],)
    _check("%s %s" % (route, lg.case_id(case)), got, ref, cond)
    assert np.all(got["var"] > 0)
    if s == 0.0:
        assert got["grad"][-1] == 0.0     # 2 sigma tr(G): exactly zero, not a rounding residue
    # the same build, factorisation and finalize as gpmi_logml_grad on this context and route
    out, _ = c.logml_grad(X, y, a, ell, s, jit)
    assert np.array_equal(got["out3"], out), (got["out3"], out)


@pytest.mark.parametrize("case", lr.CASES, ids=lg.case_id)
def test_two_routes_agree(routes, case):
    (X, y, a, ell, s, jit), ref, cond = lr.parity_reference(case)
    g1 = routes["aug"].logml_loo(X, y, a, ell, s, jit)
    g2 = routes["chains"].logml_loo(X, y, a, ell, s, jit)
    other = dict(ref, **{k: np.asarray(g2[k], np.longdouble) for k in ("mu", "var", "lpd", "loo", "grad")})
    # the bounds are those of the reference (its y, var, gabs), the values compared are the other route's
    e = lr.errors(g1, other)
    b = lr.bounds(ref, cond, 2.0)
    for k in e:
        assert np.all(e[k] <= b[k]), (k, np.max(e[k] / np.where(np.asarray(b[k]) > 0, b[k], 1.0)))


# ---- 2. independent of any formula: the model refitted without the point ----------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case,idx", lr.DELETE_CASES, ids=[lg.case_id(c) for c, _ in lr.DELETE_CASES])
def test_points_equal_gp_predict_without_the_point(routes, route, case, idx):
    c = routes[route]
    (X, y, a, ell, s, jit), ref, cond = lr.delete_reference(case)
    got = c.logml_loo(X, y, a, ell, s, jit, want_grad=False)
    assert got["info"] == 0 and got["grad"] is None
    _check("%s %s" % (route, lg.case_id(case)), got, ref, cond)
    b = lr.bounds(ref, cond)
    bmean, bvar = pr.MEAN_TOL * float(np.max(np.abs(y))), pr.VAR_TOL * a * a
    for i in idx:
        keep = np.delete(np.arange(case[0]), i)
        p = c.gp_predict(X[keep], y[keep], a, ell, s, jit, X[i:i + 1])
        assert p["info"] == 0
        em, ev = abs(p["mean"][0] - got["mu"][i]), abs(p["var"][0] + s * s + jit - got["var"][i])
        print("i = %d: mean error / bound %.3f, var %.3f" % (i, em / (b["mu"][i] + bmean), ev / (b["var"][i] + bvar)))
        assert em <= b["mu"][i] + bmean, (i, p["mean"][0], got["mu"][i])
        assert ev <= b["var"][i] + bvar, (i, p["var"][0] + s * s + jit, got["var"][i])


# ---- 3. bits ------------------------------------------------------------------------------------------------------------
BITS_CASES = {"aug": (129, 33, True, 0.0, ""), "chains": (129, 8, True, 1e-3, ""), "chains_ncu8": (129, 8, True, 1e-3, "")}
WORKSPACE_CASES = dict(BITS_CASES, chains_ncu8=NCU8_CASE)   # ... where its launches are multi-round


@pytest.mark.parametrize("route", ROUTES)
def test_repeated_calls_forms_and_null_outputs_give_identical_bits(routes, route):
    c = routes[route]
    case = BITS_CASES[route]
    assert case in lr.CASES
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    r0 = c.logml_loo(X, y, a, ell, s, jit)
    assert r0["info"] == 0 and all(np.all(np.isfinite(r0[k])) for k in KEYS)
    assert _same(r0, c.logml_loo(X, y, a, ell, s, jit))
    d0 = _loo_dev(c, X, y, a, ell, s, jit)
    assert d0["info"] == 0 and _same(r0, d0)
    # without the gradient (no SYRK, no contraction) and with any of mu, var, lpd NULL: the remaining outputs keep their bits
    for outputs, want_grad in ((("mu", "var", "lpd"), False), ((), True), (("var",), True), (("mu", "lpd"), False)):
        keys = ("out3", "loo") + outputs + (("grad",) if want_grad else ())
        r = c.logml_loo(X, y, a, ell, s, jit, want_grad=want_grad, outputs=outputs)
        assert all(r[k] is None for k in KEYS if k not in keys)
        assert _same(r0, r, keys), (outputs, want_grad)
        d = _loo_dev(c, X, y, a, ell, s, jit, want=outputs + (("grad",) if want_grad else ()))
        assert _same(r0, d, keys), (outputs, want_grad)


@pytest.mark.parametrize("route", ROUTES)
def test_results_do_not_depend_on_what_the_workspace_held(routes, route):
    """n = 129 on both routes, n = 705 on the debug_ncu one: after every double of the context's scratch was a NaN (0xFF) and
    1.38e306 (0x7F)."""
    c = routes[route]
    X, y, a, ell, s, jit = lg.case_inputs(*WORKSPACE_CASES[route])
    r0 = c.logml_loo(X, y, a, ell, s, jit)
    assert c.debug_counters() == 0
    for byte in (0xFF, 0x7F):
        c.debug_fill(byte)
        r = c.logml_loo(X, y, a, ell, s, jit)
        assert _same(r0, r), hex(byte)
        assert c.debug_counters() == 0
        c.debug_fill(byte)
        assert _same(r0, _loo_dev(c, X, y, a, ell, s, jit)), hex(byte)
        assert c.debug_counters() == 0


@pytest.mark.parametrize("route", ROUTES)
def test_dev_form_with_a_leading_dimension_past_n_and_an_odd_offset(routes, route):
    c = routes[route]
    case = BITS_CASES[route]
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    d0 = _loo_dev(c, X, y, a, ell, s, jit)
    assert _same(d0, _loo_dev(c, X, y, a, ell, s, jit, ldx=case[0] + 3))
    assert _same(d0, _loo_dev(c, X, y, a, ell, s, jit, odd=True))
    assert _same(d0, _loo_dev(c, X, y, a, ell, s, jit, ldx=case[0] + 5, odd=True))


# ---- 4. not positive definite ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_not_positive_definite_is_a_status_and_the_context_goes_on(routes, route):
    """The point the gradient grids reject (rho = 50, sigma = 1e-9, no jitter, coincident points)."""
    c = routes[route]
    X, y = lg.case_inputs(129, 9, False, 0.15, "dup")[:2]
    a, ell, s = float(GRID_A[BAD]), [float(GRID_R[BAD])], float(GRID_S[BAD])
    rc, out, g = _raw_grad(c, X, y, a, ell, s, 0.0)
    assert rc > 0 and np.all(np.isnan(g))
    for form in ("host", "dev"):
        r = c.logml_loo(X, y, a, ell, s, 0.0) if form == "host" else _loo_dev(c, X, y, a, ell, s, 0.0)
        assert r["info"] == rc, (form, r["info"], rc)
        assert np.array_equal(r["out3"], out, equal_nan=True), (form, r["out3"], out)
        assert np.isnan(r["loo"]) and all(np.all(np.isnan(r[k])) for k in ("mu", "var", "lpd", "grad")), form
        assert r["grad"].shape == (3,) and r["mu"].shape == (129,)
    # the next call on the same context is correct
    case = BITS_CASES[route]
    (X, y, a, ell, s, jit), ref, cond = lr.parity_reference(case)
    _check("%s after a failed call" % route, c.logml_loo(X, y, a, ell, s, jit), ref, cond)


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(aug):
    c = aug
    lib, h = c._lib, c._h
    n, D = 5, 2
    X = np.asfortranarray(np.random.default_rng(5).random((n, D))); y = np.ones(n); ell = np.array([0.5, 0.7])
    out, loo, mu, var, lpd, g = np.empty(3), np.empty(1), np.empty(n), np.empty(n), np.empty(n), np.empty(2 + D)
    d = C.c_double

    def host(X=X, n=n, ldx=n, D=D, y=y, alpha=1.0, ell=ell, n_ell=D, sigma=0.1, out=out, loo=loo):
        q = lambda v: None if v is None else _p(v)
        return lib.gpmi_logml_loo(h, q(X), n, ldx, D, q(y), d(alpha), q(ell), n_ell, d(sigma), d(0.0), q(out), q(loo), _p(mu),
                                  _p(var), _p(lpd), _p(g))

    assert host() == 0
    for kw in ({"n": 0, "ldx": 0}, {"n": -1}, {"D": 0}, {"D": 65}, {"ldx": n - 1}, {"alpha": 0.0}, {"alpha": -1.0},
               {"ell": np.array([0.5, 0.0])}, {"ell": np.array([-0.5]), "n_ell": 1}, {"sigma": -0.1}, {"X": None}, {"y": None},
               {"ell": None}, {"out": None}, {"loo": None}, {"n_ell": 3}):
        assert host(**kw) == EARG, kw
        assert c._lib.gpmi_last_error()
    # the device-resident form checks before it touches anything: the pointers are never dereferenced
    torch, dev = _torch()
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    P = buf.data_ptr()

    def devf(dX=P, n=n, ldx=n, D=D, dy=P, alpha=1.0, ell=ell, n_ell=D, sigma=0.1, dout=P, dloo=P, dinfo=info.data_ptr()):
        v = lambda p: C.c_void_p(p) if p else None
        return lib.gpmi_logml_loo_dev(h, v(dX), n, ldx, D, v(dy), d(alpha), None if ell is None else _p(ell), n_ell, d(sigma), d(0.0),
                                      v(dout), v(dloo), None, None, None, None, v(dinfo))

    for kw in ({"n": 0}, {"D": 0}, {"D": 65}, {"ldx": n - 1}, {"alpha": 0.0}, {"ell": np.array([0.5, 0.0])}, {"sigma": -0.1},
               {"dX": 0}, {"dy": 0}, {"ell": None}, {"dout": 0}, {"dloo": 0}, {"dinfo": 0}):
        assert devf(**kw) == EARG, kw
    c.sync()
