"""GPU: gpmi_logml_hess[_dev], the exact Hessian of the log marginal likelihood in (alpha, ell.., sigma), on the two chain routes
of tests/test_gpu_logml_grad_parity.py (`aug`: the augmented factorisation; `chains`: the three chains) -- there is no
one-workgroup form.  Against the long-double reference of tests/hess_reference.py (one product per hyper-parameter, no closed
form) within its bound, entry by entry, no tolerance of this file's own; against central differences of the device's own
gpmi_logml_grad (no Hessian formula at all) within bounds that are all derived; and against itself: across calls, forms, a NULL
gradient, workspace histories, leading dimensions and offsets, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import hess_reference as hr
import logml_grad_reference as lg
from test_gpu_logml_grad_parity import GRID_A, GRID_R, GRID_S, BAD, aug, chains, one_wg, routes  # noqa: F401  (fixtures: the contexts)

pytestmark = pytest.mark.gpu

EARG = -1
PAD = 1e3        # rows n .. ldx of X when ldx > n: never read into a result
SENTINEL = -5.0
ROUTES = ("aug", "chains")
PARITY = [(r, c) for r in ROUTES for c in hr.HESS_CASES]
KEYS = ("out3", "grad", "hess")
BITS_CASES = {"aug": (129, 8, True, 1e-3, ""), "chains": (129, 16, False, 0.15, "")}


def _same(a, b, keys=KEYS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in keys)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def _raw_grad(c, X, y, a, ell, s, jit):
    """gpmi_logml_grad without the binding's exception for k > 0: (status, out3, grad)."""
    X = np.asfortranarray(X); y = np.ascontiguousarray(y); ell = np.ascontiguousarray(ell, dtype=float)
    n, D = X.shape
    out, g = np.empty(3), np.empty(2 + ell.size)
    rc = c._lib.gpmi_logml_grad(c._h, _p(X), n, n, D, _p(y), C.c_double(a), _p(ell), ell.size, C.c_double(s), C.c_double(jit),
                                _p(out), _p(g))
    return rc, out, g


def _hess_dev(c, X, y, a, ell, s, jit, ldx=None, odd=False, pad=0, want_grad=True):
    """gpmi_logml_hess_dev into sentinel-filled device buffers -> the dict of Context.logml_hess.  ldx > n: the rows below hold
    PAD; odd: X starts one double past the (256-byte aligned) allocation; pad: ldh = q + pad, and the padding rows must keep the
    sentinel."""
    torch, dev = _torch()
    n, D = X.shape
    ldx = n if ldx is None else ldx
    ell = np.atleast_1d(np.asarray(ell, float))
    q = 2 + ell.size
    ldh = q + pad
    Xt = np.full(D * ldx + 1, PAD)
    Xt[int(odd):int(odd) + D * ldx].reshape(D, ldx)[:, :n] = X.T
    dX = torch.from_numpy(Xt).to(dev)
    dy = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    size = {"out3": 3, "grad": q, "hess": ldh * q}
    d = {k: torch.full((size[k],), SENTINEL, dtype=torch.float64, device=dev) for k in KEYS}
    di = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c.logml_hess_dev(dX.data_ptr() + 8 * int(odd), n, ldx, D, dy.data_ptr(), a, ell, s, jit, d["out3"].data_ptr(),
                     d["grad"].data_ptr() if want_grad else 0, d["hess"].data_ptr(), ldh, di.data_ptr())
    c.sync()
    out = {k: d[k].cpu().numpy() for k in KEYS}
    full = out["hess"].reshape(q, ldh).T    # column-major (ldh x q)
    assert np.all(full[q:] == SENTINEL)     # nothing outside the q rows of a column is written
    out["hess"] = np.asfortranarray(full[:q])
    if not want_grad:
        assert np.all(out["grad"] == SENTINEL)
        out["grad"] = None
    out["info"] = int(di.cpu()[0])
    return out


def _check(tag, H, ref, cond):
    """Print error / bound (worst entry) and assert every entry within its bound."""
    assert np.all(np.isfinite(H)), tag
    e, b = hr.errors(H, ref), hr.bounds(ref, cond)
    r = hr.ratio(H, ref, cond)
    print("%s: cond %.1e; hmax %.3e; error / bound %.3f" % (tag, cond, ref["hmax"], r))
    assert np.all(e <= b), (tag, r)


# ---- 1. parity with long double -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,case", PARITY, ids=["%s-%s" % (r, lg.case_id(c)) for r, c in PARITY])
def test_parity_with_long_double(routes, route, case):
    c = routes[route]
    (X, y, a, ell, s, jit), ref, cond = hr.parity_reference(case)
    got = c.logml_hess(X, y, a, ell, s, jit)
    q = 2 + ell.size
    assert got["info"] == 0 and got["hess"].shape == (q, q) and got["grad"].shape == (q,)
    _check("%s %s" % (route, lg.case_id(case)), got["hess"], ref, cond)
    assert np.array_equal(got["hess"], got["hess"].T)
    if s == 0.0:   # the sigma row: 2 tr G on the diagonal, exact zeros beside it
        assert np.all(got["hess"][-1, :-1] == 0.0) and got["hess"][-1, -1] != 0.0
    # the same chain and the same contraction as gpmi_logml_grad on this context and route
    out, g = c.logml_grad(X, y, a, ell, s, jit)
    assert np.array_equal(got["out3"], out), (got["out3"], out)
    assert np.array_equal(got["grad"], g), (got["grad"], g)


# ---- 2. bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_repeated_calls_forms_and_a_null_gradient_give_identical_bits(routes, route):
    c = routes[route]
    case = BITS_CASES[route]
    assert case in hr.HESS_CASES
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    r0 = c.logml_hess(X, y, a, ell, s, jit)
    assert r0["info"] == 0 and all(np.all(np.isfinite(r0[k])) for k in KEYS)
    assert np.array_equal(r0["hess"], r0["hess"].T)
    assert _same(r0, c.logml_hess(X, y, a, ell, s, jit))
    d0 = _hess_dev(c, X, y, a, ell, s, jit)
    assert d0["info"] == 0 and _same(r0, d0)
    assert _same(r0, _hess_dev(c, X, y, a, ell, s, jit, pad=3))
    r = c.logml_hess(X, y, a, ell, s, jit, want_grad=False)
    assert r["grad"] is None and _same(r0, r, ("out3", "hess"))
    d = _hess_dev(c, X, y, a, ell, s, jit, want_grad=False, pad=3)
    assert d["grad"] is None and _same(r0, d, ("out3", "hess"))
    assert c.debug_counters() == 0


@pytest.mark.parametrize("route", ROUTES)
def test_results_do_not_depend_on_what_the_workspace_held(routes, route):
    """n = 129 on both routes: after every double of the context's scratch was a NaN (0xFF) and 1.38e306 (0x7F)."""
    c = routes[route]
    X, y, a, ell, s, jit = lg.case_inputs(*BITS_CASES[route])
    r0 = c.logml_hess(X, y, a, ell, s, jit)
    assert c.debug_counters() == 0
    for byte in (0xFF, 0x7F):
        c.debug_fill(byte)
        assert _same(r0, c.logml_hess(X, y, a, ell, s, jit)), hex(byte)
        assert c.debug_counters() == 0
        c.debug_fill(byte)
        assert _same(r0, _hess_dev(c, X, y, a, ell, s, jit)), hex(byte)
        assert c.debug_counters() == 0


@pytest.mark.parametrize("route", ROUTES)
def test_dev_form_with_a_leading_dimension_past_n_and_an_odd_offset(routes, route):
    c = routes[route]
    case = BITS_CASES[route]
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    d0 = _hess_dev(c, X, y, a, ell, s, jit)
    assert _same(d0, _hess_dev(c, X, y, a, ell, s, jit, ldx=case[0] + 3))
    assert _same(d0, _hess_dev(c, X, y, a, ell, s, jit, odd=True))
    assert _same(d0, _hess_dev(c, X, y, a, ell, s, jit, ldx=case[0] + 5, odd=True))


# ---- 3. no Hessian formula: central differences of the device's own gradient ------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_columns_equal_central_differences_of_the_device_gradient(routes, route):
    """Column k against (grad(theta + h_k e_k) - grad(theta - h_k e_k)) / (2 h_k), h_k = 1e-4 max(|theta_k|, 1e-3), within the
    sum of: the two gradients' bounds (lg.bounds at the two points) over 2 h_k, the truncation of the same stencil in long
    double, and the Hessian's own bound."""
    c = routes[route]
    (X, y, a, ell, s, jit), theta, h, ref, cond, trunc, gb = hr.fd_reference(hr.FD_CASE)
    got = c.logml_hess(X, y, a, ell, s, jit)
    assert got["info"] == 0
    F = hr.fd_hessian(lambda t: c.logml_grad(X, y, t[0], t[1:-1], t[-1], jit)[1], theta, h)
    bound = gb + trunc + hr.bounds(ref, cond)
    err = np.abs(F - got["hess"])
    print("%s: |FD - H| / bound %.3f (gradient bounds %.2e, truncation %.2e, Hessian bound %.2e of hmax)" % (
        route, float(np.max(err / bound)), float(np.max(gb)) / ref["hmax"], float(np.max(trunc)) / ref["hmax"],
        float(np.max(hr.bounds(ref, cond))) / ref["hmax"]))
    assert np.all(err <= bound), err / bound


# ---- 4. not positive definite ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_not_positive_definite_is_a_status_and_the_context_goes_on(routes, route):
    """The point the gradient grids reject (rho = 50, sigma = 1e-9, no jitter, coincident points)."""
    c = routes[route]
    case = BITS_CASES[route]
    before = c.logml_hess(*lg.case_inputs(*case))
    X, y = lg.case_inputs(129, 9, False, 0.15, "dup")[:2]
    a, ell, s = float(GRID_A[BAD]), [float(GRID_R[BAD])], float(GRID_S[BAD])
    rc, out, g = _raw_grad(c, X, y, a, ell, s, 0.0)
    assert rc > 0 and np.all(np.isnan(g))
    for form in ("host", "dev"):
        r = c.logml_hess(X, y, a, ell, s, 0.0) if form == "host" else _hess_dev(c, X, y, a, ell, s, 0.0, pad=2)
        assert r["info"] == rc, (form, r["info"], rc)
        assert np.array_equal(r["out3"], out, equal_nan=True), (form, r["out3"], out)
        assert r["grad"].shape == (3,) and r["hess"].shape == (3, 3)
        assert np.all(np.isnan(r["grad"])) and np.all(np.isnan(r["hess"])), form
    # a healthy call straight after has the bits it had before
    assert _same(before, c.logml_hess(*lg.case_inputs(*case)))


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(aug):
    c = aug
    lib, h = c._lib, c._h
    n, D = 5, 2
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.random((n, D))); y = np.ones(n); ell = np.array([0.5, 0.7])
    X9 = np.asfortranarray(rng.random((n, 9))); ell9 = np.full(9, 0.6)
    d = C.c_double
    out, g, H = np.empty(3), np.empty(11), np.empty(11 * 11)

    def fill():
        for v in (out, g, H):
            v.fill(SENTINEL)

    def untouched():
        return all(np.all(v == SENTINEL) for v in (out, g, H))

    def host(X=X, n=n, ldx=n, D=D, y=y, alpha=1.0, ell=ell, n_ell=D, sigma=0.1, out=out, H=H, ldh=None):
        q = lambda v: None if v is None else _p(v)
        return lib.gpmi_logml_hess(h, q(X), n, ldx, D, q(y), d(alpha), q(ell), n_ell, d(sigma), d(0.0), q(out), _p(g), q(H),
                                   2 + n_ell if ldh is None else ldh)

    fill()
    assert host() == 0 and not untouched()
    assert host(X=X9, D=9, ell=np.array([0.6]), n_ell=1) == 0      # one length-scale: any D
    for kw in ({"X": X9, "D": 9, "ell": ell9, "n_ell": 9}, {"ldh": 3}, {"n": 0, "ldx": 0}, {"n": -1}, {"ldx": n - 1}, {"alpha": 0.0},
               {"alpha": -1.0}, {"ell": np.array([0.5, 0.0])}, {"ell": np.array([-0.5]), "n_ell": 1}, {"sigma": -0.1}, {"H": None},
               {"X": None}, {"y": None}, {"ell": None}, {"out": None}, {"n_ell": 3}, {"D": 0}, {"D": 65, "n_ell": 1}):
        fill()
        assert host(**kw) == EARG, kw
        assert c._lib.gpmi_last_error()
        assert untouched(), kw
    # the device-resident form checks before it touches anything: the pointers are never dereferenced
    torch, dev = _torch()
    buf = torch.full((256,), SENTINEL, dtype=torch.float64, device=dev)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    P = buf.data_ptr()

    def devf(dX=P, n=n, ldx=n, D=D, dy=P, alpha=1.0, ell=ell, n_ell=D, sigma=0.1, dout=P, dH=P + 8 * 16, dinfo=info.data_ptr(), ldh=None):
        v = lambda p: C.c_void_p(p) if p else None
        return lib.gpmi_logml_hess_dev(h, v(dX), n, ldx, D, v(dy), d(alpha), None if ell is None else _p(ell), n_ell, d(sigma),
                                       d(0.0), v(dout), None, v(dH), 2 + n_ell if ldh is None else ldh, v(dinfo))

    for kw in ({"D": 9, "ell": ell9, "n_ell": 9}, {"ldh": 3}, {"n": 0}, {"ldx": n - 1}, {"alpha": 0.0}, {"ell": np.array([0.5, 0.0])},
               {"sigma": -0.1}, {"dH": 0}, {"dX": 0}, {"dy": 0}, {"ell": None}, {"dout": 0}, {"dinfo": 0}):
        assert devf(**kw) == EARG, kw
    c.sync()
    assert bool(torch.all(buf == SENTINEL)) and int(info.cpu()[0]) == -7
