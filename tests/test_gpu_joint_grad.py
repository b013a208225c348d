"""GPU: gpmi_joint_logml_grad[_dev, _grid] -- value and gradient of the joint [y; y'] log marginal likelihood through one
factorisation of the order-2n matrix -- against the long-double reference of tests/joint_grad_reference.py, against
gpmi_joint_logml (code already in the tree) and its central differences, and against itself across routes (augmented
factorisation / three chains), calls and entry points.

The bounds are those of tests/test_gpu_centered_gp.py.  Both sides factor the same matrix backward-stably: the float64
reference stays under 1 cond eps on every parity input and cond <= 2e7 (tests/test_joint_grad_reference.py); the device gets
10 cond eps, relative, for out3[1] and out3[2].  The gradient is a sum of (2n)^2 products that cancel, so per theta
|grad - ref| <= 10 cond eps max|grad| + 32 eps gabs_theta, gabs_theta the sum of the absolute terms (a tiled fixed-order sum of
700^2 terms errs by at most 19 eps sum|t|, rounded up to 32)."""
import ctypes as C

import numpy as np
import pytest

import joint_grad_reference as jr

pytestmark = pytest.mark.gpu

EPS = jr.EPS
A, S, J = jr.PARITY_ALPHA, jr.PARITY_SIGMA, jr.PARITY_JITTER


@pytest.fixture(scope="module")
def chain_ctx():
    """A second context whose gradient calls take the three-chain route (U = L^-T, a = U z, W = -U U^T) at every size."""
    import gp_amd
    c = gp_amd.Context(0)
    c.set_option("grad_aug_n", 0)
    c.set_option("grad_aug_ng", 0)   # ... and its grids too
    yield c
    c.close()


def _routes(ctx, chain_ctx):
    return ((ctx, "augmented"), (chain_ctx, "three chains"))


@pytest.mark.parametrize("case", jr.PARITY_CASES, ids=lambda c: "n%d-l%g" % c)
def test_parity_and_value_consistency(ctx, chain_ctx, case):
    (t, yy), ref, cond = jr.parity_reference(case)
    ce = cond * EPS
    gmax = float(np.max(np.abs(ref["grad"])))
    gb = 10.0 * ce * gmax + 32.0 * EPS * ref["gabs"]
    want = np.array(ctx.joint_logml(t, yy, A, case[1], S, J))
    for c, name in _routes(ctx, chain_ctx):
        out, g = c.joint_logml_grad(t, yy, A, case[1], S, J)
        e3 = np.abs((out.astype(np.longdouble) - ref["out3"]) / ref["out3"]).astype(float)
        eg = np.abs(g.astype(np.longdouble) - ref["grad"]).astype(float)
        ev = np.abs(out - want) / np.abs(want)
        print("n %d l %g %s: cond %.1e; in cond eps: sum_log %.3f quad %.3f, value vs joint_logml %s; grad error / its bound %s"
              % (case[0], case[1], name, cond, e3[1] / ce, e3[2] / ce, ev / ce, eg / gb))
        assert np.all(e3[1:] <= 10.0 * ce), (name, e3 / ce)
        assert np.all(eg <= gb), (name, eg / gb)
        assert np.all(ev <= 10.0 * ce), (name, ev / ce)


def test_central_differences_of_joint_logml(ctx, chain_ctx):
    n, l, h = 97, 0.3, 1e-5
    t, yy = jr.case_inputs(n)
    th = np.array([A, l, S])

    def f(p):
        return ctx.joint_logml(t, yy, p[0], p[1], p[2], J)[0]

    fd = np.array([(f(th + h * e) - f(th - h * e)) / (2 * h) for e in np.eye(3)])
    for c, name in _routes(ctx, chain_ctx):
        _, g = c.joint_logml_grad(t, yy, A, l, S, J)
        err = np.max(np.abs(g - fd)) / np.max(np.abs(g))
        print("central differences, %s: g %s fd %s; max|g - fd| / max|g| = %.2e" % (name, g, fd, err))
        assert err <= 5e-6, (name, g, fd)


def test_repeated_calls_give_identical_bits(ctx, chain_ctx):
    t, yy = jr.case_inputs(129)
    for c, name in _routes(ctx, chain_ctx):
        o1, g1 = c.joint_logml_grad(t, yy, A, 0.2, S, J)
        o2, g2 = c.joint_logml_grad(t, yy, A, 0.2, S, J)
        assert np.array_equal(o1, o2) and np.array_equal(g1, g2), name
        assert np.all(np.isfinite(g1))


def _value_dev(c, t, yy, alpha, l, sigma, jitter):
    """(out3, info) of gpmi_joint_logml_dev: the value call's answer where the host-buffer form would raise."""
    import torch
    dev = torch.device("cuda:0")
    dt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
    dyy = torch.from_numpy(np.ascontiguousarray(yy, dtype=np.float64)).to(dev)
    do = torch.zeros(3, dtype=torch.float64, device=dev); di = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    c.joint_logml_dev(dt.data_ptr(), t.size, dyy.data_ptr(), alpha, l, sigma, jitter, do.data_ptr(), di.data_ptr())
    c.sync()
    return do.cpu().numpy(), int(di.item())


@pytest.mark.parametrize("route", ("augmented", "three chains"))
def test_grid_on_lanes_equals_single_calls(ctx, chain_ctx, route):
    """G = 5 (not a multiple of the lane count) at n = 129 with one point that is not positive definite (an enormous l and
    alpha against a tiny sigma: the matrix is numerically of low rank and the jitter drowns in its rounding), on each route."""
    c = ctx if route == "augmented" else chain_ctx
    n = 129
    t, yy = jr.case_inputs(n)
    a = np.array([1.1, 1.0, 1.2, 1e8, 0.9]); l = np.array([0.2, 0.25, 0.3, 50.0, 0.2]); s = np.array([0.1, 0.12, 0.2, 1e-9, 0.15])
    out, g, info = c.joint_logml_grad_grid(t, yy, a, l, s, J)
    assert out.shape == (5, 3) and g.shape == (5, 3) and info.shape == (5,)
    assert info[3] > 0 and np.all(np.isnan(g[3])) and np.all(np.delete(info, 3) == 0)
    # out3 of the failed point is what gpmi_joint_logml returns for it (which pivot fails first is decided by rounding here)
    vo, vi = _value_dev(c, t, yy, a[3], l[3], s[3], J)
    np.testing.assert_array_equal(out[3], vo)
    assert vi > 0
    for k in (0, 1, 2, 4):
        o1, g1 = c.joint_logml_grad(t, yy, a[k], l[k], s[k], J)
        assert np.array_equal(out[k], o1) and np.array_equal(g[k], g1), k
        assert np.all(np.isfinite(g1))
    # an empty grid is no error
    o0, g0, i0 = c.joint_logml_grad_grid(t, yy, np.zeros(0), np.zeros(0), np.zeros(0), J)
    assert o0.shape == (0, 3) and i0.size == 0


def test_not_positive_definite_is_a_status(ctx):
    import gp_amd
    t = np.zeros(20); yy = np.ones(40)   # identical points, no noise, no jitter: the second pivot is exactly zero
    with pytest.raises(gp_amd.NotPositiveDefinite) as ei:
        ctx.joint_logml_grad(t, yy, 1.0, 0.5, 0.0, 0.0)
    assert ei.value.order == 2
    out, g = ctx.joint_logml_grad(np.linspace(-1, 1, 30), np.ones(60), 1.0, 0.3, 0.1, J)   # healthy afterwards
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(g))


def test_dev_form_on_torch_tensors(ctx):
    import torch
    dev = torch.device("cuda:0")
    n, l = 65, 0.3
    t, yy = jr.case_inputs(n)
    want_o, want_g = ctx.joint_logml_grad(t, yy, A, l, S, J)
    dt = torch.from_numpy(t).to(dev); dyy = torch.from_numpy(yy).to(dev)
    do = torch.full((3,), -5.0, dtype=torch.float64, device=dev); dg = torch.full((3,), -5.0, dtype=torch.float64, device=dev)
    di = torch.full((1,), -7, dtype=torch.int32, device=dev)
    # not positive definite (identical points, no noise, no jitter): the device writes the NaNs and the order itself
    bt = torch.zeros(20, dtype=torch.float64, device=dev); byy = torch.ones(40, dtype=torch.float64, device=dev)
    bo = torch.zeros(3, dtype=torch.float64, device=dev); bg = torch.zeros(3, dtype=torch.float64, device=dev)
    bi = torch.zeros(1, dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream(dev)
    ctx.set_stream(cur.cuda_stream)
    try:
        ctx.joint_logml_grad_dev(dt.data_ptr(), n, dyy.data_ptr(), A, l, S, J, do.data_ptr(), dg.data_ptr(), di.data_ptr())
        seen_o, seen_g = do.clone(), dg.clone()   # enqueued on torch's stream right behind the evaluation
        ctx.joint_logml_grad_dev(bt.data_ptr(), 20, byy.data_ptr(), 1.0, 0.5, 0.0, 0.0, bo.data_ptr(), bg.data_ptr(), bi.data_ptr())
        torch.cuda.synchronize(dev)
    finally:
        ctx.set_stream(None)
    assert int(di.item()) == 0
    assert np.array_equal(seen_o.cpu().numpy(), want_o) and np.array_equal(seen_g.cpu().numpy(), want_g)
    assert int(bi.item()) == 2 and bool(torch.isnan(bg).all().item())
    # out3 of the failed evaluation is what gpmi_joint_logml returns for it
    vo, vi = _value_dev(ctx, np.zeros(20), np.ones(40), 1.0, 0.5, 0.0, 0.0)
    np.testing.assert_array_equal(bo.cpu().numpy(), vo)
    assert vi == 2


def test_bad_arguments(ctx):
    from gp_amd import _lib
    lib, h = _lib.load(), ctx._h
    d = C.c_double
    n = 10
    t = np.linspace(-1, 1, n); yy = np.ones(2 * n); out = np.zeros(3); g = np.zeros(3)
    p = lambda a: C.c_void_p(a.ctypes.data)
    ok = (d(1.0), d(0.5), d(0.1), d(J))
    assert lib.gpmi_joint_logml_grad(h, p(t), n, p(yy), d(0.0), d(0.5), d(0.1), d(J), p(out), p(g)) == -1
    assert lib.gpmi_joint_logml_grad(h, p(t), n, p(yy), d(-1.0), d(0.5), d(0.1), d(J), p(out), p(g)) == -1
    assert lib.gpmi_joint_logml_grad(h, p(t), n, p(yy), d(1.0), d(0.0), d(0.1), d(J), p(out), p(g)) == -1
    assert lib.gpmi_joint_logml_grad(h, p(t), n, p(yy), d(1.0), d(float("inf")), d(0.1), d(J), p(out), p(g)) == -1
    assert lib.gpmi_joint_logml_grad(h, p(t), 0, p(yy), *ok, p(out), p(g)) == -1
    assert lib.gpmi_joint_logml_grad(h, None, n, p(yy), *ok, p(out), p(g)) == -1
    assert lib.gpmi_joint_logml_grad(h, p(t), n, p(yy), *ok, p(out), None) == -1
    # the _dev form validates before it enqueues anything (the pointers are never dereferenced on these paths)
    assert lib.gpmi_joint_logml_grad_dev(h, None, n, None, *ok, None, None, None) == -1
    assert lib.gpmi_joint_logml_grad_dev(h, p(t), n, p(yy), d(1.0), d(-0.5), d(0.1), d(J), p(out), p(g), p(out)) == -1
    info = np.zeros(2, dtype=np.int32); a2 = np.array([1.0, 0.0]); l2 = np.array([0.5, 0.5]); s2 = np.array([0.1, 0.1])
    o2 = np.zeros(6); g2 = np.zeros(6)
    assert lib.gpmi_joint_logml_grad_grid(h, p(t), n, p(yy), p(a2), p(l2), p(s2), 2, d(J), p(o2), p(g2), p(info)) == -1
    assert lib.gpmi_joint_logml_grad_grid(h, p(t), n, p(yy), p(l2), p(l2), p(s2), -1, d(J), p(o2), p(g2), p(info)) == -1
    assert lib.gpmi_joint_logml_grad_grid(h, p(t), n, p(yy), p(l2), p(l2), p(s2), 2, d(J), p(o2), None, p(info)) == -1
    assert lib.gpmi_joint_logml_grad_grid(h, p(t), n, p(yy), p(l2), p(l2), p(s2), 0, d(J), p(o2), p(g2), p(info)) == 0
    out, g = ctx.joint_logml_grad(t, yy, 1.0, 0.5, 0.1, J)   # the context works afterwards
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(g))
