"""GPU: the forms of the log-ml gradient that the device finishes itself -- gpmi_logml_grad_dev, gpmi_logml_grad_grid_dev and the
ARD grids gpmi_logml_grad_grid_ard[_dev] -- on the three routes of tests/test_gpu_logml_grad_parity.py (its contexts, its
_check, the bounds of tests/logml_grad_reference.py at scale 1 against long double; no tolerance of this file's own).

What is bit-identical and why: k_logml_grad_finish states logml_grad_unpack (gpmi_grad_from_sums, then 2 sigma tr G; contraction
off on both sides), so a device-resident form equals the host form on the same route; an ARD grid point runs
logml_grad_small_body (one_wg) or logml_grad_core (lanes) with the parameters the single call forms (1 / ell on the host), so it
equals gpmi_logml_grad at that point on the same context; D = 1 makes the ARD grid the isotropic one.

Device buffers are torch tensors, filled with a sentinel (-5.0, -7) before every device-resident call.  X is column-major:
a (D, ldx) tensor whose row d holds column d."""
import ctypes as C

import numpy as np
import pytest

import logml_grad_ard_grids as ag
import logml_grad_reference as lg
from test_gpu_logml_grad_parity import _check, aug, chains, one_wg, routes  # noqa: F401  (fixtures: the three contexts)

pytestmark = pytest.mark.gpu

EARG = -1
PAD = 1e3   # rows n .. ldx of X when ldx > n: never read into a result


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def _up(X, y, ldx=None):
    """(dX (D, ldx), dy, ldx) on the device."""
    torch, dev = _torch()
    n, D = X.shape
    ldx = n if ldx is None else ldx
    Xt = np.full((D, ldx), PAD)
    Xt[:, :n] = X.T
    return torch.from_numpy(Xt).to(dev), torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev), ldx


def _outs(G, ncomp):
    """Sentinel-filled d_out3 (G, 3), d_grad (G, ncomp), d_info (G,)."""
    torch, dev = _torch()
    return (torch.full((G, 3), -5.0, dtype=torch.float64, device=dev), torch.full((G, ncomp), -5.0, dtype=torch.float64, device=dev),
            torch.full((G,), -7, dtype=torch.int32, device=dev))


def _down(c, do, dg, di):
    c.sync()
    return do.cpu().numpy(), dg.cpu().numpy(), di.cpu().numpy()


def _grad_dev(c, X, y, a, ell, s, jit, ldx=None):
    """gpmi_logml_grad_dev -> (out3 (3,), grad (2 + n_ell,), info)."""
    dX, dy, ldx = _up(X, y, ldx)
    ell = np.atleast_1d(np.asarray(ell, float))
    do, dg, di = _outs(1, 2 + ell.size)
    _torch()[0].cuda.synchronize()
    c.logml_grad_dev(dX.data_ptr(), X.shape[0], ldx, X.shape[1], dy.data_ptr(), a, ell, s, jit, do.data_ptr(), dg.data_ptr(), di.data_ptr())
    out, g, info = _down(c, do, dg, di)
    return out[0], g[0], int(info[0])


def _ard_dev(c, X, y, a, E, s, jit, ldx=None):
    dX, dy, ldx = _up(X, y, ldx)
    G, D = E.shape
    do, dg, di = _outs(G, D + 2)
    _torch()[0].cuda.synchronize()
    c.logml_grad_grid_ard_dev(dX.data_ptr(), X.shape[0], ldx, D, dy.data_ptr(), a, E, s, jit, do.data_ptr(), dg.data_ptr(), di.data_ptr())
    return _down(c, do, dg, di)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


SINGLE = ([("one_wg", c) for c in ag.ONE_WG_SINGLE] + [("aug", c) for c in ag.CHAIN_SINGLE] + [("chains", c) for c in ag.CHAIN_SINGLE])


# ---- 1. the device-resident single call ------------------------------------------------------------------------------
@pytest.mark.parametrize("route,case", SINGLE, ids=["%s-%s" % (r, lg.case_id(c)) for r, c in SINGLE])
def test_dev_equals_host_form_bit_for_bit(routes, route, case):
    c = routes[route]
    (X, y, a, ell, s, jit), ref, cond = lg.parity_reference(case)
    out, g = c.logml_grad(X, y, a, ell, s, jit)
    _check("%s %s (host form)" % (route, lg.case_id(case)), out, g, ref, cond, case[0])
    o1, g1, info = _grad_dev(c, X, y, a, ell, s, jit)
    assert info == 0
    assert np.array_equal(o1, out) and np.array_equal(g1, g), (o1, out, g1, g)
    if s == 0.0:
        assert g1[-1] == 0.0


@pytest.mark.parametrize("route,case", [("one_wg", ag.ONE_WG_SINGLE[1]), ("aug", ag.CHAIN_SINGLE[0]), ("chains", ag.CHAIN_SINGLE[1])],
                         ids=["one_wg", "aug", "chains"])
def test_dev_with_a_leading_dimension_past_n(routes, route, case):
    """X a view of a taller matrix (ldx = n + 3, the rows below hold PAD): the bits of the packed call."""
    c = routes[route]
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    o0, g0, i0 = _grad_dev(c, X, y, a, ell, s, jit)
    o1, g1, i1 = _grad_dev(c, X, y, a, ell, s, jit, ldx=case[0] + 3)
    assert i0 == 0 and i1 == 0 and np.all(np.isfinite(g0))
    assert np.array_equal(o0, o1) and np.array_equal(g0, g1)


# ---- 2. / 3. not positive definite: a status, on the context's and on the caller's stream -----------------------------
def _singular(n, D):
    """n coincident points without noise: S = alpha^2 in every entry, the pivot of order 2 is exactly zero."""
    return np.zeros((n, D)), np.ones(n), 1.0, np.full(D, 0.5), 0.0, 0.0


NOT_PD = [("one_wg", 20, 3, ag.ONE_WG_SINGLE[1]), ("aug", 129, 9, ag.CHAIN_SINGLE[0]), ("chains", 129, 9, ag.CHAIN_SINGLE[0])]


@pytest.mark.parametrize("route,n,D,healthy", NOT_PD, ids=[r[0] for r in NOT_PD])
def test_not_positive_definite_is_a_status_and_the_context_goes_on(routes, route, n, D, healthy):
    c = routes[route]
    X, y, a, ell, s, jit = _singular(n, D)
    o1, g1, info = _grad_dev(c, X, y, a, ell, s, jit)          # returns 0: nothing is raised
    assert info == 2 and np.all(np.isnan(g1)) and g1.shape == (D + 2,), (info, g1)
    dX, dy, ldx = _up(X, y)
    do, _, di = _outs(1, 1)
    c.logml_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), a, ell, s, jit, do.data_ptr(), di.data_ptr())
    c.sync()
    assert int(di.cpu()[0]) == info and _same(do.cpu().numpy()[0], o1), (do.cpu().numpy(), o1)
    # a healthy call right after, on the same context: the bits of the host form
    X, y, a, ell, s, jit = lg.case_inputs(*healthy)
    o2, g2, i2 = _grad_dev(c, X, y, a, ell, s, jit)
    out, g = c.logml_grad(X, y, a, ell, s, jit)
    assert i2 == 0 and np.array_equal(o2, out) and np.array_equal(g2, g)


@pytest.mark.parametrize("route,n,D,healthy", NOT_PD, ids=[r[0] for r in NOT_PD])
def test_two_calls_on_the_callers_stream(routes, route, n, D, healthy):
    """The pattern of tests/test_gpu_joint_grad.py: a healthy call and one that is not positive definite, back to back on torch's
    stream, are correct after torch.cuda.synchronize() alone."""
    torch, dev = _torch()
    c = routes[route]
    X, y, a, ell, s, jit = lg.case_inputs(*healthy)
    out, g = c.logml_grad(X, y, a, ell, s, jit)
    dX, dy, ldx = _up(X, y)
    do, dg, di = _outs(1, g.size)
    Xb, yb, ab, eb, sb, jb = _singular(n, D)
    bX, by, bld = _up(Xb, yb)
    bo, bg, bi = _outs(1, D + 2)
    torch.cuda.synchronize(dev)
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        c.logml_grad_dev(dX.data_ptr(), X.shape[0], ldx, X.shape[1], dy.data_ptr(), a, ell, s, jit, do.data_ptr(), dg.data_ptr(), di.data_ptr())
        seen_o, seen_g = do.clone(), dg.clone()     # enqueued on torch's stream right behind the evaluation
        c.logml_grad_dev(bX.data_ptr(), n, bld, D, by.data_ptr(), ab, eb, sb, jb, bo.data_ptr(), bg.data_ptr(), bi.data_ptr())
        torch.cuda.synchronize(dev)
    finally:
        c.set_stream(None)
    assert int(di.item()) == 0 and np.array_equal(seen_o.cpu().numpy()[0], out) and np.array_equal(seen_g.cpu().numpy()[0], g)
    assert int(bi.item()) == 2 and bool(torch.isnan(bg).all().item())


# ---- 4. / 5. ARD grids ----------------------------------------------------------------------------------------------------
def _ard_grid_checks(c, name, jitter, keep=None):
    """One host-form ARD grid on the context: info and NaN at the rejected point alone; the checked points within the parity
    bound of the long-double ARD reference and equal to the single call on the same context bit for bit."""
    case, G, bad, _, pts = ag.GRIDS[name]
    X, y = ag.grid_data(name)
    a, E, s = ag.grid_points(name)
    idx = np.arange(G) if keep is None else np.asarray(keep)
    out, g, info = c.logml_grad_grid_ard(X, y, a[idx], E[idx], s[idx], jitter)
    assert out.shape == (idx.size, 3) and g.shape == (idx.size, case[1] + 2) and info.shape == (idx.size,)
    for i, k in enumerate(idx):
        if k == bad:
            assert info[i] > 0 and np.all(np.isnan(g[i])), (info[i], g[i])
        else:
            assert info[i] == 0 and np.all(np.isfinite(g[i])) and np.all(np.isfinite(out[i])), (k, info[i])
        if k in pts:
            ref, cond = ag.point_reference(name, int(k), jitter)
            assert cond <= lg.COND_MAX
            _check("ARD grid %s point %d jitter %g" % (name, k, jitter), out[i], g[i], ref, cond, case[0])
            o1, g1 = c.logml_grad(X, y, a[k], E[k], s[k], jitter)
            assert np.array_equal(out[i], o1) and np.array_equal(g[i], g1), k
    return out, g, info


def test_ard_grid_one_workgroup_per_point(one_wg):
    """n = 65, D = 3, G = 5 with the rejected point in the middle (jitter 0), then the four healthy points with jitter 1e-6
    (the chain rule through diag_add = sigma^2 + jitter)."""
    _ard_grid_checks(one_wg, "n65-D3-dup", 0.0)
    _ard_grid_checks(one_wg, "n65-D3-dup", 1e-6, keep=(0, 1, 3, 4))


def test_ard_grid_of_one_point_more_than_a_launch(one_wg):
    """n = 21, D = 8, G = 129: two launches of k_logml_grad_batch_dev over the same workspace, the rejected point in the first."""
    assert ag.GRIDS["n21-D8-dup"][1] == ag.PTS_PER_LAUNCH + 1
    _ard_grid_checks(one_wg, "n21-D8-dup", 0.0)


def test_ard_grid_at_the_largest_one_workgroup_size(one_wg):
    _ard_grid_checks(one_wg, "n256-D8-ard", 1e-6)


@pytest.mark.parametrize("route,name", [("aug", "n129-D9-dup"), ("chains", "n129-D17-dup"), ("aug", "n257-D2-ard")])
def test_ard_grid_on_the_lanes(routes, route, name):
    """G = 5 (not a multiple of the lane count) at D > 8, and n = 257 (one row past the one-workgroup form) at D = 2."""
    _ard_grid_checks(routes[route], name, ag.GRIDS[name][3][0])


# ---- 6. host grids against device-resident grids ---------------------------------------------------------------------------
@pytest.mark.parametrize("route,name", [("one_wg", "n65-D3-dup"), ("one_wg", "n21-D8-dup"), ("aug", "n129-D9-dup"),
                                        ("chains", "n129-D17-dup")])
def test_ard_host_grid_equals_dev_grid(routes, route, name):
    c = routes[route]
    X, y = ag.grid_data(name)
    a, E, s = (v[:5] for v in ag.grid_points(name))
    if name == "n21-D8-dup":
        E = E.copy(); E[2], s = ag.BAD_ELL, np.where(np.arange(5) == 2, ag.BAD_SIGMA, s)   # the rejected point among the five
    out, g, info = c.logml_grad_grid_ard(X, y, a, E, s, 0.0)
    o1, g1, i1 = _ard_dev(c, X, y, a, E, s, 0.0)
    assert info[2] > 0 and np.all(np.delete(info, 2) == 0)
    assert np.array_equal(info, i1) and _same(out, o1) and _same(g, g1)
    assert np.all(np.isnan(g1[2])) and np.all(np.isfinite(np.delete(g1, 2, axis=0)))
    o2, g2, i2 = _ard_dev(c, X, y, a, E, s, 0.0, ldx=X.shape[0] + 3)
    assert np.array_equal(i1, i2) and _same(o1, o2) and _same(g1, g2)


GRID_A = np.array([1.0, 1.1, 1.0, 0.9, 1.2])
GRID_R = np.array([0.8, 0.9, 50.0, 0.7, 0.85])
GRID_S = np.array([0.1, 0.12, 1e-9, 0.2, 0.15])


@pytest.mark.parametrize("route,case", [("one_wg", (65, 3, False, 0.15, "dup")), ("aug", (129, 9, False, 0.15, "dup"))],
                         ids=["one_wg-n65-D3", "aug-n129-D9"])
def test_isotropic_host_grid_equals_dev_grid(routes, route, case):
    c = routes[route]
    X, y = lg.case_inputs(*case)[:2]
    out, g, info = c.logml_grad_grid(X, y, GRID_A, GRID_R, GRID_S, 0.0)
    dX, dy, ldx = _up(X, y)
    do, dg, di = _outs(5, 3)
    c.logml_grad_grid_dev(dX.data_ptr(), case[0], ldx, case[1], dy.data_ptr(), GRID_A, GRID_R, GRID_S, 0.0, do.data_ptr(), dg.data_ptr(),
                          di.data_ptr())
    o1, g1, i1 = _down(c, do, dg, di)
    assert info[2] > 0 and np.all(np.delete(info, 2) == 0) and np.all(np.isfinite(np.delete(g, 2, axis=0)))
    assert np.array_equal(info, i1) and _same(out, o1) and _same(g, g1)


# ---- 7. against the existing entry points ---------------------------------------------------------------------------------
def test_ard_grid_at_D1_is_the_isotropic_grid(one_wg):
    X, y = lg.case_inputs(65, 1, False, 0.15)[:2]
    out, g, info = one_wg.logml_grad_grid(X, y, GRID_A, GRID_R, GRID_S, 0.0)
    o1, g1, i1 = one_wg.logml_grad_grid_ard(X, y, GRID_A, GRID_R.reshape(5, 1), GRID_S, 0.0)
    assert np.all(np.isfinite(np.delete(g, 2, axis=0)))
    assert np.array_equal(info, i1) and _same(out, o1) and _same(g, g1)


def test_ard_grid_with_equal_length_scales_against_the_isotropic_grid(one_wg):
    """E[g, :] = rho[g] at D = 3: the same matrix, so value, d/dalpha and d/dsigma have the same bits; d/drho is the sum of the D
    components, formed in another order: twice the bound of that component (two device results)."""
    case = (65, 3, False, 0.15, "dup")
    X, y = lg.case_inputs(*case)[:2]
    keep = np.array([0, 1, 3, 4])
    a, r, s = GRID_A[keep], GRID_R[keep], GRID_S[keep]
    out, g, info = one_wg.logml_grad_grid(X, y, a, r, s, lg.PARITY_JITTER)
    o1, g1, i1 = one_wg.logml_grad_grid_ard(X, y, a, np.repeat(r[:, None], 3, axis=1), s, lg.PARITY_JITTER)
    assert np.all(info == 0) and np.all(i1 == 0)
    assert np.array_equal(out, o1) and np.array_equal(g[:, 0], g1[:, 0]) and np.array_equal(g[:, 2], g1[:, 4])
    for i in range(4):
        ref, cond = lg.point_reference(case, float(a[i]), float(r[i]), float(s[i]), lg.PARITY_JITTER)
        bound = lg.bounds(ref, cond, 65, 2.0)[2][1]
        err = abs(float(g1[i, 1:4].sum()) - float(g[i, 1]))
        print("point %d: |sum_d d/dell_d - d/drho| / bound = %.3f" % (i, err / bound))
        assert err <= bound, (i, err, bound)


# ---- 8. identical bits on every call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,case", [("one_wg", (129, 8, True, 1e-3, "")), ("aug", (129, 33, True, 0.0, "")),
                                        ("chains", (129, 33, True, 0.0, ""))], ids=["one_wg-D8", "aug-D33", "chains-D33"])
def test_repeated_calls_give_identical_bits(routes, route, case):
    c = routes[route]
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    r1, r2 = _grad_dev(c, X, y, a, ell, s, jit), _grad_dev(c, X, y, a, ell, s, jit)
    assert r1[2] == 0 and np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and np.all(np.isfinite(r1[1]))
    rng = np.random.default_rng(8)
    A, E, S = 0.8 + 0.4 * rng.random(3), ell * (0.9 + 0.2 * rng.random((3, case[1]))), 0.05 + 0.2 * rng.random(3)
    q1, q2 = c.logml_grad_grid_ard(X, y, A, E, S, jit), c.logml_grad_grid_ard(X, y, A, E, S, jit)
    assert np.all(q1[2] == 0) and np.all(np.isfinite(q1[1]))
    assert all(np.array_equal(u, v) for u, v in zip(q1, q2))


# ---- 9. arguments ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_an_empty_grid_writes_nothing(one_wg):
    import gp_amd
    c = one_wg
    X, y = ag.grid_data("n65-D3-dup")
    a, E, s = (v[:3].copy() for v in ag.grid_points("n65-D3-dup"))
    E[2] = 0.8; s[2] = 0.1
    n, D = X.shape
    dX, dy, ldx = _up(X, y)
    do, dg, di = _outs(3, D + 2)
    ptrs = (do.data_ptr(), dg.data_ptr(), di.data_ptr())

    def refused(call):
        with pytest.raises(gp_amd.GpmiError) as e:
            call()
        assert e.value.code == EARG, e.value

    Eb = E.copy(); Eb[1, 2] = 0.0
    refused(lambda: c.logml_grad_grid_ard(X, y, a, Eb, s, 0.0))
    refused(lambda: c.logml_grad_grid_ard_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), a, Eb, s, 0.0, *ptrs))
    refused(lambda: c.logml_grad_grid_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), a, np.array([0.8, -1.0, 0.8]), s, 0.0, *ptrs))
    refused(lambda: c.logml_grad_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), 1.0, Eb[1], 0.1, 0.0, *ptrs))
    # ldx < n, a NULL output
    refused(lambda: c.logml_grad_grid_ard_dev(dX.data_ptr(), n, n - 1, D, dy.data_ptr(), a, E, s, 0.0, *ptrs))
    refused(lambda: c.logml_grad_grid_dev(dX.data_ptr(), n, n - 1, D, dy.data_ptr(), a, E[:, 0], s, 0.0, *ptrs))
    refused(lambda: c.logml_grad_dev(dX.data_ptr(), n, n - 1, D, dy.data_ptr(), 1.0, E[0], 0.1, 0.0, *ptrs))
    refused(lambda: c.logml_grad_grid_ard_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), a, E, s, 0.0, ptrs[0], 0, ptrs[2]))
    refused(lambda: c.logml_grad_grid_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), a, E[:, 0], s, 0.0, 0, ptrs[1], ptrs[2]))
    refused(lambda: c.logml_grad_dev(dX.data_ptr(), n, ldx, D, dy.data_ptr(), 1.0, E[0], 0.1, 0.0, ptrs[0], ptrs[1], 0))
    # G < 0 (the C ABI itself: the binding takes G from the arrays), all three grids
    lib, h = c._lib, c._h
    vp, dbl = C.c_void_p, C.c_double
    host = [np.ascontiguousarray(v) for v in (a, E, s)]
    hp = [vp(v.ctypes.data) for v in host]
    dev_args = (h, vp(dX.data_ptr()), n, ldx, D, vp(dy.data_ptr()), hp[0], hp[1], hp[2])
    assert lib.gpmi_logml_grad_grid_ard_dev(*dev_args, -1, dbl(0.0), *map(vp, ptrs)) == EARG
    assert lib.gpmi_logml_grad_grid_dev(*dev_args, -1, dbl(0.0), *map(vp, ptrs)) == EARG
    Xf = np.asfortranarray(X)
    ho, hg, hi = np.full((3, 3), -5.0), np.full((3, D + 2), -5.0), np.full(3, -7, dtype=np.int32)
    host_args = (h, vp(Xf.ctypes.data), n, n, D, vp(y.ctypes.data), hp[0], hp[1], hp[2])
    assert lib.gpmi_logml_grad_grid_ard(*host_args, -1, dbl(0.0), vp(ho.ctypes.data), vp(hg.ctypes.data), vp(hi.ctypes.data)) == EARG
    # G = 0: success, and nothing is written
    assert lib.gpmi_logml_grad_grid_ard_dev(*dev_args, 0, dbl(0.0), *map(vp, ptrs)) == 0
    assert lib.gpmi_logml_grad_grid_dev(*dev_args, 0, dbl(0.0), *map(vp, ptrs)) == 0
    assert lib.gpmi_logml_grad_grid_ard(*host_args, 0, dbl(0.0), vp(ho.ctypes.data), vp(hg.ctypes.data), vp(hi.ctypes.data)) == 0
    o, g, i = _down(c, do, dg, di)
    assert np.all(o == -5.0) and np.all(g == -5.0) and np.all(i == -7)        # ... nor by any refused call above
    assert np.all(ho == -5.0) and np.all(hg == -5.0) and np.all(hi == -7)
    # and the context still works
    out, g, info = c.logml_grad_grid_ard(X, y, a, E, s, 0.0)
    assert np.all(info == 0) and np.all(np.isfinite(g))
