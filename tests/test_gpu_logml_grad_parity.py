"""GPU: gpmi_logml_grad and gpmi_logml_grad_grid against the long-double reference of tests/logml_grad_reference.py on every
route -- one workgroup (k_logml_grad_small[_batch]), the augmented factorisation and the three chains, with k_grad_partial
(D <= 8) and k_grad_partial_big (D = 9 .. 64) as the contraction -- with ARD length-scales checked component by component,
sigma = 0 and a non-zero jitter; against gpmi_logml; and against itself across routes, calls and the grid.
tests/test_gpu_grad.py compares with a float64 oracle at rtol 1e-8 and checks ARD by central differences only.

The bounds are those of tests/test_gpu_joint_grad.py (cond <= 2e7 and the float64 reference within half of each on every parity
input: tests/test_logml_grad_reference.py):
  z'z: 10 cond eps, relative;   each theta: |grad - ref| <= 10 cond eps max|grad| + 32 eps gabs_theta;
  sum log L_ii: 10 cond eps |ref| + SUM_LOG_FLOOR_C n eps (the floor and how c = 4 was measured: tests/logml_grad_reference.py);
  the value -z'z / 2 - sum_log - n / 2 log(2 pi): the bounds of its two parts added.
Two device results are compared with twice the bound (each is within one of the reference).

Bit-identical pairs.  A grid point and a single call agree bit for bit where both run the same kernel with the same switches:
  the pinned batch (G <= 8) and the uploaded batches of k_logml_grad_small_batch   against  the single call on `one_wg`
      (small_ng1 = 256: k_logml_grad_small, the same device function for one point);
  the lanes of `aug` (n = 129 <= grad_aug_ng = 2304: augmented)                    against  the single call on `aug` (129 <= grad_aug_n = 3072);
  the lanes of `chains` (grad_aug_ng = 0: three chains)                            against  the single call on `chains` (grad_aug_n = 0).
A single call and a lane differ only in which of the two limits they read.  Across routes the results agree to rounding only.
"""
import numpy as np
import pytest

import logml_grad_reference as lg

pytestmark = pytest.mark.gpu

ROUTES = {"one_wg": {"small_ng1": 256},
          "aug": {"small_ng1": 0},
          "chains": {"small_ng1": 0, "grad_aug_n": 0, "grad_aug_ng": 0}}
PARITY = ([("one_wg", c) for c in lg.ONE_WG_CASES] + [("aug", c) for c in lg.CHAIN_CASES] + [("chains", c) for c in lg.CHAIN_CASES])
# the point test_gpu_grad.py::test_grad_grid_on_lanes_equals_single_calls rejects, in the middle of four healthy ones
BAD = 2
GRID_A = np.array([1.0, 1.1, 1.0, 0.9, 1.2])
GRID_R = np.array([0.8, 0.9, 50.0, 0.7, 0.85])
GRID_S = np.array([0.1, 0.12, 1e-9, 0.2, 0.15])


def _context(options):
    import gp_amd
    c = gp_amd.Context(0)
    for name, value in options.items():
        c.set_option(name, value)
    return c


@pytest.fixture(scope="module")
def one_wg():
    """Value + gradient by ONE workgroup up to n = 256 (the default stops at 128)."""
    c = _context(ROUTES["one_wg"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def aug():
    """No one-workgroup form for a single call: the augmented (2n + 1)-row factorisation at every size here."""
    c = _context(ROUTES["aug"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def chains():
    """... and the three-chain route (U = L^-T, a = U z, W = -U U^T) at every size, grids included."""
    c = _context(ROUTES["chains"])
    yield c
    c.close()


@pytest.fixture
def routes(one_wg, aug, chains):
    return {"one_wg": one_wg, "aug": aug, "chains": chains}


def _check(tag, out, g, ref, cond, n, scale=1.0):
    """Print error / bound of (sum_log, z'z, value, worst theta) and assert each <= 1."""
    es, eq, eg = lg.errors(out, g, ref)
    bs, bq, bg = lg.bounds(ref, cond, n, scale)
    ev, bv = abs(float(np.longdouble(out[0]) - ref["out3"][0])), lg.value_bound(ref, cond, n, scale)
    rg = np.where(bg > 0, eg / np.where(bg > 0, bg, 1.0), np.where(eg == 0, 0.0, np.inf))
    k = int(np.argmax(rg))
    print("%s: cond %.1e; error / bound: sum_log %.3f, z'z %.3f, value %.3f, grad %.3f (theta %d of %d)"
          % (tag, cond, es / bs, eq / bq, ev / bv, rg[k], k, rg.size))
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(g)), tag
    assert es <= bs, (tag, es / bs)
    assert eq <= bq, (tag, eq / bq)
    assert ev <= bv, (tag, ev / bv)
    assert np.all(rg <= 1.0), (tag, rg)


def _as_ref(out, g):
    """A device result in the shape of a reference (for route-against-route comparisons: gabs comes from the real one)."""
    return {"out3": np.asarray(out, np.longdouble), "grad": np.asarray(g, np.longdouble)}


@pytest.mark.parametrize("route,case", PARITY, ids=["%s-%s" % (r, lg.case_id(c)) for r, c in PARITY])
def test_parity_with_long_double(routes, route, case):
    c = routes[route]
    (X, y, a, ell, s, jit), ref, cond = lg.parity_reference(case)
    n = case[0]
    out, g = c.logml_grad(X, y, a, ell, s, jit)
    assert g.shape == (2 + ell.size,)
    _check("%s %s" % (route, lg.case_id(case)), out, g, ref, cond, n)
    if s == 0.0:
        assert g[-1] == 0.0     # 2 sigma tr(G): exactly zero, not a rounding residue (and finite: checked above)
    plain = c.logml(X, y, a, ell, s, jit)
    if route == "one_wg" and n <= 128:
        assert out[0] == plain[0]   # the same one-workgroup factorisation as the plain entry point (small_n1 = 128)
    else:                           # another factorisation of the same matrix
        assert abs(out[0] - plain[0]) <= lg.value_bound(ref, cond, n, 2.0), (out[0], plain[0])


@pytest.mark.parametrize("case", [c for c in lg.ONE_WG_CASES if c[0] in (128, 256) and not c[4]], ids=lg.case_id)
def test_three_routes_agree(routes, case):
    (X, y, a, ell, s, jit), ref, cond = lg.parity_reference(case)
    res = {name: c.logml_grad(X, y, a, ell, s, jit) for name, c in routes.items()}
    for p, q in (("one_wg", "aug"), ("one_wg", "chains"), ("aug", "chains")):
        other = dict(ref, **_as_ref(*res[q]))
        _check("%s: %s against %s" % (lg.case_id(case), p, q), res[p][0], res[p][1], other, cond, case[0], 2.0)


def test_two_chain_routes_agree_at_n385_D17(routes):
    case = (385, 17, True, 1e-3, "")
    assert case in lg.CHAIN_CASES
    (X, y, a, ell, s, jit), ref, cond = lg.parity_reference(case)
    o1, g1 = routes["aug"].logml_grad(X, y, a, ell, s, jit)
    o2, g2 = routes["chains"].logml_grad(X, y, a, ell, s, jit)
    _check("n385-D17: aug against chains", o1, g1, dict(ref, **_as_ref(o2, g2)), cond, 385, 2.0)


def _grid_checks(c, case, a, r, s, single, points):
    """One grid call with jitter 0 on the inputs of `case` (coincident points: without noise the matrix is singular): the point
    BAD fails alone and the others are healthy; the points `points` are within the parity bound of the long-double reference
    and equal the single call on `single` bit for bit (the pairs of the module docstring)."""
    X, y = lg.case_inputs(*case)[:2]
    n = case[0]
    bad = int(np.flatnonzero(s == 1e-9)[0])
    out, g, info = c.logml_grad_grid(X, y, a, r, s, 0.0)
    G = a.size
    assert out.shape == (G, 3) and g.shape == (G, 3) and info.shape == (G,)
    assert info[bad] > 0 and np.all(np.isnan(g[bad])), (info[bad], g[bad])
    assert np.all(np.delete(info, bad) == 0) and np.all(np.isfinite(np.delete(g, bad, axis=0)))
    for k in points:
        ref, cond = lg.point_reference(case, float(a[k]), float(r[k]), float(s[k]), 0.0)
        assert cond <= lg.COND_MAX
        _check("grid %s point %d" % (lg.case_id(case), k), out[k], g[k], ref, cond, n)
        o1, g1 = single.logml_grad(X, y, a[k], [r[k]], s[k], 0.0)
        assert np.array_equal(out[k], o1) and np.array_equal(g[k], g1), k
    return X, y


def test_grid_pinned_batch(one_wg):
    """G = 5 <= 8, n = 65, D = 3: ONE launch of k_logml_grad_small_batch through the pinned buffer; and a second grid of the
    four healthy points with jitter 1e-6 (the chain rule through diag_add = sigma^2 + jitter on this path)."""
    case = (65, 3, False, 0.15, "dup")
    X, y = _grid_checks(one_wg, case, GRID_A, GRID_R, GRID_S, one_wg, (0, 1, 3, 4))
    keep = np.delete(np.arange(5), BAD)
    out, g, info = one_wg.logml_grad_grid(X, y, GRID_A[keep], GRID_R[keep], GRID_S[keep], lg.PARITY_JITTER)
    assert np.all(info == 0)
    for i, k in enumerate(keep):
        ref, cond = lg.point_reference(case, float(GRID_A[k]), float(GRID_R[k]), float(GRID_S[k]), lg.PARITY_JITTER)
        _check("grid with jitter, point %d" % k, out[i], g[i], ref, cond, 65)
        o1, g1 = one_wg.logml_grad(X, y, GRID_A[k], [GRID_R[k]], GRID_S[k], lg.PARITY_JITTER)
        assert np.array_equal(out[i], o1) and np.array_equal(g[i], g1), k


def test_grid_uploaded_batches(one_wg):
    """G = 130 > 128 points of one launch, n = 21, D = 8: two launches of k_logml_grad_small_batch from device memory."""
    G = 130
    rng = np.random.default_rng(130)
    a = 0.8 + 0.4 * rng.random(G); r = 0.6 + 0.4 * rng.random(G); s = 0.05 + 0.2 * rng.random(G)
    a[G // 2], r[G // 2], s[G // 2] = GRID_A[BAD], GRID_R[BAD], GRID_S[BAD]
    _grid_checks(one_wg, (21, 8, False, 0.15, "dup"), a, r, s, one_wg, (0, 127, 128, 129))


@pytest.mark.parametrize("route,D", [("aug", 9), ("chains", 17)])
def test_grid_on_lanes(routes, route, D):
    """G = 5 (not a multiple of the lane count), n = 129, D > 8: no one-workgroup form, the points go round the lanes."""
    c = routes[route]
    _grid_checks(c, (129, D, False, 0.15, "dup"), GRID_A, GRID_R, GRID_S, c, (0, 1, 3, 4))


@pytest.mark.parametrize("route,case", [("one_wg", (129, 8, True, 1e-3, "")), ("aug", (129, 33, True, 0.0, "")),
                                        ("chains", (129, 33, True, 0.0, ""))], ids=["one_wg-D8", "aug-D33", "chains-D33"])
def test_repeated_calls_give_identical_bits(routes, route, case):
    """Each route once at the largest D it is tested at with n past a tile and a panel (every sum has a fixed order)."""
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    o1, g1 = routes[route].logml_grad(X, y, a, ell, s, jit)
    o2, g2 = routes[route].logml_grad(X, y, a, ell, s, jit)
    assert np.array_equal(o1, o2) and np.array_equal(g1, g2)
    assert np.all(np.isfinite(o1)) and np.all(np.isfinite(g1))
