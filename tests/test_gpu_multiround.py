"""GPU: the multi-round paths of the trailing update -- band walk, per-XCD quadrant tail, row-major tail split, thin last row,
fused diagonal block of a multi-round launch, trapezoids -- checked ELEMENT BY ELEMENT at orders 768 .. 1345.

On the device's own CU count these paths start at n > 4100, where the suite compares one scalar per factorisation.  The
"debug_ncu" option makes the planner of the trailing update see 8 or 12 compute units (16 or 24 workgroup slots), which changes
no kernel: the same code then runs on launches of 21 .. 55 tiles.  tests/multiround_shapes.py holds the shapes and routes,
tests/test_syrk_walk_host.py shows on the CPU which path class each of their updates takes.

Bounds, none of them measured on the device (eps = 2^-52, u = eps / 2):
  factor, backward   |fl(L L^T) - A| <= (2 (n + 2) eps + g_n) |L| |L|^T / (1 - g_n) componentwise, g_n = n u / (1 - n u): the
                     bound of a float64 Cholesky factorisation of order n, (n + 1) eps |L| |L|^T, times 2 as in
                     tests/test_gpu_predict_joint.py, plus the rounding of the float64 product that forms L L^T here
  factor, forward    max |L - L_ld| <= cond_2(A) eps max |L_ld| against the long-double factor of the same float64 matrix
  logml              tests/logml_grad_reference.py: bounds() on sum log L_ii and z'z, value_bound() on the value
  gp_condition       tests/posterior_reference.py: condition_bounds()
The context is this module's own; every test puts back the options it sets.
"""
import contextlib
import functools

import numpy as np
import pytest

import logml_grad_reference as lg
import multiround_shapes as ms
import posterior_reference as po
import vjp_reference as vr
from abi_cases import _spd, same_bits

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
LD = np.longdouble
MULTI = tuple(r for r in ms.ROUTES if ms.options(r)["debug_ncu"])       # the routes with multi-round launches
RESTORE = dict(ms.DEFAULTS, small_n1=256, small_gc=180, kernel_timing=0, grid_lanes=0)   # gpmi_tuning_defaults


@pytest.fixture(scope="module")
def mctx():
    import gp_amd
    c = gp_amd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _on(c, route, **extra):
    """The context on one route (plus `extra` options), defaults again afterwards."""
    opts = dict(ms.options(route), **extra)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        yield c
    finally:
        for k in opts:
            c.set_option(k, RESTORE[k])


# ---- references, once per process -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _potrf_case(n):
    """(A, long-double factor of A, cond_2(A)): the matrix of test_potrf_vs_oracle -- a squared-exponential covariance of
    uniform points in the unit square (alpha = 1, rho = 0.3) plus 0.05 I -- in float64, the same bits for device and reference."""
    rng = np.random.default_rng(n)
    X = rng.random((n, 2))
    A = np.asfortranarray(vr.se_cov(X, 1.0, [0.3], 0.05)[0])
    A = np.tril(A) + np.tril(A, -1).T          # exactly symmetric
    ev = np.linalg.eigvalsh(A)
    L = vr._chol_ld(A.astype(LD))
    A.setflags(write=False)
    L.setflags(write=False)
    return A, L, float(ev[-1] / ev[0])


def _backward_ratio(L, A):
    """Worst |fl(L L^T) - A| / bound over the entries (module docstring)."""
    n = A.shape[0]
    g = n * EPS / 2 / (1.0 - n * EPS / 2)
    bound = (2.0 * (n + 2) * EPS + g) / (1.0 - g) * (np.abs(L) @ np.abs(L).T)
    return float(np.max(np.abs(L @ L.T - A) / bound))


def _factor_ratios(L, A, Lld, cond):
    """(worst |fl(L L^T) - A| / bound, max |L - L_ld| / (cond eps max |L_ld|)) of one factor."""
    fwd = float(np.max(np.abs(L.astype(LD) - Lld)) / (cond * EPS * float(np.max(np.abs(Lld)))))
    return _backward_ratio(L, A), fwd


@functools.lru_cache(maxsize=None)
def _logml_case(n):
    """(inputs, {"out3"} in long double, cond_2(S)) on the inputs of logml_grad_reference.case_inputs(n, 2, isotropic, 0.15):
    the value's part of logml_grad_reference (the same matrix, factor and solve routines), without its n^3 gradient terms."""
    X, y, a, ell, s, jit = lg.case_inputs(n, 2, False, 0.15)
    K = vr.se_cov(X, a, ell, LD(s) * LD(s) + LD(jit), dtype=LD)[0]
    L = vr._chol_ld(K)
    z = vr._fwd_solve_ld(L, np.asarray(y, float).astype(LD))
    sld, q = np.log(np.diag(L)).sum(), z @ z
    two_pi = 2 * LD(4) * np.arctan(LD(1))
    ref = {"out3": np.array([-q / 2 - sld - n * np.log(two_pi) / 2, sld, q], dtype=LD), "grad": np.zeros(1, LD), "gabs": np.zeros(1)}
    cond = lg.cond2(X, a, ell, s, jit)
    assert cond <= lg.COND_MAX
    return (X, y, a, ell, s, jit), ref, cond


def _check_logml(tag, out3, ref, cond, n):
    es, eq, _ = lg.errors(out3, np.zeros(1), ref)
    bs, bq, _ = lg.bounds(ref, cond, n)
    ev, bv = abs(float(LD(out3[0]) - ref["out3"][0])), lg.value_bound(ref, cond, n)
    print("%s: cond %.1e; error / bound: sum_log %.3f, z'z %.3f, value %.3f" % (tag, cond, es / bs, eq / bq, ev / bv))
    assert np.all(np.isfinite(out3)), tag
    assert es <= bs and eq <= bq and ev <= bv, (tag, es / bs, eq / bq, ev / bv)


# ---- 1. the factor, elementwise, on every route and shape -------------------------------------------------------------------
@pytest.mark.parametrize("n", ms.POTRF_N)
@pytest.mark.parametrize("route", list(ms.ROUTES))
def test_factor_elementwise_on_every_route(mctx, route, n):
    """gpmi_potrf: the strict upper triangle exactly zero, the diagonal positive, the componentwise backward bound and the
    forward bound against the long-double factor (module docstring).  Prints the two ratios to their bounds.
    Worst over all routes and shapes on an MI355X: backward 0.0081 and forward 0.0090 of the bound (both on
    ncu12-walk2-ks1-fd15-nbo256); the all-defaults route 0.0076 and 0.0057, the other routes between 0.0066 and 0.0090."""
    A, Lld, cond = _potrf_case(n)
    with _on(mctx, route) as c:
        L = c.potrf(A)
        assert c.debug_counters() == 0
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0) and np.all(np.isfinite(L))
    back, fwd = _factor_ratios(L, A, Lld, cond)
    print("potrf n=%d %s: cond %.1e; backward %.4f of its bound, forward %.4f of its bound" % (n, route, cond, back, fwd))
    assert back <= 1.0 and fwd <= 1.0, (route, n, back, fwd)


# ---- 2. routes that add up the same numbers give the same bits --------------------------------------------------------------
@pytest.mark.parametrize("n", ms.SAME_SUMS_N)
def test_walks_that_add_the_same_numbers_give_the_same_bits(mctx, n):
    """fuse_diag = 0, ksplit = 0, nb_outer = 128 at orders without a thin last tile row: every element of every trailing update
    is computed by gemm_tile, which sums its K = 128 products in an order fixed by the element's place in its 128 x 128 tile
    and by nothing else -- not by the block that owns the tile.  The diagonal blocks and panels run the same unfused kernels.
    So the single-round launch (debug_ncu = 0), the multi-round row-major walk and the band walk (debug_ncu = 8) differ only in
    which block multiplies which tile, and the factors agree bit for bit (tests/test_syrk_walk_host.py checks on the CPU that
    these routes take no quadrant and fuse nothing at these orders).  Where the routine differs -- quadrants, sub-tiles --
    test 1 is the check."""
    A = _potrf_case(n)[0]
    got = {}
    for route in ms.SAME_SUMS:
        with _on(mctx, route) as c:
            got[route] = c.potrf(A)
    for route in ms.SAME_SUMS[1:]:
        assert same_bits(got[ms.SAME_SUMS[0]], got[route]), (n, route, float(np.max(np.abs(got[ms.SAME_SUMS[0]] - got[route]))))


# ---- 3. the path ran --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ms.ROUTES))
def test_the_multi_round_launches_are_the_ones_the_table_says(mctx, route):
    """kernel_timing counts the trailing launches of more than one round of tiles: at every order as many as the shape table
    lists for the route (none on the routes that plan for the device's own CU count), and no counter is left non-zero."""
    total = 0
    for n in ms.POTRF_N:
        A = _potrf_case(n)[0]
        with _on(mctx, route, kernel_timing=1) as c:
            c.kernel_timing(reset=True)
            c.potrf(A)
            kt = c.kernel_timing(reset=True)
            assert c.debug_counters() == 0
        want = ms.multi_round_updates(route, "potrf-%d" % n)
        assert int(kt["syrk_multi_round"][0]) == want, (route, n, kt["syrk_multi_round"], want)
        assert int(kt["syrk"][0]) == len(ms.updates(n, n, n, ms.options(route)["nb_outer"]))
        total += want
    assert (total > 0) == bool(ms.options(route)["debug_ncu"]), (route, total)


# ---- 4. augmented row and trapezoids ----------------------------------------------------------------------------------------
# (route, shape) pairs the shape table lists with at least one multi-round update (at nb_outer = 256 the smaller ones have none)
LOGML_ON = [(r, n) for r in MULTI for n in ms.LOGML_N if ms.multi_round_updates(r, "logml-%d" % n)]
COND_ON = [(r, nm) for r in MULTI for nm in ms.COND_NM if ms.multi_round_updates(r, "cond-%d-%d" % nm)]


@pytest.mark.parametrize("route,n", LOGML_ON, ids=["%s-%d" % rn for rn in LOGML_ON])
def test_logml_chain_with_its_augmented_row(mctx, route, n):
    """gpmi_logml on the chain: n + 1 rows over n columns, n a multiple of 128 -- every trailing update is a trapezoid (one tile
    row more than tile columns) whose last tile row holds ONE valid row."""
    (X, y, a, ell, s, jit), ref, cond = _logml_case(n)
    with _on(mctx, route, small_n1=0, kernel_timing=1) as c:
        c.kernel_timing(reset=True)
        out3 = np.array(c.logml(X, y, a, ell, s, jit))
        kt = c.kernel_timing(reset=True)
        assert c.debug_counters() == 0
    assert int(kt["syrk_multi_round"][0]) == ms.multi_round_updates(route, "logml-%d" % n) > 0
    _check_logml("logml n=%d %s" % (n, route), out3, ref, cond, n)


@pytest.mark.parametrize("route,nm", COND_ON, ids=["%s-%dx%d" % (r, nm[0], nm[1]) for r, nm in COND_ON])
def test_gp_condition_chain_with_its_rectangular_trailing_block(mctx, route, nm):
    """gpmi_gp_condition on the chain: the first n of n + m columns are factored, the m x m Schur complement and the row of the
    mean are what the trailing updates leave.  (300, 980) is the shape whose updates are trapezoids (n + m = 1280)."""
    case = (nm[0], nm[1], 0)
    inp, ref, cond = po.cond_reference(case)
    t, ts, y, a, l, s2, jit, kinds, compat = inp
    with _on(mctx, route, small_gc=0, kernel_timing=1) as c:
        c.kernel_timing(reset=True)
        mn, Kn = c.gp_condition(t, ts, y, a, l, s2, jit, *kinds)
        kt = c.kernel_timing(reset=True)
        assert c.debug_counters() == 0
    assert int(kt["syrk_multi_round"][0]) == ms.multi_round_updates(route, "cond-%d-%d" % nm) > 0
    bm, bk = po.condition_bounds(ref, cond)
    em = float(po.errors(mn, ref["mn"]).max() / bm)
    ek = float(po.ratios(Kn, ref["Kn"], bk).max())
    print("gp_condition %s %s: cond %.1e; error / bound: mn %.3f, Kn %.3f" % (nm, route, cond, em, ek))
    assert np.all(np.isfinite(mn)) and np.all(np.isfinite(Kn))
    assert em <= 1.0 and ek <= 1.0, (route, nm, em, ek)


# ---- 5. under the lanes -----------------------------------------------------------------------------------------------------
def test_grid_lanes_take_the_row_major_tail_split_and_match_single_evaluations(mctx):
    """gpmi_logml_grid, four lanes, G = 5, n = 897, debug_ncu = 8: under the lanes every launch walks row-major, multi-round
    ones with the tail split.  Every point equals, bit for bit, the single evaluation on the same context with syrk_order = 0
    (the same plan: the lanes only force the walk), and meets the bounds of test 4."""
    n = ms.LANES_N
    X, y, a, ell, s, jit = lg.case_inputs(n, 2, False, 0.15)
    alpha = np.array([1.0, 1.1, 1.2, 0.9, 1.2]); rho = np.array([0.8, 0.9, 0.7, 1.0, 0.85]); sig = np.array([0.15, 0.12, 0.2, 0.15, 0.1])
    with _on(mctx, ms.route_id(8, 2, 1, 15, 128), grid_lanes=4) as c:
        out, info = c.logml_grid(X, y, alpha, rho, sig, jit)
        assert c.debug_counters() == 0
    assert np.all(info == 0)
    with _on(mctx, ms.route_id(8, 0, 1, 15, 128)) as c:
        single = np.array([c.logml(X, y, alpha[g], [rho[g]], sig[g], jit) for g in range(5)])
        assert c.debug_counters() == 0
    assert same_bits(out, single), np.max(np.abs(out - single))
    for g in range(5):
        K = vr.se_cov(X, alpha[g], [rho[g]], LD(sig[g]) * LD(sig[g]) + LD(jit), dtype=LD)[0]
        L = vr._chol_ld(K)
        z = vr._fwd_solve_ld(L, np.asarray(y, float).astype(LD))
        sld, q = np.log(np.diag(L)).sum(), z @ z
        ref = {"out3": np.array([-q / 2 - sld - n * np.log(2 * LD(4) * np.arctan(LD(1))) / 2, sld, q], dtype=LD),
               "grad": np.zeros(1, LD), "gabs": np.zeros(1)}
        _check_logml("lanes point %d" % g, out[g], ref, lg.cond2(X, alpha[g], [rho[g]], sig[g], jit), n)


# ---- 7. the hook itself -----------------------------------------------------------------------------------------------------
def test_debug_ncu_is_checked_restored_and_per_context(mctx):
    """3, -1 and the device's count + 1 are GPMI_EARG and change nothing; 0 after 8 restores the device's count; a second context
    keeps its own.  "Nothing changed" is read from the bits of a factor whose plan depends on the count (n = 896)."""
    import gp_amd
    A = _spd(896)
    fresh = gp_amd.Context(0)
    other = gp_amd.Context(0)
    try:
        want = fresh.potrf(A)
        for bad in (3, -1, 1, 2, 1 << 20):
            with pytest.raises(gp_amd.GpmiError) as e:
                mctx.set_option("debug_ncu", bad)
            assert e.value.code == -1
            assert same_bits(mctx.potrf(A), want), bad
        lo, hi = 4, 1 << 20        # the device's count by bisection on a third context: lo is accepted, hi is not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            try:
                other.set_option("debug_ncu", mid)
                lo = mid
            except gp_amd.GpmiError:
                hi = mid
        other.set_option("debug_ncu", 0)
        ncu = lo
        assert ncu >= 8
        with pytest.raises(gp_amd.GpmiError):
            mctx.set_option("debug_ncu", ncu + 1)
        assert same_bits(mctx.potrf(A), want)
        try:
            mctx.set_option("debug_ncu", ncu)      # the device's own count, stated: the default plan
            assert same_bits(mctx.potrf(A), want)
            mctx.set_option("debug_ncu", 8)
            with pytest.raises(gp_amd.GpmiError):
                mctx.set_option("debug_ncu", 3)    # rejected: 8 stays
            mctx.set_option("kernel_timing", 1)
            mctx.kernel_timing(reset=True)
            L8 = mctx.potrf(A)
            assert int(mctx.kernel_timing(reset=True)["syrk_multi_round"][0]) == 1    # M = 768: 21 tiles on 16 slots
            assert same_bits(other.potrf(A), want)                                    # the second context is unaffected
        finally:
            mctx.set_option("debug_ncu", 0)
            mctx.set_option("kernel_timing", 0)
        assert same_bits(mctx.potrf(A), want)
        assert np.all(np.isfinite(L8)) and _backward_ratio(L8, A) <= 1.0   # the multi-round factor is a factor of A (test 1's bound)
        assert mctx.debug_counters() == 0
    finally:
        fresh.close()
        other.close()
