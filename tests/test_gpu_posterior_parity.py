"""GPU: the derivative-observation posteriors against the long-double references of tests/posterior_reference.py --
gpmi_deriv_cov / gpmi_deriv_elem entry by entry (all nine kinds and GPMI_COMPAT_RR, from coincident points to the underflow of the
exponential), gpmi_gp_condition on its three routes (one launch, the chain around the one-workgroup partial factorisation, the
blocked chain) over the nine consistent kind triples, gpmi_sample_derivs[_batch] on both routes with their status codes, and
the sampler gpmi_seq_* stepped past 256 points on commits taken from the long-double chain.  The other GPU tests of this
family compare with a float64 oracle at 1e-8 of the largest entry, which is the size of the jitter.

The bounds and how their constants were measured (on the CPU, float64 against long double): the docstring of
tests/posterior_reference.py; tests/test_posterior_reference.py holds the reference to HALF of each and the inputs to
cond_2 <= 2e7 and bound <= jitter / 8 on every diagonal (the draw's bound, 10 cond(cov) eps max|chol(cov) z| + the bound on
mu, is the exception: the float64 routes meet it, using up to 0.58 of it).  Two device results are compared with twice the bound.
"""
import numpy as np
import pytest

import posterior_reference as po

pytestmark = pytest.mark.gpu

ROUTES = {"one_launch": {},                                     # defaults: small_gc = 180, small_m = 160
          "big_launch": {"small_gc": 1024},
          "chain_wg": {"small_gc": 0, "small_m": 1024},         # launch chain, the partial factorisation by one workgroup
          "blocked": {"small_gc": 0, "small_m": 0},
          "sd_wg": {"small_sdb": 0},                            # one workgroup per draw whatever the batch size
          "sd_lanes": {"small_sd": 0}}                          # a launch chain per draw on the lanes


@pytest.fixture(scope="module")
def routes():
    """One context per route, with its own options (the shared `ctx` keeps its defaults)."""
    import gp_amd
    made = {}
    for name, options in ROUTES.items():
        c = gp_amd.Context(0)
        for k, v in options.items():
            c.set_option(k, v)
        made[name] = c
    yield made
    for c in made.values():
        c.close()


# ---- kernels ---------------------------------------------------------------------------------------------------------------
KERNEL_IDS = po.KINDS + ("RR-compat",)


def _flags(compat, lower=False):
    from gp_amd._lib import COMPAT_RR, FULL, LOWER
    return (COMPAT_RR if compat else FULL) | (LOWER if lower else FULL)


def _check_kernel(tag, got, kd, x, y, alpha, l, compat, mask=None):
    K, ab, arg = po.deriv_cov(kd, x, y, alpha, l, compat, po.LD)
    r = po.ratios(got, K, po.kernel_bound(kd, ab, arg, alpha, l, compat))
    under = np.abs(K) < po.TINY           # the reference underflows: an exact zero or a subnormal, whichever
    if mask is not None:
        r, under, got = r[mask], under[mask], got[mask]
    assert np.all(np.isfinite(got)), tag
    assert np.all(np.abs(got[under]) <= po.TINY), (tag, np.abs(got[under]).max())
    r = np.where(under, 0.0, r)
    assert np.all(r <= 1.0), (tag, float(r.max()))
    return float(r.max()), int(under.sum())


@pytest.mark.parametrize("kind", KERNEL_IDS)
def test_deriv_cov_every_entry(routes, kind):
    ctx = routes["one_launch"]
    compat = kind == "RR-compat"
    kd = "RR" if compat else kind
    worst, n_under = 0.0, 0
    for l in po.KERNEL_LS:
        for n, m in po.KERNEL_RECTS:
            x, y = po.kernel_points(n, m, l)
            got = ctx.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, _flags(compat))
            w, u = _check_kernel("%s l=%g %dx%d" % (kind, l, n, m), got, kd, x, y, po.KERNEL_ALPHA, l, compat)
            worst, n_under = max(worst, w), n_under + u
            # the elementwise entry point on the same pairs, unit amplitude
            if not compat:
                one = ctx.deriv_cov(kd, x, y, 1.0, l)
                assert np.array_equal(ctx.deriv_elem(kd, x[:, None], y[None, :], l), one), (kind, l, n, m)
                _check_kernel("%s l=%g %dx%d alpha=1" % (kind, l, n, m), one, kd, x, y, 1.0, l, False)
        # one symmetric call, lower triangle
        x, _ = po.kernel_points(131, 131, l, seed=1)
        got = ctx.deriv_cov(kd, x, x, po.KERNEL_ALPHA, l, _flags(compat, lower=True))
        w, u = _check_kernel("%s l=%g lower" % (kind, l), got, kd, x, x, po.KERNEL_ALPHA, l, compat, mask=np.tril(np.ones((131, 131), bool)))
        worst, n_under = max(worst, w), n_under + u
    print("deriv_cov %s: worst error / bound %.3f; %d entries where the reference underflows" % (kind, worst, n_under))
    assert n_under > 0


# ---- gp_condition ----------------------------------------------------------------------------------------------------------
def _condition(ctx, inp):
    t, ts, y, a, l, s2, jit, kinds, compat = inp
    return ctx.gp_condition(t, ts, y, a, l, s2, jit, *kinds, flags=_flags(compat))


def _check_condition(tag, mn, Kn, ref, cond, scale=1.0, against=None):
    """error / bound of (mn, Kn) against the long-double parts, or (scale 2) against another device result."""
    bm, bk = po.condition_bounds(ref, cond, scale)
    want = (ref["mn"], ref["Kn"]) if against is None else against
    em = float(po.errors(mn, want[0]).max() / bm)
    ek = float(po.ratios(Kn, want[1], bk).max())
    print("%s: cond %.1e; error / bound: mn %.3f, Kn %.3f" % (tag, cond, em, ek))
    assert np.all(np.isfinite(mn)) and np.all(np.isfinite(Kn)), tag
    assert em <= 1.0 and ek <= 1.0, (tag, em, ek)


COND_ROUTES = ([("one_launch", po.cond_case(*s)) for s in po.ONE_LAUNCH_SIZES]
               + [("big_launch", po.cond_case(*po.BIG_LAUNCH_SIZE))]
               + [(r, po.cond_case(*s)) for r in ("chain_wg", "blocked")
                  for s in po.ONE_LAUNCH_SIZES + (po.NEXT_ROUTE_SIZE, po.BIG_LAUNCH_SIZE) + po.CHAIN_SIZES])


@pytest.mark.parametrize("route,case", COND_ROUTES, ids=["%s-%s" % (r, po.case_id(c)) for r, c in COND_ROUTES])
def test_gp_condition_against_long_double(routes, route, case):
    inp, ref, cond = po.cond_reference(case)
    mn, Kn = _condition(routes[route], inp)
    assert mn.shape == (case[1],) and Kn.shape == (case[1], case[1])
    _check_condition("%s %s" % (route, po.case_id(case)), mn, Kn, ref, cond)
    assert np.array_equal(Kn, Kn.T)


@pytest.mark.parametrize("case", [c for c in po.COND_CASES if c[:2] != po.NEXT_ROUTE_SIZE], ids=po.case_id)
def test_gp_condition_routes_agree(routes, case):
    inp, ref, cond = po.cond_reference(case)
    names = ["chain_wg", "blocked"]
    if case[:2] in po.ONE_LAUNCH_SIZES:
        names.insert(0, "one_launch")
    if case[:2] == po.BIG_LAUNCH_SIZE:
        names.insert(0, "big_launch")
    res = {name: _condition(routes[name], inp) for name in names}
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            _check_condition("%s: %s against %s" % (po.case_id(case), p, q), res[p][0], res[p][1], ref, cond, 2.0, res[q])


def test_gp_condition_takes_the_next_route_past_180_rows(routes):
    """(100, 79) is M = 180 rows exactly: one launch under the defaults; (100, 80) is not, and 181 rows are more than the
    default small_m = 160 too: the blocked chain, bit for bit."""
    case = po.cond_case(*po.NEXT_ROUTE_SIZE)
    inp, ref, cond = po.cond_reference(case)
    mn, Kn = _condition(routes["one_launch"], inp)
    _check_condition("defaults %s" % po.case_id(case), mn, Kn, ref, cond)
    mb, Kb = _condition(routes["blocked"], inp)
    assert np.array_equal(mn, mb) and np.array_equal(Kn, Kb)
    assert np.array_equal(Kn, Kn.T)


# ---- sample_derivs ---------------------------------------------------------------------------------------------------------
def _check_draws(tag, case, draws, mus, info, skip=()):
    worst_mu = worst_d = 0.0
    for b in range(case[2]):
        if b in skip:
            continue
        ref = po.sd_reference(case, b)
        assert info[b] == 0, (tag, b, info)
        em = float(po.errors(mus[:, b], ref["mu"]).max() / ref["mu_bound"])
        ed = float(po.errors(draws[:, b], ref["draw"]).max() / ref["draw_bound"])
        print("%s draw %d: cond %.1e, cond(cov) %.1e; error / bound: mu %.3f, draw %.3f" % (tag, b, ref["cond"], ref["cond_cov"], em, ed))
        worst_mu, worst_d = max(worst_mu, em), max(worst_d, ed)
    assert worst_mu <= 1.0 and worst_d <= 1.0, (tag, worst_mu, worst_d)


@pytest.mark.parametrize("route", ["sd_wg", "sd_lanes"])
@pytest.mark.parametrize("case", po.SD_SIZES, ids=lambda c: "n%d-m%d-B%d" % c)
def test_sample_derivs_against_long_double(routes, route, case):
    import gp_amd
    ctx = routes[route]
    n, m, B = case
    t, ts, Y, P, Z, jit = po.sd_inputs(*case)
    draws, mus, info = ctx.sample_derivs_batch(t, ts, Y, P, jit, Z)
    tag = "%s n%d m%d" % (route, n, m)
    _check_draws(tag, case, draws, mus, info)
    # the single call and B = 1 of the batch: the same route on this context, the same bits
    b = B - 1
    d1, m1 = ctx.sample_derivs(t, ts, Y[:, b], P[b, 0], P[b, 1], P[b, 2], jit, Z[:, b])
    db, mb, ib = ctx.sample_derivs_batch(t, ts, Y[:, b:b + 1], P[b:b + 1], jit, Z[:, b:b + 1])
    assert ib[0] == 0 and np.array_equal(d1, db[:, 0]) and np.array_equal(m1, mb[:, 0])
    ref = po.sd_reference(case, b)
    assert po.errors(m1, ref["mu"]).max() <= ref["mu_bound"] and po.errors(d1, ref["draw"]).max() <= ref["draw_bound"]
    # status n + k: with jitter = -1 the posterior covariance fails at its first pivot, whichever draw; K + sy^2 I is fine
    assert all(float(po.sd_reference(case, k)["cov"][0, 0]) < 1.0 for k in range(B))
    _, _, ineg = ctx.sample_derivs_batch(t, ts, Y, P, -1.0, Z)
    assert np.all(ineg == n + 1), ineg
    with pytest.raises(gp_amd.NotPositiveDefinite) as ei:
        ctx.sample_derivs(t, ts, Y[:, b], P[b, 0], P[b, 1], P[b, 2], -1.0, Z[:, b])
    assert ei.value.order == n + 1
    # status 1 .. n: no noise and a huge length-scale, K is numerically singular; the other draws do not notice either failure
    Pbad = P.copy()
    Pbad[1] = (500.0, P[1, 1], 0.0)
    dbad, mbad, ibad = ctx.sample_derivs_batch(t, ts, Y, Pbad, jit, Z)
    assert 1 <= ibad[1] <= n, ibad
    keep = np.arange(B) != 1
    assert np.all(ibad[keep] == 0) and np.array_equal(dbad[:, keep], draws[:, keep]) and np.array_equal(mbad[:, keep], mus[:, keep])
    again, mus2, info2 = ctx.sample_derivs_batch(t, ts, Y, P, jit, Z)
    assert np.all(info2 == 0) and np.array_equal(again, draws) and np.array_equal(mus2, mus)


@pytest.mark.parametrize("case", po.SD_SIZES, ids=lambda c: "n%d-m%d-B%d" % c)
def test_sample_derivs_routes_agree(routes, case):
    t, ts, Y, P, Z, jit = po.sd_inputs(*case)
    dw, mw, _ = routes["sd_wg"].sample_derivs_batch(t, ts, Y, P, jit, Z)
    dl, ml, _ = routes["sd_lanes"].sample_derivs_batch(t, ts, Y, P, jit, Z)
    for b in range(case[2]):
        ref = po.sd_reference(case, b)
        bd = po.draw_bound(2.0 * ref["mu_bound"], ref["cond_cov"], ref["parts"], ref["draw"], 2.0)
        em = float(np.abs(mw[:, b] - ml[:, b]).max() / (2.0 * ref["mu_bound"]))
        ed = float(np.abs(dw[:, b] - dl[:, b]).max() / bd)
        print("n%d m%d draw %d, one workgroup against the lanes: difference / twice the bound: mu %.3f, draw %.3f" % (case[0], case[1], b, em, ed))
        assert em <= 1.0 and ed <= 1.0


# ---- the sampler past 256 steps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", po.SEQ_CASES, ids=lambda c: "n%d-D%d-steps%d" % c)
def test_sampler_past_256_steps(routes, case):
    import gp_amd
    n, D, steps = case
    inp, out, commits, bm, bv, ct, cs = po.seq_reference(case)
    X, mn, Kn, a, ell, jit, pts, z = inp
    s = routes["one_launch"].seq_sampler(X, mn, Kn, a, ell, jit, max_steps=steps)
    got = np.empty((steps, 2))
    try:
        for i in range(steps):
            if i == po.SEQ_SKIP:     # a step that is not committed is discarded by the next one
                s.step(pts[(i + 7) % steps] + 0.25)
                assert s.count == i
            got[i] = s.step(pts[i])
            s.commit(commits[i])
        assert s.count == steps
        with pytest.raises(gp_amd.GpmiError):
            s.step(pts[0])
        assert s.count == steps
    finally:
        s.close()
    e = po.errors(got, out)
    im, iv = int(np.argmax(e[:, 0])), int(np.argmax(e[:, 1]))
    print("sampler n%d D%d: cond(K~) %.1e, cond(K*) %.1e; error / bound: condMean %.3f (step %d), condVar %.3f (step %d); past step 256: %.3f, %.3f"
          % (n, D, ct, cs, e[im, 0] / bm, im, e[iv, 1] / bv, iv, e[256:, 0].max() / bm, e[256:, 1].max() / bv))
    assert np.all(np.isfinite(got))
    assert np.all(e[:, 0] <= bm) and np.all(e[:, 1] <= bv)
