"""CPU: the reference of the derivative-observation posteriors (tests/posterior_reference.py): float64 against long double on
every parity input within HALF of every bound that tests/test_gpu_posterior_parity.py gives the device (the draw: within the
device's bound, and within half of the wider CPU bound of the module docstring), a second and a third float64 order of the sums
within the same halves, each measured constant the smallest power of two that does, the long-double
route against the oracle's LU / QR formulas and the stored posterior of tests/golden/gp_derivs.json, the two conditions on the
inputs (cond_2 <= COND_MAX; the bound on every diagonal entry <= jitter / 8, so that a jitter dropped or doubled is sixteen
bounds away), and the mutation checks: a float64 evaluation with one thing wrong leaves the bound on every case it applies to."""
import numpy as np
import pytest

import posterior_reference as po

LD = po.LD
KERNEL_IDS = po.KINDS + ("RR-compat",)


def _kernel_cases(kind):
    compat = kind == "RR-compat"
    kd = "RR" if compat else kind
    for l in po.KERNEL_LS:
        for n, m in po.KERNEL_RECTS:
            x, y = po.kernel_points(n, m, l)
            yield kd, compat, l, x, y


def _kernel_worst(c_k, c_f):
    """(worst float64 error / bound where e is a normal number, worst elsewhere) over every kernel input."""
    normal = tail = 0.0
    for kind in KERNEL_IDS:
        for kd, compat, l, x, y in _kernel_cases(kind):
            K64 = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, compat)[0]
            K, ab, arg = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, compat, LD)
            r = po.ratios(K64, K, po.kernel_bound(kd, ab, arg, po.KERNEL_ALPHA, l, compat, c_k, c_f))
            big = arg < 700.0
            normal = max(normal, float(r[big].max()))
            if not big.all():
                tail = max(tail, float(r[~big].max()))
    return normal, tail


@pytest.mark.parametrize("kind", KERNEL_IDS)
def test_kernels_float64_against_long_double(kind):
    worst = 0.0
    seen_zero = seen_far = seen_sub = False
    for kd, compat, l, x, y in _kernel_cases(kind):
        K64 = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, compat)[0]
        K, ab, arg = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, compat, LD)
        r = po.ratios(K64, K, po.kernel_bound(kd, ab, arg, po.KERNEL_ALPHA, l, compat))
        worst = max(worst, float(r.max()))
        seen_zero |= bool(np.any(arg == 0.0))
        seen_far |= bool(np.any(arg > 745.0))
        seen_sub |= bool(np.any((arg > 709.0) & (arg < 745.0)))
        # the closed form that the floor uses is the polynomial of deriv_cov
        ok = (arg < 600.0)
        e = np.exp(-arg[ok])
        np.testing.assert_allclose(po.poly_abs(kd, arg[ok], po.KERNEL_ALPHA, l, compat) * e, ab[ok], rtol=1e-12, atol=1e-300)
    print("%s: worst float64 error / bound %.3f" % (kind, worst))
    assert worst <= 0.5
    assert seen_zero and seen_far and seen_sub


def test_transposed_kinds_and_symmetries():
    x, y = po.kernel_points(17, 23, 0.6)
    for kind, base in po.SWAPPED.items():
        assert np.array_equal(po.deriv_cov(kind, x, y, 1.3, 0.6)[0], po.deriv_cov(base, y, x, 1.3, 0.6)[0].T)
    for kind in ("QQ", "RR", "TT"):
        K = po.deriv_cov(kind, x, x, 1.3, 0.6, dtype=LD)[0]
        assert np.array_equal(K, K.T)
    # odd orders are antisymmetric, QT = TQ = -RR
    assert np.array_equal(po.deriv_cov("QR", x, x, 1.3, 0.6)[0], -po.deriv_cov("RQ", x, x, 1.3, 0.6)[0])
    assert np.array_equal(po.deriv_cov("QT", x, y, 1.3, 0.6)[0], -po.deriv_cov("RR", x, y, 1.3, 0.6)[0])
    # each kind is the derivative of its neighbour: central differences of the long-double value
    h = LD(1e-5)
    xs, ys = x[:6], y[7:12]
    for kind, base, wrt in (("QR", "QQ", "y"), ("RQ", "QQ", "x"), ("RR", "QR", "x"), ("QT", "QR", "y"), ("TQ", "RQ", "x"),
                            ("RT", "QT", "x"), ("TR", "TQ", "y"), ("TT", "RT", "x")):
        def f(dx, dy):
            xx = (xs.astype(LD) + dx); yy = (ys.astype(LD) + dy)
            r = (yy[None, :] - xx[:, None]) if base in po.SWAPPED else (xx[:, None] - yy[None, :])
            l2 = LD(0.6) * LD(0.6)
            e = np.exp(-(r * r) / (2 * l2))
            t = po._terms(po.SWAPPED.get(base, base), r, l2, 6)
            return e * sum(t[1:], t[0])
        fd = (f(h, 0) - f(-h, 0)) / (2 * h) if wrt == "x" else (f(0, h) - f(0, -h)) / (2 * h)
        want = po.deriv_cov(kind, xs, ys, 1.0, 0.6, dtype=LD)[0]
        assert float(np.max(np.abs(fd - want))) <= 1e-7 * float(np.max(np.abs(want))), kind


def _second_routes(orc, inp):
    t, ts, y, a, l, s2, jit, kinds, compat = inp
    p = po.condition_parts(t, ts, y, a, l, s2, jit, kinds, compat, chol=lambda K: orc.cholesky(K, blocked=True))
    return (("schur", po.condition_schur(*inp)), ("blocked", (p["mn"], p["Kn"])))


@pytest.mark.parametrize("case", po.COND_CASES, ids=po.case_id)
def test_condition_float64_against_long_double(orc, case):
    inp, ref, cond = po.cond_reference(case)
    _, r64, _ = po.cond_reference(case, False)
    jit = inp[6]
    bm, bk = po.condition_bounds(ref, cond)
    assert cond <= po.COND_MAX, cond
    assert np.max(np.diag(bk)) <= jit / 8, np.max(np.diag(bk)) / jit
    for name, (mn, Kn) in (("lapack", (r64["mn"], r64["Kn"])),) + _second_routes(orc, inp):
        em = float(po.errors(mn, ref["mn"]).max() / bm)
        ek = float(po.ratios(Kn, ref["Kn"], bk).max())
        print("%s %s: cond %.1e; float64 error / the device's bound: mn %.3f, Kn %.3f" % (po.case_id(case), name, cond, em, ek))
        assert em <= 0.5 and ek <= 0.5, (name, em, ek)


def _sd_routes(orc, case, b):
    t, ts, Y, P, Z, jit = po.sd_inputs(*case)
    l, a, sy = P[b]
    blocked = lambda K: orc.cholesky(K, blocked=True)   # noqa: E731
    yield "lapack", po.sd_reference(case, b, False)["mu"], po.sd_reference(case, b, False)["draw"]
    mu, _, d = po.sample_derivs(t, ts, Y[:, b], l, a, sy, jit, Z[:, b], schur=True)
    yield "schur", mu, d
    p = po.condition_parts(t, ts, Y[:, b], a, l, sy * sy, jit, ("QQ", "RQ", "RR"), chol=blocked)
    yield "blocked", p["mn"], p["mn"] + blocked(p["Kn"]) @ Z[:, b]


@pytest.mark.parametrize("case", po.SD_SIZES, ids=lambda c: "n%d-m%d-B%d" % c)
def test_sample_derivs_float64_against_long_double(orc, case):
    for b in range(case[2]):
        ref = po.sd_reference(case, b)
        assert ref["cond"] <= po.COND_MAX and ref["cond_cov"] <= po.COND_MAX, (ref["cond"], ref["cond_cov"])
        assert np.max(np.diag(po.condition_bounds(ref["parts"], ref["cond"])[1])) <= po.SD_JITTER / 8
        for name, mu, d in _sd_routes(orc, case, b):
            em = float(po.errors(mu, ref["mu"]).max() / ref["mu_bound"])
            e = float(po.errors(d, ref["draw"]).max())
            ed, ec = e / ref["draw_bound"], e / ref["draw_bound_cpu"]
            print("n%d m%d draw %d %s: cond %.1e, cond(cov) %.1e; float64 error / the device's bound: mu %.3f, draw %.3f (%.3f of the CPU bound)"
                  % (case[0], case[1], b, name, ref["cond"], ref["cond_cov"], em, ed, ec))
            # the draw: within the device's bound, and within half of the one that allows for the size of cov's two terms
            assert em <= 0.5 and ed <= 1.0 and ec <= 0.5, (name, em, ed, ec)


@pytest.mark.parametrize("case", po.SEQ_CASES, ids=lambda c: "n%d-D%d-steps%d" % c)
def test_sampler_float64_against_long_double(case):
    inp, out, commits, bm, bv, ct, cs = po.seq_reference(case)
    X, mn, Kn, a, ell, jit, pts, z = inp
    assert ct <= po.COND_MAX and cs <= po.COND_MAX, (ct, cs)
    assert bv <= jit / 8, bv / jit
    assert float(out[:, 1].min()) > 0 and case[2] > 256 + 3
    o64 = po.seq_chain(X, mn, Kn, a, ell, jit, pts, commits)
    e = po.errors(o64, out)
    print("n%d D%d: cond(K~) %.1e, cond(K*) %.1e; float64 error / the device's bound: condMean %.3f, condVar %.3f"
          % (case[0], case[1], ct, cs, e[:, 0].max() / bm, e[:, 1].max() / bv))
    assert e[:, 0].max() <= 0.5 * bm and e[:, 1].max() <= 0.5 * bv
    # the chain that is given its commits reproduces the chain that drew them, bit for bit in long double
    again = po.seq_chain(X, mn, Kn, a, ell, jit, pts, commits, LD)
    assert np.array_equal(again, out)


def test_constants_are_the_smallest_powers_of_two(orc):
    """With half of C_K, C_F or C_D the float64 route (for C_D: one of its three orders of the sums) leaves half of the bound
    on some parity input.  C_S = 1 is one rounding per term of the entry's own sum: no parity input needs it (the worst Kn entry
    uses 0.06 of the bound, at n = 1), and a smaller constant would not be a rounding model."""
    for c in (po.C_K, po.C_F, po.C_S, po.C_D):
        assert c > 0 and 2.0 ** round(np.log2(c)) == c
    assert po.C_S == 1.0
    normal, tail = _kernel_worst(po.C_K, po.C_F)
    half_n, _ = _kernel_worst(po.C_K / 2, po.C_F)
    _, half_t = _kernel_worst(po.C_K, po.C_F / 2)
    print("kernels: worst %.3f (normal e), %.3f (subnormal e); with C_K / 2 %.3f, with C_F / 2 %.3f" % (normal, tail, half_n, half_t))
    assert normal <= 0.5 and tail <= 0.5 and half_n > 0.5 and half_t > 0.5
    worst = worst_half = 0.0
    for case in po.SD_SIZES:
        for b in range(case[2]):
            ref = po.sd_reference(case, b)
            half = po.draw_bound(ref["mu_bound"], ref["cond_cov"], ref["parts"], ref["draw"], c_d=po.C_D / 2)
            for _, _, d in _sd_routes(orc, case, b):
                e = float(po.errors(d, ref["draw"]).max())
                worst, worst_half = max(worst, e / ref["draw_bound_cpu"]), max(worst_half, e / half)
    print("draws: worst %.3f; with C_D / 2 %.3f" % (worst, worst_half))
    assert worst <= 0.5 < worst_half


# ---- the long-double route against formulas of another shape ---------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in po.COND_CASES if c[0] + c[1] <= 400], ids=po.case_id)
def test_condition_equals_the_lu_formula(orc, case):
    inp, ref, _ = po.cond_reference(case)
    t, ts, y, a, l, s2, jit, kinds, compat = inp
    K, Ks, Kss = (po.deriv_cov(k, u, v, a, l, compat)[0] for k, u, v in ((kinds[0], t, t), (kinds[1], ts, t), (kinds[2], ts, ts)))
    mn, Kn = orc.gp_condition(K, Ks, Kss, y, s2, jit)
    assert po.errors(mn, ref["mn"]).max() <= 1e-9 * np.abs(mn).max()
    assert po.errors(Kn, ref["Kn"]).max() <= 1e-9 * np.abs(Kss).max()
    if not compat:   # ... and the kernels against the oracle's
        for k, u, v, M in ((kinds[0], t, t, K), (kinds[1], ts, t, Ks), (kinds[2], ts, ts, Kss)):
            np.testing.assert_allclose(M, orc.deriv_cov(k, u, v, a, l), rtol=1e-12, atol=1e-14 * np.abs(M).max())


def test_sample_derivs_moments_equal_the_oracle():
    from oracle import oracle as orc
    orc.build()
    t, _, Y, P, Z, _ = po.sd_inputs(25, 25, 3)
    l, a, sy = P[1]
    mu, cov, draw = po.sample_derivs(t, t, Y[:, 1], l, a, sy, 1e-8, Z[:, 1], LD)
    mu_o, cov_o = orc.sample_derivs_moments(t, Y[:, 1], l, a, sy, 1e-8)
    assert po.errors(mu_o, mu).max() <= 1e-9 * np.abs(mu_o).max()
    assert po.errors(cov_o, cov).max() <= 1e-9 * np.abs(cov_o).max()
    assert po.errors(mu_o + np.linalg.cholesky((cov_o + cov_o.T) / 2) @ Z[:, 1], draw).max() <= 1e-6 * np.abs(mu_o).max()


def test_sampler_equals_the_qr_restatement(orc):
    """orc.create_p_dotXnS rebuilds the joint law at every call and conditions with an explicit inverse (jitter 1e-6 on both
    matrices, as here); fed the same commits, its (mu, sigma) are those of the chain.  30 steps of the D = 3 case and of a
    D = 1 case at a spacing where the QR solve keeps nine digits."""
    for n, D in ((40, 3), (30, 1)):
        X, mn, Kn, a, ell, jit, pts, z = po.seq_inputs(n, D, 30)
        if D == 1:
            X = np.asfortranarray(2.0 * X)
            pts = 2.0 * pts
        out, commits = po.seq_commits(X, mn, Kn, a, ell, jit, pts, z)
        g = orc.create_p_dotXnS([X[:, d] for d in range(D)], mn, Kn, a, ell)
        for i in range(30):
            r = g(pts[i], 0.0)
            g.dot_Xs[-1] = commits[i]       # the value committed to the sampler
            assert abs(r["mu"] - float(out[i, 0])) <= 1e-9 * max(1.0, np.abs(commits).max()), i
            assert abs(r["sigma"] - float(out[i, 1])) <= 1e-9 * a * a, i


def test_golden_posterior(golden):
    g = golden["gp_derivs"]["posterior"]
    ts, y = np.array(g["ts"]), np.array(g["y"])
    l, a, s = g["l"], g["a"], g["s"]
    for kind, key in (("QQ", "K"), ("TQ", "KsKi_TQ"), ("TT", "KsKsi_TT")):
        want = np.array(g[key])
        assert po.errors(want, po.deriv_cov(kind, ts, ts, a, l, dtype=LD)[0]).max() <= 1e-14 * np.abs(want).max()
    for kinds, km, kc in ((("QQ", "QQ", "QQ"), "mu_value", "cov_value"), (("QQ", "RQ", "RR"), "mu_deriv", "cov_deriv"),
                          (("QQ", "TQ", "TT"), "mu_second", "cov_second")):
        mn, Kn = po.condition(ts, ts, y, a, l, s * s, 0.0, kinds, dtype=LD)
        mu, cov = np.array(g[km]), np.array(g[kc])
        assert po.errors(mu, mn).max() <= 1e-9 * np.abs(mu).max(), km
        assert po.errors(cov, Kn).max() <= 1e-9 * np.abs(cov).max(), kc


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_cases_are_deterministic_and_cover_what_they_have_to():
    for a, b in zip(po.cond_inputs(21, 30, 7), po.cond_inputs(21, 30, 7)):
        assert np.array_equal(a, b)
    assert {c[2] for c in po.COND_CASES} == set(range(10))                       # the nine triples and compat RR
    one = [c for c in po.COND_CASES if c[0] + c[1] + 1 <= 180]
    chain = [c for c in po.COND_CASES if c[:2] in po.CHAIN_SIZES]
    assert [c[:2] for c in one] == list(po.ONE_LAUNCH_SIZES) and len(chain) == 6
    assert (100 + 79 + 1, 100 + 80 + 1) == (180, 181)
    assert all(n + m <= 650 for n, m, _ in po.COND_CASES) and all(n + m <= 650 for n, m, _ in po.SD_SIZES)
    assert any(n > m for n, m, _ in chain) and any(m > n for n, m, _ in chain)
    for edge in (16, 64, 128, 256):
        dims = [d for c in po.COND_CASES for d in c[:2]]
        assert any(d < edge for d in dims) and any(d > edge for d in dims)
    # transposed kinds (RQ, TQ, TR) and cancelling sums (RR, QT, RT, TT) reach a posterior on both sides of the divide
    for cases in (one, chain):
        used = {k for c in cases for k in po.TRIPLES[c[2]][:3]}
        assert {"RQ", "TQ", "TR"} & used and {"RR", "QT", "RT", "TT"} <= used | {"QT", "RT"}, used
    assert {k for c in po.COND_CASES for k in po.TRIPLES[c[2]][:3]} == set(po.KINDS)
    t, ts, y, a, l, s2, jit, kinds, compat = po.cond_inputs(64, 65, 8)
    assert s2 == 0.01 * a * a * 3 / l ** 4 and jit == 1e-8 * a * a * 3 / l ** 4 and t.size == 64 and ts.size == 65
    assert np.all(np.diff(t) >= 0) and 0 <= t[0] and t[-1] <= 6.4


# ---- each check can fail: a float64 evaluation with one thing wrong leaves the bound -----------------------------------------
def _outside(case, mn, Kn):
    _, ref, cond = po.cond_reference(case)
    bm, bk = po.condition_bounds(ref, cond)
    return float(po.errors(mn, ref["mn"]).max() / bm), float(po.ratios(Kn, ref["Kn"], bk).max())


@pytest.mark.parametrize("case", po.COND_CASES, ids=po.case_id)
def test_mutations_of_the_conditioning_leave_the_bound(case):
    inp, _, _ = po.cond_reference(case)
    t, ts, y, a, l, s2, jit, kinds, compat = inp
    em, ek = _outside(case, *po.condition(*inp))
    assert em <= 0.5 and ek <= 0.5
    # jitter dropped, jitter added twice: Kn alone
    for j in (0.0, 2 * jit):
        em, ek = _outside(case, *po.condition(t, ts, y, a, l, s2, j, kinds, compat))
        assert ek > 1.0, (j, ek)
    # s2 taken as sqrt(s2)
    em, ek = _outside(case, *po.condition(t, ts, y, a, l, np.sqrt(s2), jit, kinds, compat))
    assert em > 1.0 and ek > 1.0, (em, ek)
    # compat flipped on RR (alpha = 1.2: the second term changes by a factor 1.44)
    if "RR" in kinds and case[:2] != (1, 1):     # at n = m = 1 the only pair is coincident: RR(0) has no second term
        em, ek = _outside(case, *po.condition(t, ts, y, a, l, s2, jit, kinds, not compat))
        assert max(em, ek) > 1.0, (em, ek)
    # a transposed kind evaluated as its base form
    if kinds[1] in po.SWAPPED:
        wrong = (kinds[0], po.SWAPPED[kinds[1]], kinds[2])
        em, ek = _outside(case, *po.condition(t, ts, y, a, l, s2, jit, wrong, compat))
        if kinds[1] == "TQ":
            assert em <= 0.5 and ek <= 0.5   # QT is even in r: TQ = QT entry by entry, there is nothing to get wrong
        else:
            assert em > 1.0, em              # RQ = -QR, TR = -RT: the mean changes sign (Kn is even in Ks)
    # TT's middle coefficient 6 taken as 3
    if "TT" in kinds and case[:2] != (1, 1):
        em, ek = _outside(case, *po.condition(t, ts, y, a, l, s2, jit, kinds, compat, tt_mid=3))
        assert max(em, ek) > 1.0, (em, ek)


@pytest.mark.parametrize("kind", ["RQ", "TR", "TT", "RR"])
def test_mutations_of_a_kernel_leave_the_bound(kind):
    for kd, compat, l, x, y in _kernel_cases(kind):
        if x.size == 1:
            continue    # the single pair is coincident
        K, ab, arg = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, compat, LD)
        b = po.kernel_bound(kd, ab, arg, po.KERNEL_ALPHA, l, compat)
        if kind in po.SWAPPED:
            wrong = po.deriv_cov(po.SWAPPED[kd], x, y, po.KERNEL_ALPHA, l)[0]
        elif kind == "TT":
            wrong = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, tt_mid=3)[0]
        else:
            wrong = po.deriv_cov(kd, x, y, po.KERNEL_ALPHA, l, True)[0]
        r = po.ratios(wrong, K, b)
        near = (arg > 0) & (arg < 30)
        assert np.all(r[near] > 1.0), (kind, l, float(r[near].min()))


@pytest.mark.parametrize("case", po.SEQ_CASES, ids=lambda c: "n%d-D%d-steps%d" % c)
def test_mutation_of_the_chain_leaves_the_bound(case):
    inp, out, commits, bm, bv, _, _ = po.seq_reference(case)
    X, mn, Kn, a, ell, jit, pts, z = inp
    wrong = po.seq_chain(X, mn, Kn, a, ell, jit, pts, commits, w_from_var=True)
    e = po.errors(wrong, out)
    assert e[0, 0] <= bm and e[:, 1].max() <= bv      # the first step has no w, the variances never do
    assert e[1:, 0].max() > bm
    # every later step whose row of Ls is not numerically empty feels it
    assert np.mean(e[1:, 0] > bm) > 0.9
