"""GPU: gpmi_centered_gp_lp_grad[_dev] -- the centred latent GP's log-density and gradient with one factorisation -- against
the long-double reference of tests/centered_gp_reference.py, against gpmi_logml_grad (code already in the tree), and against
itself across paths (one workgroup / blocked chain), calls, entry points and numbers of columns; the model-level function
gp_amd.stan_models.heteroscedastic_centered_log_prob_grad on top of it.

The bounds.  Both sides factor the same matrix backward-stably, so their forward errors are c(n) cond_2(Sigma) eps with
different constants: tests/test_centered_gp_reference.py holds the float64 reference under 1 cond eps on every parity input
(and cond <= 2e7); the device gets 10 cond eps for out[2], out[3], prior (relative) and Fgrad (max norm relative to max|Fgrad|).
The hyper-gradient is a sum of n^2 products that cancel (a difference of terms up to 1e6 times its size), so per theta
|grad - ref| <= 10 cond eps max|grad| + 32 eps gabs_theta, gabs_theta the sum of the absolute terms: a tiled or pairwise
fixed-order sum of n^2 terms errs by at most ceil(log2 n^2) eps sum|t| <= 19 eps sum|t| for n <= 700, rounded up to 32."""
import ctypes as C
import math

import numpy as np
import pytest

import centered_gp_reference as cr
import latent_lik_reference as lr

pytestmark = pytest.mark.gpu

EPS = cr.EPS
J = cr.PARITY_JITTER


@pytest.fixture(scope="module")
def chain_ctx():
    """A second context whose centred call always takes the blocked chain."""
    import gp_amd
    c = gp_amd.Context(0)
    c.set_option("small_cen", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wg_ctx():
    """A third context whose centred call takes one workgroup wherever it can (n <= 256, D <= 8, k <= 8): the default
    threshold is the measured crossover of the two paths, below 256."""
    import gp_amd
    c = gp_amd.Context(0)
    c.set_option("small_cen", 256)
    yield c
    c.close()


def _call(c, family, inp, jitter=J, **kw):
    X, a, ell, F, Y, sg = inp
    return c.centered_gp_lp_grad(X, a, ell, F, family, Y, sg, jitter, **kw)


def _same(r1, r2):
    for key in ("lp", "dlik_dsigma", "sum_log_diag", "quad"):
        assert r1[key] == r2[key], key
    np.testing.assert_array_equal(r1["Fgrad"], r2["Fgrad"])
    np.testing.assert_array_equal(r1["grad"], r2["grad"])


def _check_against(r, ref, cond, label, mult=10.0):
    """The parity bounds (module docstring) of a result dict against a reference dict; prints the achieved multiples of cond eps."""
    e = cr.reference_errors(r, ref)
    ce = cond * EPS
    gmax = float(np.max(np.abs(ref["grad"])))
    gb = mult * ce * gmax + 32.0 * EPS * ref["gabs"]
    print("%s: cond %.1e; in cond eps: sum_log %.3f quad %.3f prior %.3f Fgrad %.3f grad %.3f; grad error / its bound %.3f" % (
        label, cond, e["sum_log_diag"] / ce, e["quad"] / ce, e["prior"] / ce, e["Fgrad"] / ce, e["grad"] / ce,
        float(np.max(e["grad_abs"] / gb))))
    for key in ("sum_log_diag", "quad", "prior", "Fgrad"):
        assert e[key] <= mult * ce, (label, key, e[key] / ce)
    assert np.all(e["grad_abs"] <= gb), (label, e["grad_abs"] / gb)


def _check_head(c, family, inp, r, ref, cond):
    """lik, d lik / d sigma and the head's adjoint on the given F, relative to the sums of their absolute terms (HEAD_TOL, as
    test_gpu_latent_lik.py::test_parity).  lik = out[0] - prior is formed from two rounded numbers: 4 eps (|lp| + |prior|) on
    top.  Fbar_head = Fgrad + A_ref with the reference's A: the device's own A errs by up to the Fgrad bound, 10 cond eps
    max|Fgrad|, which comes on top of the head's error.  And free of that term -- the "none" call on the same path returns -A
    with the bits this call subtracted -- as Fgrad - Fgrad_none, two roundings of |Fgrad| + |A| on top of the head's own
    error."""
    X, a, ell, F, Y, sg = inp
    lik, ds, Fb, asum = lr.head(family, F, Y, sg, dtype=np.longdouble)
    fb_abs, ds_abs = lr.head_abs(family, F, Y, sg)
    assert abs(float(np.longdouble(r["lik"]) - lik)) <= cr.HEAD_TOL * float(asum) + 4 * EPS * (abs(r["lp"]) + abs(r["prior"]))
    if ds_abs:
        assert abs(float(np.longdouble(r["dlik_dsigma"]) - ds)) <= cr.HEAD_TOL * ds_abs
    else:
        assert r["dlik_dsigma"] == 0.0
    k = F.shape[1]
    fbar_ref = (r["Fgrad"].reshape(-1, k).astype(np.longdouble) + ref["A"]).astype(float)
    a_err = 10 * cond * EPS * float(np.max(np.abs(ref["Fgrad"])))
    assert np.all(np.abs(fbar_ref - Fb.astype(float)) <= cr.HEAD_TOL * fb_abs + a_err)
    r0 = c.centered_gp_lp_grad(X, a, ell, F, "none", None, None, J)
    fbar = r["Fgrad"].reshape(-1, k) - r0["Fgrad"].reshape(-1, k)
    slack = 2 * EPS * (np.abs(r["Fgrad"].reshape(-1, k)) + np.abs(r0["Fgrad"].reshape(-1, k)))
    assert np.all(np.abs(fbar - Fb.astype(float)) <= cr.HEAD_TOL * fb_abs + slack)
    assert r0["sum_log_diag"] == r["sum_log_diag"] and r0["quad"] == r["quad"]


@pytest.mark.parametrize("case", cr.parity_cases(), ids=lambda c: "%s-n%d-D%d-ard%d-m%d-k%d" % c)
def test_parity(ctx, wg_ctx, case):
    """n <= 256 by one workgroup (small_cen = 256) and on the default context (the chain above the default threshold); n > 256:
    the chain."""
    family, n, D, ard, m, k = case
    inp, ref, cond = cr.parity_reference(case)
    for c, name in ((wg_ctx, "one workgroup"), (ctx, "default")) if n <= 256 else ((ctx, "chain"),):
        r = _call(c, family, inp)
        assert r["info"] == 0 and r["Fgrad"].shape == (n, k) and r["grad"].shape == (1 + len(inp[2]),)
        assert r["prior"] == -0.5 * r["quad"] - k * r["sum_log_diag"]
        _check_against(r, ref, cond, "%s %s" % (case, name))
        if family == "none":
            assert r["lp"] == r["prior"] and r["dlik_dsigma"] == 0.0
        else:
            _check_head(c, family, inp, r, ref, cond)


@pytest.mark.parametrize("family,D,ard,m,k", [("normal_logsd", 2, True, 5, 2), ("none", 3, False, 1, 3)])
def test_parity_n2100_float64(ctx, family, D, ard, m, k):
    """n = 2100 against the float64 reference alone (long double in Python loops is too slow there), same bounds."""
    n = 2100
    inp = cr.parity_case(family, n, D, ard, m, k)
    X, a, ell, F, Y, sg = inp
    cond = cr.cond2(X, a, ell, J)
    assert cond <= cr.COND_MAX
    ref = cr.centered_reference(X, a, ell, F, family, Y, sg, J)
    r = _call(ctx, family, inp)
    assert r["info"] == 0
    _check_against(r, ref, cond, "%s n=2100 D=%d k=%d (float64 reference)" % (family, D, k))
    if family != "none":
        _check_head(ctx, family, inp, r, ref, cond)


@pytest.mark.parametrize("n", [100, 256, 700, 2100])
@pytest.mark.parametrize("D,ard", [(1, False), (2, True)])
def test_against_the_shipped_gradient(ctx, chain_ctx, wg_ctx, n, D, ard):
    """Family none, k = 1: out[2], out[3] and grad are what gpmi_logml_grad (sigma = 0) computes for y = f -- code already in
    the tree, not numpy.  Each side is within the parity bounds of the truth; so is their difference.  gpmi_logml_grad takes one
    workgroup up to n = 128, its augmented factorisation (order 2n + 1) up to n = 3072; the centred call takes one workgroup up
    to small_cen (256 on the third context) and the plain chain above (it has no augmented route), so the pairs cross routes."""
    inp = cr.parity_case("none", n, D, ard, 1, 1)
    X, a, ell, F, _, _ = inp
    cond = cr.cond2(X, a, ell, J)
    ref = cr.centered_reference(X, a, ell, F, "none", None, None, J)
    out3, g = ctx.logml_grad(X, F[:, 0], a, ell, 0.0, J)
    shipped = {"sum_log_diag": np.longdouble(out3[1]), "quad": np.longdouble(out3[2]),
               "prior": np.longdouble(-0.5 * out3[2] - out3[1]), "Fgrad": ref["Fgrad"], "grad": np.asarray(g[:-1], np.longdouble),
               "gabs": ref["gabs"]}
    for c, name in ((ctx, "default"), (chain_ctx, "chain")) + (((wg_ctx, "one workgroup"),) if n <= 256 else ()):
        r = _call(c, "none", inp)
        r = dict(r, Fgrad=ref["Fgrad"])        # gpmi_logml_grad has no gradient in y: Fgrad is the parity test's business
        _check_against(r, shipped, cond, "n=%d D=%d %s path vs gpmi_logml_grad" % (n, D, name))


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("n", [100, 256])
def test_one_workgroup_and_chain_agree(wg_ctx, chain_ctx, family, n):
    """The path_case layout (D = 2, ARD, about one point per length-scale) with F a draw from the prior: the two paths factor
    Sigma in different block orders, each within the parity bounds of the truth, so their difference is held to the same
    bounds."""
    X, a, ell, Zd, Y, sg = lr.path_case(family if family != "none" else "normal_logsd", n)
    K = cr.vr.se_cov(X, a, ell, J)[0]
    F = np.linalg.cholesky(K) @ Zd
    inp = (X, a, ell, F, None if family == "none" else Y, sg if family == "normal" else None)
    cond = cr.cond2(X, a, ell, J)
    ref = cr.centered_reference(X, a, ell, F, family, inp[4], inp[5], J)
    r1, r2 = _call(wg_ctx, family, inp), _call(chain_ctx, family, inp)
    other = {key: np.longdouble(r2[key]) for key in ("sum_log_diag", "quad", "prior")}
    other.update(Fgrad=r2["Fgrad"].astype(np.longdouble), grad=r2["grad"].astype(np.longdouble), gabs=ref["gabs"])
    _check_against(r1, other, cond, "%s n=%d one workgroup vs chain" % (family, n))
    assert abs(r1["lp"] - r2["lp"]) <= 10 * cond * EPS * abs(r2["lp"])


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("n", [100, 700])
def test_repeated_calls_bit_identical(ctx, chain_ctx, family, n):
    k = 3 if family == "none" else None
    inp = cr.parity_case(family, n, 1, False, 5, k)
    other = cr.parity_case(family, n - 3, 2, True, 1, k, seed=1)
    for c in (ctx, chain_ctx):
        r1 = _call(c, family, inp)
        _call(c, family, other)                      # a different problem in between: nothing of it may linger
        _same(r1, _call(c, family, inp))


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("n", [100, 700])
def test_dev_equals_host(ctx, chain_ctx, family, n):
    """The _dev form on torch tensors with leading dimensions larger than n, bit for bit, on both paths (n = 100: one workgroup
    on the default context, the chain on the other; n = 700: the chain)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    m, D = 5, 2
    k = 3 if family == "none" else cr.k_of(family)
    inp = cr.parity_case(family, n, D, True, m, k)
    X, a, ell, F, Y, sg = inp
    ldx, ldf, ldy, ldfg = n + 3, n + 8, n + 1, n + 5

    def up(A, ld):      # (cols, ld) row-major == ld x cols column-major, rows n .. ld - 1 poisoned
        T = torch.full((A.shape[1], ld), float("nan"), dtype=torch.float64, device=dev)
        T[:, :n] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
        return T
    dX, dF = up(X, ldx), up(F, ldf)
    dY = up(Y, ldy) if Y is not None else None
    for c in (ctx, chain_ctx):
        r = _call(c, family, inp)
        dFg = torch.full((k, ldfg), -3.0, dtype=torch.float64, device=dev)
        dg = torch.zeros(1 + len(ell), dtype=torch.float64, device=dev); dout = torch.zeros(4, dtype=torch.float64, device=dev)
        info = torch.full((1,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        c.centered_gp_lp_grad_dev(dX.data_ptr(), n, ldx, D, a, ell, J, dF.data_ptr(), k, ldf, family,
                                  dY.data_ptr() if dY is not None else None, m, ldy, sg, dout.data_ptr(), dFg.data_ptr(), ldfg,
                                  dg.data_ptr(), info.data_ptr())
        c.sync()
        assert int(info.item()) == 0
        o = dout.cpu().numpy()
        assert o[0] == r["lp"] and o[1] == r["dlik_dsigma"] and o[2] == r["sum_log_diag"] and o[3] == r["quad"]
        got = dFg.cpu().numpy()
        np.testing.assert_array_equal(got[:, :n].T, r["Fgrad"])
        assert np.all(got[:, n:] == -3.0)            # nothing written past row n
        np.testing.assert_array_equal(dg.cpu().numpy(), r["grad"])


@pytest.mark.parametrize("n", [100, 256, 700])
def test_two_columns_against_two_one_column_calls(wg_ctx, chain_ctx, n):
    """k = 2, family none, against the two one-column calls on the same path.  out[2] does not depend on F (the factorisation
    of the leading n x n block never reads the rows below it): its bits are equal on both paths, and that is asserted.
    Fgrad, the chain (n = 700 on both contexts, and every n on the second): the bits ARE equal, and that is asserted -- every
    augmented row is solved by the same per-row panel arithmetic whatever its index and however many rows ride along, and
    A = U Z is computed column by column by the same two kernels.  Fgrad, one workgroup (n = 100, 256 with small_cen = 256):
    the bits differ (measured: 1e-14 .. 5e-14 relative at cond 1e6) -- the one-column call solves its single row with the
    scalar substitution, the two-column call with the MFMA strip, a different order of the same sum -- so there each column is
    held to the parity bound, 10 cond eps, relative to the one-column call.  quad = quad_1 + quad_2 within rounding of the sum;
    grad is not additive in the columns bit for bit on either path (the columns are added inside the contraction)."""
    inp = cr.parity_case("none", n, 2, True, 1, 2)
    X, a, ell, F, _, _ = inp
    cond = cr.cond2(X, a, ell, J)
    ref = cr.centered_reference(X, a, ell, F, "none", None, None, J)
    for c, chain in ((wg_ctx, n > 256), (chain_ctx, True)):
        r = _call(c, "none", inp)
        cols = [c.centered_gp_lp_grad(X, a, ell, F[:, q], "none", None, None, J) for q in range(2)]
        for q in range(2):
            assert cols[q]["sum_log_diag"] == r["sum_log_diag"]
            e = cr.rel(r["Fgrad"][:, q], cols[q]["Fgrad"])
            print("n=%d %s column %d: Fgrad of the two-column call vs the one-column call %.2e (%.3f cond eps)" % (
                n, "chain" if chain else "one workgroup", q, e, e / (cond * EPS)))
            if chain:
                np.testing.assert_array_equal(r["Fgrad"][:, q], cols[q]["Fgrad"])
            else:
                assert e <= 10 * cond * EPS
        assert abs(r["quad"] - (cols[0]["quad"] + cols[1]["quad"])) <= 10 * cond * EPS * r["quad"]
        gsum = cols[0]["grad"] + cols[1]["grad"]
        assert np.all(np.abs(r["grad"] - gsum) <= 10 * cond * EPS * np.max(np.abs(ref["grad"])) + 32 * EPS * ref["gabs"])


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("n", [50, 300])
def test_not_positive_definite(ctx, chain_ctx, family, n):
    """Two coincident points (all of them, here) with jitter 0: the minor's order comes back and every output is NaN, on both
    paths and both forms; the next valid call is unaffected."""
    from gp_amd._lib import NotPositiveDefinite
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    k = 3 if family == "none" else cr.k_of(family)
    X = np.ones((n, 1)); F = np.ones((n, k)); Y = None if family == "none" else np.ones((n, 2))
    sg = 1.0 if family == "normal" else None
    good = cr.parity_case(family, n, 1, False, 1, k)
    for c in (ctx, chain_ctx):
        with pytest.raises(NotPositiveDefinite):
            c.centered_gp_lp_grad(X, 1.0, [1.0], F, family, Y, sg, 0.0)
        r = c.centered_gp_lp_grad(X, 1.0, [1.0], F, family, Y, sg, 0.0, raise_not_pd=False)
        assert 1 < r["info"] <= n
        for key in ("lp", "dlik_dsigma", "sum_log_diag", "quad"):
            assert math.isnan(r[key]), key
        assert np.all(np.isnan(r["Fgrad"])) and np.all(np.isnan(r["grad"]))
        # the _dev form
        dX = torch.ones((1, n), dtype=torch.float64, device=dev); dF = torch.ones((k, n), dtype=torch.float64, device=dev)
        dY = torch.ones((2, n), dtype=torch.float64, device=dev)
        dFg = torch.zeros((k, n), dtype=torch.float64, device=dev); dg = torch.zeros(2, dtype=torch.float64, device=dev)
        dout = torch.zeros(4, dtype=torch.float64, device=dev); info = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        c.centered_gp_lp_grad_dev(dX.data_ptr(), n, n, 1, 1.0, [1.0], 0.0, dF.data_ptr(), k, n, family,
                                  None if family == "none" else dY.data_ptr(), 2, n, sg, dout.data_ptr(), dFg.data_ptr(), n,
                                  dg.data_ptr(), info.data_ptr())
        c.sync()
        assert int(info.item()) == r["info"]
        assert bool(torch.isnan(dout).all()) and bool(torch.isnan(dFg).all()) and bool(torch.isnan(dg).all())
        # the context is usable afterwards
        assert _call(c, family, good)["info"] == 0


def test_bad_arguments(ctx):
    from gp_amd._lib import _p
    n = 10
    X = np.asfortranarray(np.linspace(0, 3, n).reshape(-1, 1)); F = np.ones((n, 3), order="F") * 0.1; Y = np.ones((n, 3), order="F")
    Fg = np.zeros((n, 3), order="F"); g = np.zeros(2); e = np.ones(1); out = np.zeros(4)
    lib, h = ctx._lib, ctx._h
    d = C.c_double

    def call(family=0, k=1, m=3, ldy=n, sigma=1.0, Yp=Y, n_=n, ldx=n, ldf=n, ldfg=n, alpha=1.0, Xp=X, Fp=F, outp=out, Fgp=Fg, gp=g):
        pp = lambda A: None if A is None else _p(A)
        return lib.gpmi_centered_gp_lp_grad(h, pp(Xp), n_, ldx, 1, d(alpha), _p(e), 1, d(1e-6), pp(Fp), k, ldf, family, pp(Yp), m, ldy,
                                            d(sigma), pp(outp), pp(Fgp), ldfg, pp(gp))
    assert call() == 0 and call(family=1) == 0 and call(family=2, k=2) == 0
    for k in (1, 2, 3):                                  # GPMI_LIK_NONE: any k; Y, m, ldy and sigma are ignored
        assert call(family=3, k=k, Yp=None, m=0, ldy=0, sigma=-1.0) == 0
    Yhalf = Y.copy(order="F"); Yhalf[3, 1] = 0.5
    for kw in ({"n_": 0}, {"k": 0}, {"family": 3, "k": 0}, {"ldx": n - 1}, {"ldf": n - 1}, {"ldfg": n - 1}, {"k": 2}, {"family": 1, "k": 2},
               {"family": 2, "k": 1}, {"family": 2, "k": 3}, {"ldy": n - 1}, {"m": 0}, {"sigma": 0.0}, {"sigma": -1.0}, {"sigma": math.nan},
               {"family": 4}, {"family": -1}, {"Xp": None}, {"Fp": None}, {"Yp": None}, {"outp": None}, {"Fgp": None}, {"gp": None},
               {"family": 1, "Yp": Yhalf}, {"alpha": 0.0}):
        assert call(**kw) == -1, kw
    assert call(family=2, k=2, sigma=-1.0) == 0 and call(family=1, sigma=0.0) == 0      # sigma is ignored there
    assert call(family=0, Yp=Yhalf) == 0
    # GPMI_LIK_NONE is still an unknown family to gpmi_latent_gp_lp_grad
    Zb = np.zeros((n, 3), order="F"); o2 = np.zeros(2)
    assert lib.gpmi_latent_gp_lp_grad(h, _p(X), n, n, 1, d(1.0), _p(e), 1, d(1e-6), _p(F), 1, n, 3, _p(Y), 3, n, d(1.0), _p(o2), None, n,
                                      None, n, _p(Zb), n, _p(g)) == -1
    # the _dev form validates before it enqueues anything (host pointers are never dereferenced on these paths)
    assert lib.gpmi_centered_gp_lp_grad_dev(h, None, n, n, 1, d(1.0), _p(e), 1, d(1e-6), None, 1, n, 3, None, 0, 0, d(1.0), None, None, n,
                                            None, None) == -1
    with pytest.raises(Exception):
        ctx.set_option("small_cen", 257)
    with pytest.raises(Exception):
        ctx.centered_gp_lp_grad(X, 1.0, e, F[:, 0], "poisson", Y, 1.0)
    from gp_amd._lib import GpmiError
    with pytest.raises(GpmiError, match="needs Y"):
        ctx.centered_gp_lp_grad(X, 1.0, e, F[:, 0], "normal", None, 1.0)
    with pytest.raises(GpmiError, match="needs sigma"):
        ctx.centered_gp_lp_grad(X, 1.0, e, F[:, 0], "normal", Y)


@pytest.mark.parametrize("n", [1, 2, 15, 17, 63, 65, 255, 257])
def test_ragged_sizes(ctx, chain_ctx, wg_ctx, n):
    """k = 3, family none, against float64 at the parity bounds: the default path, one workgroup (up to 256) and the chain at
    every size (the chain is reachable at n = 1 through small_cen = 0, D > 8 or k > 8)."""
    inp = cr.parity_case("none", n, 2, True, 1, 3)
    X, a, ell, F, _, _ = inp
    cond = cr.cond2(X, a, ell, J)
    ref = cr.centered_reference(X, a, ell, F, "none", None, None, J)
    for c, name in ((ctx, "default"), (wg_ctx, "one workgroup"), (chain_ctx, "chain")):
        r = _call(c, "none", inp)
        assert r["info"] == 0 and r["Fgrad"].shape == (n, 3)
        _check_against(r, ref, cond, "ragged n=%d %s" % (n, name))


@pytest.mark.parametrize("n,D,ard,k", [(300, 9, True, 2), (300, 20, False, 3), (40, 9, False, 9)])
def test_more_than_eight_dimensions_or_columns(ctx, n, D, ard, k):
    """D > 8 takes the chain with the wide k-column contraction (k_grad_partial_big) at every n, and so does k > 8: family none
    against the long-double reference at the parity bounds, above the one-workgroup threshold and below it."""
    inp = cr.parity_case("none", n, D, ard, 1, k)
    X, a, ell, F, _, _ = inp
    cond = cr.cond2(X, a, ell, J)
    assert cond <= cr.COND_MAX
    ref = cr.centered_reference(X, a, ell, F, "none", None, None, J, dtype=np.longdouble)
    r = _call(ctx, "none", inp)
    assert r["info"] == 0 and r["Fgrad"].shape == (n, k) and r["grad"].shape == (1 + len(ell),)
    _check_against(r, ref, cond, "none n=%d D=%d ard=%d k=%d" % (n, D, ard, k))


@pytest.mark.parametrize("n", [10, 100])
def test_model_log_prob_grad(ctx, n):
    """heteroscedastic_centered_log_prob_grad at the reference's own size (N = 10, M = 5, x = linspace) and at N = 100, at the
    model's jitter 1e-9: cond_2(Sigma) is far higher there than on the parity inputs, and the bound is that case's own 10 cond
    eps against long double (tests/test_centered_gp_reference.py::test_model_cases_reference_error holds float64 under 1)."""
    from gp_amd import stan_models
    x, Y, l, sf, mu, s = cr.model_case(n)
    lp, g = stan_models.heteroscedastic_centered_log_prob_grad(x, Y, l, sf, mu, s, ctx=ctx)
    assert g.shape == (2 + 2 * n,)
    e_lp, e_g, cond = cr.model_errors(lp, g, x, Y, l, sf, mu, s)
    print("model N=%d: cond %.1e; in cond eps: lp %.3f gradient %.3f" % (n, cond, e_lp / (cond * EPS), e_g / (cond * EPS)))
    assert e_lp <= 10 * cond * EPS and e_g <= 10 * cond * EPS


def test_rejected_proposal(ctx):
    """Not positive definite (coincident points, no jitter): (-inf, NaN), as the neighbouring model functions."""
    from gp_amd import stan_models
    n = 40
    lp, g = stan_models.heteroscedastic_centered_log_prob_grad(np.ones(n), np.ones((n, 5)), 0.1, 1.0, np.ones(n), np.ones(n), ctx=ctx,
                                                               jitter=0.0)
    assert lp == -math.inf and g.shape == (2 + 2 * n,) and np.all(np.isnan(g))
