"""GPU: the Hermite-eigenfunction low-rank GP (gpmi_hermite_basis, gpmi_lowrank_logml_grad, gpmi_lowrank_latent_lp_grad and their
_dev forms) against tests/lowrank_reference.py -- the 50-digit closed form, the n x n long-double factorisation, the long-double
heads -- within that module's bounds (this file has no tolerance of its own beyond the ones reasoned where they stand), the
layout and NULL conventions of the C ABI, bit-for-bit agreement of the two forms, of repeated calls and of calls after
gpmi_debug_fill, the models' own convergence check against gpmi_se_cov / gpmi_logml_grad, the westbrook fixture, the status and
every GPMI_EARG case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import logml_grad_reference as lg
import lowrank_reference as lr

pytestmark = pytest.mark.gpu
LD = np.longdouble
SC, AMP, SIG = lr.SCALE, lr.AMP, lr.SIGMA
ALL_CASES = lr.CASES + lr.BIG_CASES
FAMILIES = ((lr.NORMAL, "normal"), (lr.BERNOULLI, "bernoulli_logit"))
cid = lambda c: "n%d_M%d_l%g" % c
SENT = -5.25


@pytest.fixture(scope="module")
def ctx():
    import gp_amd
    c = gp_amd.Context(0)
    yield c
    c.close()


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _d(v):
    return C.c_double(float(v))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, float)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _Y(case, fam):
    Y = lr.case_inputs(*case)[3]
    return Y if fam == lr.NORMAL else Y[:, :1]


# ---- against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=cid)
def test_basis_against_the_closed_form(ctx, case):
    n, M, l = case
    x = lr.case_inputs(*case)[0]
    Pr, Dr = lr.basis_ld(x, M, SC, AMP, l)
    bP, bD = lr.basis_bounds(Pr, Dr, l)
    P, D = ctx.hermite_basis(x, M, SC, AMP, l, want_dl=True)
    r = lr.worst_ratio(P, Pr, bP), lr.worst_ratio(D, Dr, bD)
    print(case, "Phi %.3f dPhi %.3f" % r)
    assert max(r) <= 1.0


@pytest.mark.parametrize("case", ALL_CASES, ids=cid)
def test_marginal_form_against_the_dense_reference(ctx, case):
    n, M, l = case
    (x, y, _, _), ref, rec = lr.marginal_reference(case)
    b = lr.bounds(rec)
    out3, g, info = ctx.lowrank_logml_grad(x, y, M, SC, AMP, l, SIG)
    r = lr.worst_ratio(out3, ref["out3"], b["out3"]), lr.worst_ratio(g, ref["grad"], b["grad"])
    print(case, "out3 %.3f grad %.3f" % r)
    assert info == 0 and max(r) <= 1.0


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f[1])
@pytest.mark.parametrize("case", ALL_CASES, ids=cid)
def test_latent_form_against_the_reference(ctx, case, fam):
    n, M, l = case
    x, _, z, _ = lr.case_inputs(*case)
    Y = _Y(case, fam[0])
    ref, b = lr.latent_bounds(x, M, SC, AMP, l, z, fam[0], Y, SIG)
    got = ctx.lowrank_latent_lp_grad(x, M, SC, AMP, l, z, fam[1], Y, SIG, want_q=True, want_qbar=True)
    got["out"] = np.array([got["lik"], got["dlik_dsigma"]])
    r = {k: lr.worst_ratio(got[k], ref[k], b[k]) for k in b}
    print(case, fam[1], " ".join("%s %.3f" % kv for kv in r.items()))
    assert max(r.values()) <= 1.0, r
    # q and zbar against the library's own basis: two float64 evaluations, twice the bound
    P = ctx.hermite_basis(x, M, SC, AMP, l)
    assert lr.worst_ratio(got["q"], P @ z, 2 * b["q"]) <= 1.0
    assert lr.worst_ratio(got["zbar"], P.T @ got["qbar"], 2 * b["zbar"]) <= 1.0


# ---- layout: leading dimensions, padding, NULL outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(21, 17, 0.3), (257, 3, 0.3), (1, 2, 0.3)], ids=cid)
def test_basis_leading_dimensions_padding_and_null(ctx, case):
    n, M, l = case
    x = np.ascontiguousarray(lr.case_inputs(*case)[0])
    P0, D0 = ctx.hermite_basis(x, M, SC, AMP, l, want_dl=True)
    ldp, ldd = n + 3, n + 5
    P = np.full((ldp, M), SENT, order="F")
    D = np.full((ldd, M), SENT, order="F")
    assert ctx._lib.gpmi_hermite_basis(ctx._h, _p(x), n, M, _d(SC), _d(AMP), _d(l), _p(P), ldp, _p(D), ldd) == 0
    assert _same_bits(P[:n], P0) and _same_bits(D[:n], D0)
    assert np.all(P[n:] == SENT) and np.all(D[n:] == SENT)
    P2 = np.full((ldp, M), SENT, order="F")
    assert ctx._lib.gpmi_hermite_basis(ctx._h, _p(x), n, M, _d(SC), _d(AMP), _d(l), _p(P2), ldp, None, 0) == 0
    assert _same_bits(P2, P)


@pytest.mark.parametrize("case", [(65, 17, 0.3), (1438, 10, 1.0)], ids=cid)
def test_null_outputs_leave_the_neighbours_bits(ctx, case):
    n, M, l = case
    x, y, z, Y = lr.case_inputs(*case)
    out3, g, _ = ctx.lowrank_logml_grad(x, y, M, SC, AMP, l, SIG)
    out3b, gb, _ = ctx.lowrank_logml_grad(x, y, M, SC, AMP, l, SIG, want_grad=False)
    assert gb is None and _same_bits(out3, out3b)
    full = ctx.lowrank_latent_lp_grad(x, M, SC, AMP, l, z, "normal", Y, SIG, want_q=True, want_qbar=True)
    for wq, wb in ((False, True), (True, False), (False, False)):
        part = ctx.lowrank_latent_lp_grad(x, M, SC, AMP, l, z, "normal", Y, SIG, want_q=wq, want_qbar=wb)
        for k in ("lik", "dlik_dsigma", "zbar", "grad") + (("q",) if wq else ()) + (("qbar",) if wb else ()):
            assert _same_bits(part[k], full[k]), (k, wq, wb)
        assert (part["q"] is None) == (not wq) and (part["qbar"] is None) == (not wb)
    # Y with a leading dimension above n
    Yp = np.full((n + 4, 2), 0.5, order="F")
    Yp[:n] = Y
    out = np.empty(2); zb = np.empty(M); gr = np.empty(2); q = np.full(n + 2, SENT)
    zc = np.ascontiguousarray(z); xc = np.ascontiguousarray(x)
    assert ctx._lib.gpmi_lowrank_latent_lp_grad(ctx._h, _p(xc), n, M, _d(SC), _d(AMP), _d(l), _p(zc), 0, _p(Yp), 2, n + 4, _d(SIG), _p(out),
                                                _p(q), None, _p(zb), _p(gr)) == 0
    assert _same_bits(out, [full["lik"], full["dlik_dsigma"]]) and _same_bits(zb, full["zbar"]) and _same_bits(gr, full["grad"])
    assert _same_bits(q[:n], full["q"]) and np.all(q[n:] == SENT)


# ---- the two forms, repeated calls, workspace history --------------------------------------------------------------------------
def _dev_all(ctx, case, fam, ldpad=3):
    """Every _dev entry point on one case; returns host copies, with the padding rows of the matrices."""
    torch, dev = _torch()
    n, M, l = case
    x, y, z, _ = lr.case_inputs(*case)
    Y = _Y(case, fam[0])
    m = Y.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    ld = n + ldpad
    Yp = np.full((ld, m), 0.5)
    Yp[:n] = Y
    dx, dy, dz, dY = up(x), up(y), up(z), up(Yp.T.copy())   # dY: m columns of ld rows, column-major
    mk = lambda *shape: torch.full(shape, SENT, dtype=torch.float64, device=dev)
    dP, dD = mk(M, ld), mk(M, ld)
    o3, g3, o2, g2, q, qb, zb = mk(3), mk(3), mk(2), mk(2), mk(ld), mk(ld), mk(M)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.hermite_basis_dev(dx.data_ptr(), n, M, SC, AMP, l, dP.data_ptr(), ld, dD.data_ptr(), ld)
    ctx.lowrank_logml_grad_dev(dx.data_ptr(), n, dy.data_ptr(), M, SC, AMP, l, SIG, o3.data_ptr(), g3.data_ptr(), info.data_ptr())
    ctx.lowrank_latent_lp_grad_dev(dx.data_ptr(), n, M, SC, AMP, l, dz.data_ptr(), fam[1], dY.data_ptr(), m, ld, SIG, o2.data_ptr(),
                                   q.data_ptr(), qb.data_ptr(), zb.data_ptr(), g2.data_ptr())
    ctx.sync()
    h = lambda t: t.cpu().numpy()
    return {"Phi": h(dP).T, "dPhi": h(dD).T, "out3": h(o3), "grad3": h(g3), "info": int(info.cpu()[0]), "out": h(o2), "grad": h(g2),
            "q": h(q), "qbar": h(qb), "zbar": h(zb)}


def _host_all(ctx, case, fam):
    n, M, l = case
    x, y, z, _ = lr.case_inputs(*case)
    Y = _Y(case, fam[0])
    P, D = ctx.hermite_basis(x, M, SC, AMP, l, want_dl=True)
    out3, g3, info = ctx.lowrank_logml_grad(x, y, M, SC, AMP, l, SIG)
    r = ctx.lowrank_latent_lp_grad(x, M, SC, AMP, l, z, fam[1], Y, SIG, want_q=True, want_qbar=True)
    return {"Phi": P, "dPhi": D, "out3": out3, "grad3": g3, "info": info, "out": np.array([r["lik"], r["dlik_dsigma"]]), "grad": r["grad"],
            "q": r["q"], "qbar": r["qbar"], "zbar": r["zbar"]}


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f[1])
@pytest.mark.parametrize("case", [(3, 3, 0.3), (65, 128, 0.1), (257, 40, 0.3), (1438, 10, 1.0)], ids=cid)
def test_dev_forms_have_the_bits_of_the_host_forms(ctx, case, fam):
    n = case[0]
    hst, dv = _host_all(ctx, case, fam), _dev_all(ctx, case, fam)
    assert dv["info"] == 0 and hst["info"] == 0
    for k in ("out3", "grad3", "out", "grad", "zbar"):
        assert _same_bits(hst[k], dv[k]), k
    for k in ("Phi", "dPhi", "q", "qbar"):
        assert _same_bits(hst[k], dv[k][:n]), k
        assert np.all(dv[k][n:] == SENT), k   # rows >= n of every output keep the sentinel


@pytest.mark.parametrize("case", [(65, 128, 0.1), (1438, 10, 1.0), (2049, 3, 0.3)], ids=cid)
def test_repeated_calls_and_workspace_history_change_no_bit(ctx, case):
    fam = FAMILIES[1]
    first = _host_all(ctx, case, fam)
    runs = [_host_all(ctx, case, fam)]
    for byte in (0xFF, 0x7F):
        ctx.debug_fill(byte)
        runs.append(_host_all(ctx, case, fam))
        ctx.debug_fill(byte)
        runs.append(_dev_all(ctx, case, fam, ldpad=0))
    for r in runs:
        for k in first:
            assert _same_bits(first[k], r[k]) if k != "info" else first[k] == r[k], k


# ---- the models' own checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,M", lr.CONVERGED)
def test_converged_basis_reproduces_se_cov(ctx, l, M):
    """westbrook.stan:72: max |cov_exp_quad(x, amp, l) - L L'|, here against gpmi_se_cov on the same x.  Per entry: the truncation
    bound, the basis bounds carried through the product, the product's own rounding, and the kernel's rounding (a few eps plus
    the relative error eps |argument| of its exponential)."""
    x = np.linspace(-0.5, 0.5, 41)
    Pr, Dr = lr.basis_ld(x, M, SC, AMP, l)
    bP, _ = lr.basis_bounds(Pr, Dr, l)
    aP = np.abs(np.asarray(Pr, float))
    P = ctx.hermite_basis(x, M, SC, AMP, l)
    K = ctx.se_cov(x[:, None], None, AMP, [l])
    arg = (x[:, None] - x[None, :]) ** 2 / (2 * l * l)
    bound = (lr.truncation_bound(M, SC, AMP, l, 0.5) + bP @ aP.T + aP @ bP.T + lr.BOUND_C * lr.EPS * (aP @ aP.T)
             + (4 + arg) * lr.EPS * np.abs(K))
    err = np.abs(P @ P.T - K)
    print(l, M, "max |K - Phi Phi'| %.3g, worst ratio %.3f" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("l,M", [(0.3, 40), (1.0, 20)])
def test_converged_marginal_form_matches_the_exact_logml_grad(ctx, l, M):
    """out3 and grad entry by entry against gpmi_logml_grad (D = 1, jitter 0): the long-double difference of the two MODELS at this
    M (both by n x n factorisations on the CPU) plus the two device bounds."""
    n = 64
    x, y, _, _ = lr.case_inputs(n, M, l)
    X = x[:, None]
    lo_ref = lr.marginal_dense(x, y, M, SC, AMP, l, SIG)
    ex_ref = lg.logml_grad_reference(X, y, AMP, [l], SIG, 0.0, dtype=LD)
    cond = lg.cond2(X, AMP, [l], SIG, 0.0)
    bs, bq, bg = lg.bounds(ex_ref, cond, n)
    ex_b3 = np.array([lg.value_bound(ex_ref, cond, n), bs, bq * abs(float(ex_ref["out3"][2]))])
    lo_b = lr.bounds(lr.marginal_identity(x, y, M, SC, AMP, l, SIG))
    tr3 = np.abs(lo_ref["out3"] - ex_ref["out3"]).astype(float)
    trg = np.abs(lo_ref["grad"] - ex_ref["grad"]).astype(float)
    out3, g, info = ctx.lowrank_logml_grad(x, y, M, SC, AMP, l, SIG)
    eo, eg = ctx.logml_grad(X, y, AMP, [l], SIG, 0.0)
    print(l, M, "truncation", tr3, trg, "difference", np.abs(out3 - eo), np.abs(g - eg))
    assert info == 0
    assert np.all(np.abs(out3 - eo) <= tr3 + lo_b["out3"] + ex_b3)
    assert np.all(np.abs(g - eg) <= trg + lo_b["grad"] + bg)


def _westbrook():
    d = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "westbrook.json")))
    x = np.asarray(d["x"], float)
    return x, np.asarray(d["made"], float)


def test_westbrook_fixture_bernoulli_head(ctx):
    x, y = _westbrook()
    M, l, amp = 10, 0.4, 1.1
    assert x.size == 1438 and set(np.unique(y)) <= {0.0, 1.0}
    z = np.random.default_rng(7).standard_normal(M)
    z[0] *= 0.01
    ref, b = lr.latent_bounds(x, M, SC, amp, l, z, lr.BERNOULLI, y[:, None], SIG)
    got = ctx.lowrank_latent_lp_grad(x, M, SC, amp, l, z, "bernoulli_logit", y, None, want_q=True, want_qbar=True)
    got["out"] = np.array([got["lik"], got["dlik_dsigma"]])
    r = {k: lr.worst_ratio(got[k], ref[k], b[k]) for k in b}
    print(" ".join("%s %.3f" % kv for kv in r.items()))
    assert max(r.values()) <= 1.0, r


def test_westbrook_log_prob_grad_is_the_difference_quotient_of_its_value(ctx):
    """westbrook_log_prob_grad against central differences of lp__ itself, evaluated on the CPU in long double (the recurrence in
    long double, which test_lowrank_reference.py ties to the closed form; priors and Jacobians of models/westbrook.stan:56-61).
    Tolerance, reasoned: a central difference with step h has truncation error ~ h^2 |lp'''| / 6 and rounding error
    ~ eps_ld |lp| / h; at h = 2^-21 and |lp| ~ 1e3 (1438 Bernoulli terms), |lp'''| <~ 1e4 (z_1's prior alone contributes none: it
    is quadratic) these are 4e-10 and 2e-10: 1e-8 absolute plus 1e-9 relative leaves a factor ten."""
    from gp_amd import stan_models
    x, y = _westbrook()
    M, l, amp = 10, 0.4, 1.1
    z = np.random.default_rng(7).standard_normal(M)
    z[0] *= 0.01
    lp, grad = stan_models.westbrook_log_prob_grad(x, y, z, amp, l, M, SC, ctx=ctx)

    def value(th):
        zz, a, ll = th[:M], th[M], th[M + 1]
        P, _ = lr.basis_f64(x, M, SC, a, ll, dtype=LD)
        q = P @ zz
        lik = np.sum(y.astype(LD) * q - (np.maximum(q, 0) + np.log1p(np.exp(-np.abs(q)))))
        w = np.ones(M, LD)
        w[0] = LD(1) / (LD("0.01") * LD("0.01"))
        return 3 * np.log(ll) - 4 * ll - zz @ (w * zz) / 2 - a * a / 2 + lik + np.log(a) + np.log(ll)

    th = np.concatenate([z, [amp, l]]).astype(LD)
    assert abs(float(value(th) - LD(lp))) <= 1e-9 * abs(lp)
    h = LD(2.0) ** -21
    for k in range(M + 2):
        tp, tm = th.copy(), th.copy()
        tp[k] += h
        tm[k] -= h
        fd = float((value(tp) - value(tm)) / (2 * h))
        assert abs(fd - grad[k]) <= 1e-8 + 1e-9 * abs(fd), (k, fd, grad[k])


def test_fit_approx_gp_log_prob_grad_is_the_difference_quotient_of_its_value(ctx):
    """fit_approx_gp_log_prob_grad (the NORMAL head, scale 1) the same way on a small input; |lp| ~ 1e2 here."""
    from gp_amd import stan_models
    n, M, l, alpha, sigma = 65, 17, 0.3, 0.9, 0.4
    x, y, zm, _ = lr.case_inputs(n, M, l)
    x = 3.0 * x
    lp, grad = stan_models.fit_approx_gp_log_prob_grad(x, y, l, alpha, sigma, zm, M, 1.0, ctx=ctx)

    def value(th):
        ll, a, s, zz = th[0], th[1], th[2], th[3:]
        P, _ = lr.basis_f64(x, M, 1.0, a, ll, dtype=LD)
        r = y.astype(LD) - P @ zz
        return 3 * np.log(ll) - 4 * ll - a * a / 2 - zz @ zz / 2 - n * np.log(s) - r @ r / (2 * s * s) + np.log(ll) + np.log(a) + np.log(s)

    th = np.concatenate([[l, alpha, sigma], zm]).astype(LD)
    assert abs(float(value(th) - LD(lp))) <= 1e-9 * abs(lp)
    h = LD(2.0) ** -21
    for k in range(M + 3):
        tp, tm = th.copy(), th.copy()
        tp[k] += h
        tm[k] -= h
        fd = float((value(tp) - value(tm)) / (2 * h))
        assert abs(fd - grad[k]) <= 1e-8 + 1e-9 * abs(fd), (k, fd, grad[k])


# ---- status and argument errors -------------------------------------------------------------------------------------------------
def test_not_positive_definite_status(ctx):
    """n = 1, x = [0], M = 2, sigma = 1e-170: the second column is exactly zero at x = 0 and sigma^2 underflows, so the second pivot
    is exactly 0: status 2, every output NaN, d_info = 2 on the _dev form."""
    import gp_amd
    x, y = np.zeros(1), np.ones(1)
    out3, g, info = ctx.lowrank_logml_grad(x, y, 2, SC, AMP, 0.3, 1e-170, raise_not_pd=False)
    assert info == 2 and np.all(np.isnan(out3)) and np.all(np.isnan(g))
    with pytest.raises(gp_amd.NotPositiveDefinite) as e:
        ctx.lowrank_logml_grad(x, y, 2, SC, AMP, 0.3, 1e-170)
    assert e.value.order == 2
    torch, dev = _torch()
    dx = torch.zeros(1, dtype=torch.float64, device=dev)
    dy = torch.ones(1, dtype=torch.float64, device=dev)
    o = torch.full((6,), SENT, dtype=torch.float64, device=dev)
    di = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ctx.lowrank_logml_grad_dev(dx.data_ptr(), 1, dy.data_ptr(), 2, SC, AMP, 0.3, 1e-170, o.data_ptr(), o.data_ptr() + 24, di.data_ptr())
    ctx.sync()
    assert int(di.cpu()[0]) == 2 and bool(torch.isnan(o).all().cpu())


BAD_COMMON = [dict(n=0), dict(M=0), dict(M=129), dict(scale=0.0), dict(scale=np.inf), dict(amp=-1.0), dict(amp=np.nan), dict(l=0.0),
              dict(l=np.inf), dict(x=None)]


def _earg(ctx, rc):
    assert rc == -1, rc
    assert ctx._lib.gpmi_last_error()


def test_every_argument_error_returns_earg_and_writes_nothing(ctx):
    n, M, l = 21, 10, 1.0
    x, y, z, Y = lr.case_inputs(n, M, l)
    x, y, z = (np.ascontiguousarray(v) for v in (x, y, z))
    Yf = np.asfortranarray(Y)
    L = ctx._lib
    torch, dev = _torch()
    dbuf = torch.full((4096,), SENT, dtype=torch.float64, device=dev)
    dY01 = torch.zeros(64, dtype=torch.float64, device=dev)
    dinfo = torch.full((1,), -7, dtype=torch.int32, device=dev)
    DP = dbuf.data_ptr()

    def basis(dev_form=False, **kw):
        a = dict(x=x, n=n, M=M, scale=SC, amp=AMP, l=l, ldp=n, lddp=n, Phi=True, dPhi=True)
        a.update(kw)
        if dev_form:
            return L.gpmi_hermite_basis_dev(ctx._h, C.c_void_p(DP) if a["x"] is not None else None, a["n"], a["M"], _d(a["scale"]), _d(a["amp"]),
                                            _d(a["l"]), C.c_void_p(DP + 8 * 64) if a["Phi"] else None, a["ldp"],
                                            C.c_void_p(DP + 8 * 2048) if a["dPhi"] else None, a["lddp"])
        return L.gpmi_hermite_basis(ctx._h, _p(a["x"]), a["n"], a["M"], _d(a["scale"]), _d(a["amp"]), _d(a["l"]), _p(hP) if a["Phi"] else None,
                                    a["ldp"], _p(hD) if a["dPhi"] else None, a["lddp"])

    def logml(dev_form=False, **kw):
        a = dict(x=x, y=y, n=n, M=M, scale=SC, amp=AMP, l=l, sigma=SIG, out3=True, info=True)
        a.update(kw)
        if dev_form:
            return L.gpmi_lowrank_logml_grad_dev(ctx._h, C.c_void_p(DP) if a["x"] is not None else None, a["n"],
                                                 C.c_void_p(DP) if a["y"] is not None else None, a["M"], _d(a["scale"]), _d(a["amp"]), _d(a["l"]),
                                                 _d(a["sigma"]), C.c_void_p(DP + 8 * 64) if a["out3"] else None, C.c_void_p(DP + 8 * 72),
                                                 C.c_void_p(dinfo.data_ptr()) if a["info"] else None)
        return L.gpmi_lowrank_logml_grad(ctx._h, _p(a["x"]), a["n"], _p(a["y"]), a["M"], _d(a["scale"]), _d(a["amp"]), _d(a["l"]), _d(a["sigma"]),
                                         _p(h3) if a["out3"] else None, _p(hg))

    def latent(dev_form=False, **kw):
        a = dict(x=x, z=z, Y=Yf, n=n, M=M, scale=SC, amp=AMP, l=l, sigma=SIG, family=0, m=2, ldy=n, out=True, zbar=True, grad=True)
        a.update(kw)
        if dev_form:
            dp = lambda key, off: C.c_void_p(DP + 8 * off) if (a[key] is not None and a[key] is not False) else None
            return L.gpmi_lowrank_latent_lp_grad_dev(ctx._h, dp("x", 0), a["n"], a["M"], _d(a["scale"]), _d(a["amp"]), _d(a["l"]), dp("z", 0),
                                                     a["family"], C.c_void_p(dY01.data_ptr()) if a["Y"] is not None else None, a["m"], a["ldy"],
                                                     _d(a["sigma"]), dp("out", 64), C.c_void_p(DP + 8 * 128), C.c_void_p(DP + 8 * 256),
                                                     dp("zbar", 512), dp("grad", 72))
        return L.gpmi_lowrank_latent_lp_grad(ctx._h, _p(a["x"]), a["n"], a["M"], _d(a["scale"]), _d(a["amp"]), _d(a["l"]), _p(a["z"]), a["family"],
                                             _p(a["Y"]), a["m"], a["ldy"], _d(a["sigma"]), _p(h2) if a["out"] else None, _p(hq), _p(hqb),
                                             _p(hzb) if a["zbar"] else None, _p(hg2) if a["grad"] else None)

    hP = np.full((n, M), SENT, order="F"); hD = np.full((n, M), SENT, order="F")
    h3 = np.full(3, SENT); hg = np.full(3, SENT); h2 = np.full(2, SENT); hg2 = np.full(2, SENT)
    hq = np.full(n, SENT); hqb = np.full(n, SENT); hzb = np.full(M, SENT)
    bad_sigma = [dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.inf), dict(sigma=np.nan)]
    Ybad = Yf.copy()
    Ybad[3, 0] = 0.5
    table = (
        (basis, BAD_COMMON + [dict(ldp=n - 1), dict(lddp=n - 1), dict(Phi=False)]),
        (logml, BAD_COMMON + bad_sigma + [dict(y=None), dict(out3=False)]),
        (latent, BAD_COMMON + bad_sigma + [dict(m=0), dict(ldy=n - 1), dict(family=2), dict(family=3), dict(family=7), dict(z=None), dict(Y=None),
                                           dict(out=False), dict(zbar=False), dict(grad=False)]),
    )
    for fn, bads in table:
        for dev_form in (False, True):
            assert fn(dev_form) == 0   # the baseline call is valid
            ctx.sync()
            dbuf.fill_(SENT)
            for arr in (hP, hD, h3, hg, h2, hg2, hq, hqb, hzb):
                arr.fill(SENT)
            torch.cuda.synchronize()
            for kw in bads + ([dict(info=False)] if (fn is logml and dev_form) else []):
                _earg(ctx, fn(dev_form, **kw))
            ctx.sync()
            assert bool((dbuf == SENT).all().cpu()), (fn.__name__, dev_form)
            for arr in (hP, hD, h3, hg, h2, hg2, hq, hqb, hzb):
                assert np.all(arr == SENT), (fn.__name__, dev_form)
    # the host-buffer form alone can look at Y: outcomes other than 0 or 1 under the Bernoulli head
    _earg(ctx, latent(False, family=1, Y=Ybad))
    assert latent(False, family=1) == 0
