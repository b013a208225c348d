"""GPU: reverse mode of the interpolated latent-GP models of test_interpolate.R -- the cubic Hermite model
(gpmi_approx_Lz_vjp, models/cubic_interpolated_gp.hpp:6-32,38-73) and the GP-regression model (gpmi_interp_gp_*,
models/interpolated_gp.stan:9-47): F = A(l) Z, Zbar = A(l)^T Fbar, lbar = sum(Fbar o (dA/dl) Z)."""
import math

import numpy as np
import pytest

import interp_vjp_reference as ref

pytestmark = pytest.mark.gpu


def _qgamma44(p):
    # quantile of gamma(shape 4, rate 4): the Erlang CDF 1 - exp(-4x) sum_{k<4} (4x)^k / k!, by bisection
    cdf = lambda x: 1.0 - math.exp(-4 * x) * sum((4 * x) ** k / math.factorial(k) for k in range(4))
    lo, hi = 0.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


def _reference_grid():
    # lp = seq(qgamma(0.05, 4, 4), qgamma(0.95, 4, 4), length = 10), test_interpolate.R:9
    return np.linspace(_qgamma44(0.05), _qgamma44(0.95), 10)


@pytest.fixture(scope="module")
def ref_table(orc):
    x = np.linspace(0.0, 10.0, 100)
    lp = _reference_grid()
    Ls, dLs = zip(*[orc.rbf_cov_chol(x, l) for l in lp])
    return x, lp, list(Ls), list(dLs)


def _check_hermite(ctx, l, Z, Fb):
    F, Zb, lb = ctx.approx_Lz_vjp(l, Z, Fb)
    A = ctx.approx_L(l)
    k = Z.shape[1]
    G = np.empty_like(F)
    for c in range(k):
        assert np.array_equal(F[:, c], ctx.approx_Lz(l, Z[:, c])), (l, k, c)     # bit for bit
        G[:, c] = ctx.approx_Lz_grad(l, Z[:, c])[1]
    bound = 1e-13 * (np.abs(A).T @ np.abs(Fb)) + 1e-300
    assert np.all(np.abs(Zb - A.T @ Fb) <= bound), (l, k)
    assert abs(lb - float(np.sum(Fb * G))) <= 1e-14 * float(np.sum(np.abs(Fb * G))), (l, k)
    return F, Zb, lb


def test_hermite_vjp_on_the_reference_grid(ctx, ref_table):
    x, lp, Ls, dLs = ref_table
    ctx.interp_load(lp, Ls, dLs)
    rng = np.random.default_rng(1)
    n = x.size
    ls = (lp[0], 0.5 * (lp[0] + lp[1]), lp[3] + 0.3 * (lp[4] - lp[3]), lp[5], lp[8] + 0.9 * (lp[9] - lp[8]), lp[9], 0.2, 2.5)
    for k in (1, 3, 9):
        Z = rng.standard_normal((n, k)); Fb = rng.standard_normal((n, k))
        for l in ls:
            _check_hermite(ctx, l, Z, Fb)
    # lbar against central differences of Fbar^T approx_Lz(l) Z inside an interval
    Z = rng.standard_normal(n); Fb = rng.standard_normal(n)
    l = lp[6] + 0.4 * (lp[7] - lp[6]); h = 1e-6
    _, _, lb = ctx.approx_Lz_vjp(l, Z, Fb)
    fd = (Fb @ ctx.approx_Lz(l + h, Z) - Fb @ ctx.approx_Lz(l - h, Z)) / (2 * h)
    assert abs(lb - fd) <= 1e-7 * abs(fd)
    ctx.interp_free()


@pytest.mark.parametrize("n,ks", [(1111, (1, 9)), (4096, (1, 3))])
def test_hermite_vjp_random_tables(ctx, n, ks):
    """row blocks, ragged chunk edges and the multi-workgroup path on random lower-triangular tables (P = 2)"""
    rng = np.random.default_rng(n)
    lp = np.array([1.0, 2.0])
    Ls = [np.tril(rng.standard_normal((n, n))) for _ in lp]
    dLs = [np.tril(rng.standard_normal((n, n))) for _ in lp]
    ctx.interp_load(lp, Ls, dLs)
    del Ls, dLs
    for k in ks:
        Z = rng.standard_normal((n, k)); Fb = rng.standard_normal((n, k))
        for l in (1.3, 2.4):
            F, Zb, lb = _check_hermite(ctx, l, Z, Fb)
            F2, Zb2, lb2 = ctx.approx_Lz_vjp(l, Z, Fb)
            assert np.array_equal(F, F2) and np.array_equal(Zb, Zb2) and lb == lb2   # repeated calls: the same bits
    ctx.interp_free()


def _gp_setup_well_conditioned(orc):
    x = np.linspace(0.0, 8.0, 12)
    lp = np.array([0.5, 1.5, 2.5, 3.5])    # knots 1.0 apart: cond(Sigma_P) ~ 16
    exact = [orc.rbf_cov_chol(x, l)[0] for l in lp]
    return x, lp, exact


def test_gp_table_well_conditioned(ctx, orc):
    x, lp, exact = _gp_setup_well_conditioned(orc)
    n = x.size
    ctx.interp_gp_load(lp, exact)
    M = ref.gp_lookup(lp, exact)
    for l in (0.5, 0.9, 1.7, 2.5, 3.1, 3.5):
        got = ctx.interp_gp_L(l)
        assert np.max(np.abs(got - ref.gp_L(l, lp, M))) <= 1e-12, l
        assert np.all(np.triu(got, 1) == 0.0)
    for p, l in enumerate(lp):   # at a knot: that knot's factor, up to the jitter's ~2e-10
        assert np.max(np.abs(ctx.interp_gp_L(l) - exact[p])) <= 1e-9, p
    # the table built on the device from x equals the one loaded from the device's own factors, and the oracle's closely
    loaded_dev = [ctx.rbf_cov_chol(x, l)[0] for l in lp]
    ctx.interp_gp_load(lp, loaded_dev)
    Lload = [ctx.interp_gp_L(l) for l in (0.8, 2.2)]
    ctx.interp_gp_build(x, lp)
    for L0, l in zip(Lload, (0.8, 2.2)):
        Lb = ctx.interp_gp_L(l)
        assert np.max(np.abs(Lb - L0)) <= 1e-12, l
        assert np.max(np.abs(Lb - ref.gp_L(l, lp, M))) <= 1e-8, l
    # F of _Lz and of _Lz_vjp bit for bit; Zbar against the device's own L(l); lbar against central differences
    rng = np.random.default_rng(7)
    for k in (1, 3, 9):
        Z = rng.standard_normal((n, k)); Fb = rng.standard_normal((n, k))
        for l in (0.7, 1.9, 3.3):
            F, Zb, lb = ctx.interp_gp_Lz_vjp(l, Z, Fb)
            assert np.array_equal(F, ctx.interp_gp_Lz(l, Z)), (l, k)
            L = ctx.interp_gp_L(l)
            assert np.all(np.abs(Zb - L.T @ Fb) <= 1e-13 * (np.abs(L).T @ np.abs(Fb)) + 1e-300), (l, k)
            h = 1e-6
            fd = (np.sum(Fb * ctx.interp_gp_Lz(l + h, Z)) - np.sum(Fb * ctx.interp_gp_Lz(l - h, Z))) / (2 * h)
            assert abs(lb - fd) <= 1e-7 * max(abs(fd), 1e-3), (l, k, lb, fd)
            wd = ref.gp_weights(l, lp)[1]
            dL = sum(w * Mp for w, Mp in zip(wd, M))
            assert abs(lb - float(np.sum(Fb * (dL @ Z)))) <= 1e-8 * float(np.sum(np.abs(Fb) * (np.abs(dL) @ np.abs(Z))))
    ctx.interp_gp_free()


def test_gp_table_reference_configuration(ctx, ref_table):
    """x = linspace(0, 10, 100), P = 10 knots of test_interpolate.R:9, rho = 1, jitter 1e-10: cond(Sigma_P) ~ 8e10 and
    max|lookup| ~ 2e8 against max|L| = 1, so two float64 orderings of the same formula (the device's LU substitutions and
    numpy's LAPACK solve) differ by ~6e-8 in L(l): the comparison bound is 1e-6 absolute."""
    x, lp, Ls, _ = ref_table
    ctx.interp_gp_load(lp, Ls)
    M = ref.gp_lookup(lp, Ls)
    for l in (lp[0], 0.5 * (lp[2] + lp[3]), lp[5], 1.37, lp[9]):
        assert np.max(np.abs(ctx.interp_gp_L(l) - ref.gp_L(l, lp, M))) <= 1e-6, l
    ctx.interp_gp_free()


def _dev_vs_host(ctx, fn_host, fn_dev, n, k, l, rng):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    Z = rng.standard_normal((n, k)); Fb = rng.standard_normal((n, k))
    F, Zb, lb = fn_host(l, Z, Fb)
    dZ = torch.from_numpy(np.ascontiguousarray(Z.T)).to(dev)     # (k, n) row-major == n x k column-major
    dFb = torch.from_numpy(np.ascontiguousarray(Fb.T)).to(dev)
    dF = torch.zeros((k, n), dtype=torch.float64, device=dev); dZb = torch.zeros_like(dF)
    dl = torch.zeros(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    fn_dev(l, dZ.data_ptr(), k, n, dFb.data_ptr(), n, dF.data_ptr(), n, dZb.data_ptr(), n, dl.data_ptr())
    ctx.sync()
    assert np.array_equal(dF.cpu().numpy().T, F) and np.array_equal(dZb.cpu().numpy().T, Zb) and float(dl.cpu()[0]) == lb
    # F = NULL: Zbar and lbar unchanged
    dZb2 = torch.zeros_like(dF); dl2 = torch.zeros_like(dl)
    fn_dev(l, dZ.data_ptr(), k, n, dFb.data_ptr(), n, None, n, dZb2.data_ptr(), n, dl2.data_ptr())
    ctx.sync()
    assert torch.equal(dZb2, dZb) and torch.equal(dl2, dl)
    _, Zb3, lb3 = fn_host(l, Z, Fb, False)
    assert np.array_equal(Zb3, Zb) and lb3 == lb


def test_both_models_dev_calls_null_F_and_coexisting_tables(ctx, orc, ref_table):
    x, lp, Ls, dLs = ref_table
    n = x.size
    rng = np.random.default_rng(11)
    ctx.interp_load(lp, Ls, dLs)
    z = rng.standard_normal(n)
    before = [ctx.approx_Lz(l, z) for l in (0.6, 1.1)]
    before_g = [ctx.approx_Lz_grad(l, z) for l in (0.6, 1.1)]
    ctx.interp_gp_load(lp, Ls)                      # the GP table does not touch the Hermite table ...
    gp_before = ctx.interp_gp_L(1.1)
    for l, f0, (f1, g1) in zip((0.6, 1.1), before, before_g):
        assert np.array_equal(ctx.approx_Lz(l, z), f0)
        f2, g2 = ctx.approx_Lz_grad(l, z)
        assert np.array_equal(f2, f1) and np.array_equal(g2, g1)
    ctx.interp_load(lp, Ls, dLs)                    # ... nor the Hermite table the GP table
    assert np.array_equal(ctx.interp_gp_L(1.1), gp_before)
    for k in (1, 3, 9):
        _dev_vs_host(ctx, ctx.approx_Lz_vjp, ctx.approx_Lz_vjp_dev, n, k, 0.93, rng)
        _dev_vs_host(ctx, ctx.interp_gp_Lz_vjp, ctx.interp_gp_Lz_vjp_dev, n, k, 0.93, rng)
    # the multi-workgroup path
    xb = np.linspace(0.0, 60.0, 600)
    ctx.interp_gp_load([0.5, 1.5, 2.5], [orc.rbf_cov_chol(xb, l)[0] for l in (0.5, 1.5, 2.5)])
    _dev_vs_host(ctx, ctx.interp_gp_Lz_vjp, ctx.interp_gp_Lz_vjp_dev, 600, 2, 1.2, rng)
    ctx.interp_gp_free()
    ctx.interp_free()


def test_errors(ctx, ref_table):
    import gp_amd
    x, lp, Ls, dLs = ref_table
    n = x.size
    z = np.ones(n)
    ctx.interp_free(); ctx.interp_gp_free()
    ctx._itp_n = n; ctx._igp_n = n
    with pytest.raises(gp_amd.GpmiError):
        ctx.approx_Lz_vjp(1.0, z, z)             # no table
    with pytest.raises(gp_amd.GpmiError):
        ctx.interp_gp_Lz_vjp(1.0, z, z)
    with pytest.raises(gp_amd.GpmiError):
        ctx.interp_gp_L(1.0)
    ctx.interp_load(lp, Ls, dLs)
    ctx.interp_gp_load(lp, Ls)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(gp_amd.GpmiError):
            ctx.approx_Lz_vjp(bad, z, z)
        with pytest.raises(gp_amd.GpmiError):
            ctx.interp_gp_Lz_vjp(bad, z, z)
    import ctypes as C
    lib = ctx._lib
    buf = np.zeros(4 * n)
    p = lambda off: C.c_void_p(buf.ctypes.data + 8 * off)
    for fn in (lib.gpmi_approx_Lz_vjp, lib.gpmi_interp_gp_Lz_vjp):
        assert fn(ctx._h, C.c_double(1.0), p(0), 0, n, p(n), n, p(2 * n), n, p(3 * n), n, p(0)) == -1   # GPMI_EARG
    with pytest.raises(gp_amd.GpmiError):     # P above 64
        ctx.interp_gp_load(np.linspace(0.5, 2.0, 65), [Ls[0]] * 65)
    with pytest.raises(gp_amd.GpmiError):     # singular Sigma_P: a repeated knot without jitter
        ctx.interp_gp_load([0.5, 0.5, 1.0], Ls[:3], jitter=0.0)
    ctx.interp_gp_free(); ctx.interp_free()


def test_log_prob_grads_by_central_differences(ctx, orc):
    from gp_amd.covariance import FactorInterpolator, GPFactorInterpolator
    from gp_amd.stan_models import cubic_interpolated_gp_log_prob_grad, interpolated_gp_log_prob_grad
    x = np.linspace(0.0, 8.0, 12)
    rng = np.random.default_rng(5)
    y = np.sin(x) + 0.2 * rng.standard_normal(12)
    z = rng.standard_normal(12)
    cases = [(FactorInterpolator(x, np.linspace(0.6, 1.1, 5), ctx=ctx), cubic_interpolated_gp_log_prob_grad, (0.71, 0.97)),
             (GPFactorInterpolator(x, [0.5, 1.5, 2.5, 3.5], ctx=ctx), interpolated_gp_log_prob_grad, (0.8, 2.1, 3.3))]
    h = 1e-6
    for interp, fn, ls in cases:
        for l in ls:
            lp0, g = fn(interp, y, l, 0.4, z)
            f = lambda l_, s_, z_: fn(interp, y, l_, s_, z_)[0]
            fd = [(f(l + h, 0.4, z) - f(l - h, 0.4, z)) / (2 * h), (f(l, 0.4 + h, z) - f(l, 0.4 - h, z)) / (2 * h)]
            for i in (0, 5, 11):
                e = np.zeros(12); e[i] = h
                fd.append((f(l, 0.4, z + e) - f(l, 0.4, z - e)) / (2 * h))
            got = np.concatenate([g[:2], g[2 + np.array([0, 5, 11])]])
            assert np.all(np.abs(got - np.array(fd)) <= 1e-5 * np.maximum(1.0, np.abs(fd))), (fn.__name__, l, got, fd)
        assert fn(interp, y, float(np.min(interp.lp)) - 0.01, 0.4, z)[0] == -math.inf
    ctx.interp_free(); ctx.interp_gp_free()
