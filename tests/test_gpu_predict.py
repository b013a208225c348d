"""GPU: gpmi_gp_predict / gpmi_gp_predict_dev (posterior mean and pointwise variance at new D-dimensional inputs) and
gpmi_seq_marginals (the sweep of R/tests.R:89-97 over a create_p_dotXnS sampler, R/ode_gp_library.R:43-93, in one call) against
the numpy yardstick tests/predict_reference.py, numpy's LAPACK at the full sizes, and the library's own older entry points.

Tolerances (predict_reference.MEAN_TOL / VAR_TOL, tied to the yardstick's own error by tests/test_predict_reference.py):
mean 1e-9 relative in the max norm, variance 1e-9 of alpha^2 absolute; gpmi_seq_marginals 1e-8 max(1, |.|), the bound
tests/test_gpu_seq.py holds the sampler itself to."""
import ctypes as C
import functools

import numpy as np
import pytest

import predict_reference as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def octx():
    """A context of this module's own for the runs that change options (the session context keeps its defaults)."""
    import gp_amd
    c = gp_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    for c in pr.parity_cases():
        if c[0] == name:
            _, n, D, m, alpha, ell, sigma, jitter = c
            X, y, Xs = pr.inputs(n, D, m)
            want = pr.predict(X, y, Xs, alpha, ell, sigma, jitter, float)
            return X, y, Xs, alpha, ell, sigma, jitter, want
    raise KeyError(name)


def _errors(got, want, alpha):
    em = pr.max_rel(got["mean"], want[0])
    ev = float(np.max(np.abs(got["var"] - want[1]))) / alpha ** 2
    return em, ev


def _ragged_chunk(m):
    """A chunk size that splits m rows into at least three chunks with a shorter last one."""
    mb = m // 3
    mb -= mb % 8
    if m % mb == 0:
        mb -= 1
    assert mb >= 1 and m % mb != 0 and (m + mb - 1) // mb >= 3
    return mb


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "chain", "chunks"])
@pytest.mark.parametrize("name", [c[0] for c in pr.parity_cases()])
def test_parity_with_the_reference(ctx, octx, name, mode):
    X, y, Xs, alpha, ell, sigma, jitter, want = _case(name)
    c = ctx
    if mode != "default":
        c = octx
        c.set_option("small_pr", 0)
        c.set_option("predict_mb", _ragged_chunk(Xs.shape[0]) if mode == "chunks" else 0)
    got = c.gp_predict(X, y, alpha, ell, sigma, jitter, Xs)
    em, ev = _errors(got, want, alpha)
    print("%s [%s]: mean %.2e var/alpha^2 %.2e" % (name, mode, em, ev))
    assert got["info"] == 0
    assert em <= pr.MEAN_TOL
    assert ev <= pr.VAR_TOL


# ---- 2. full size ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(8192, 1000), (16384, 257)])
def test_full_size_against_lapack(ctx, n, m):
    X, y, Xs = pr.inputs(n, 3, m)
    alpha, ell, sigma, jitter = 1.0, pr.ARD3, 0.1, 1e-6
    want = pr.predict_lapack(X, y, Xs, alpha, ell, sigma, jitter)
    got = ctx.gp_predict(X, y, alpha, ell, sigma, jitter, Xs)
    em, ev = _errors(got, want, alpha)
    print("n = %d m = %d: mean %.2e var/alpha^2 %.2e" % (n, m, em, ev))
    assert got["info"] == 0
    assert em <= pr.MEAN_TOL and ev <= pr.VAR_TOL


# ---- 3. mean-only path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,m", [(300, 3, 128), (4096, 3, 700), (500, 8, 333), (500, 17, 333)])
def test_mean_only_path(ctx, n, D, m):
    X, y, Xs = pr.inputs(n, D, m)
    ell = np.linspace(0.3, 0.8, D) * np.sqrt(D / 3.0)
    both = ctx.gp_predict(X, y, 1.0, ell, 0.1, 1e-6, Xs)
    only = ctx.gp_predict(X, y, 1.0, ell, 0.1, 1e-6, Xs, want_var=False)
    e = pr.max_rel(only["mean"], both["mean"])
    print("mean only n = %d D = %d: %.2e" % (n, D, e))
    assert only["info"] == 0 and only["var"] is None
    assert e <= pr.MEAN_TOL
    if n <= 500:
        want = pr.predict(X, y, Xs, 1.0, ell, 0.1, 1e-6)
        assert pr.max_rel(only["mean"], want[0]) <= pr.MEAN_TOL
    # the raw entry point leaves a var buffer it was not given alone: pass NULL and keep a sentinel beside the mean
    mean = np.full(m + 1, -7.0)
    rc = _raw(ctx, X, y, 1.0, ell, 0.1, 1e-6, Xs, mean=mean, var=None)
    assert rc == 0 and mean[m] == -7.0
    np.testing.assert_array_equal(mean[:m], only["mean"])


# ---- 4. determinism and entry points -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,want_var", [(21, 41, True), (700, 300, True), (700, 300, False)])
def test_repeated_calls_give_identical_bits(ctx, n, m, want_var):
    X, y, Xs = pr.inputs(n, 3, m)
    a = ctx.gp_predict(X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs, want_var=want_var)
    b = ctx.gp_predict(X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs, want_var=want_var)
    np.testing.assert_array_equal(a["mean"], b["mean"])
    if want_var:
        np.testing.assert_array_equal(a["var"], b["var"])


@pytest.mark.parametrize("n,m,want_var", [(21, 41, True), (700, 300, True), (700, 300, False)])
def test_dev_equals_host(ctx, n, m, want_var):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    X, y, Xs = pr.inputs(n, 3, m)
    host = ctx.gp_predict(X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs, want_var=want_var)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)      # (D, n) row-major == n x D column-major
    dXs = torch.from_numpy(np.ascontiguousarray(Xs.T)).to(dev)
    dy = torch.from_numpy(y).to(dev)
    dmean = torch.zeros(m, dtype=torch.float64, device=dev)
    dvar = torch.full((m,), -7.0, dtype=torch.float64, device=dev)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.gp_predict_dev(dX.data_ptr(), n, n, 3, dy.data_ptr(), 1.0, pr.ARD3, 0.1, 1e-6, dXs.data_ptr(), m, m, dmean.data_ptr(),
                       dvar.data_ptr() if want_var else None, info.data_ptr())
    ctx.sync()
    assert int(info.item()) == 0
    np.testing.assert_array_equal(dmean.cpu().numpy(), host["mean"])
    if want_var:
        np.testing.assert_array_equal(dvar.cpu().numpy(), host["var"])
    else:
        assert np.all(dvar.cpu().numpy() == -7.0)


# ---- 5. existing entry points as yardsticks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(100, 64), (500, 200)])
def test_agrees_with_gp_condition_1d(ctx, n, m):
    X, y, Xs = pr.inputs(n, 1, m)
    alpha, l, sigma, jp, jc = 1.2, 0.3, 0.1, 1e-6, 1e-8
    got = ctx.gp_predict(X, y, alpha, [l], sigma, jp, Xs)
    mn, Kn = ctx.gp_condition(X[:, 0], Xs[:, 0], y, alpha, l, sigma ** 2 + jp, jc, "QQ", "QQ", "QQ")
    em = pr.max_rel(got["mean"], mn)
    ev = float(np.max(np.abs(got["var"] - (np.diag(Kn) - jc)))) / alpha ** 2
    print("gp_condition n = %d: mean %.2e var/alpha^2 %.2e" % (n, em, ev))
    assert em <= pr.MEAN_TOL and ev <= pr.VAR_TOL


@pytest.mark.parametrize("n,want_var", [(150, True), (1000, True), (1000, False)])
def test_mean_at_the_data_is_y_minus_noise_times_a(ctx, n, want_var):
    X, y, _ = pr.inputs(n, 3, 1)
    alpha, ell, sigma, jitter = 1.0, pr.ARD3, 0.1, 1e-6
    S = pr.se_cov(X, X, alpha, ell)
    S[np.diag_indices(n)] += sigma ** 2 + jitter
    a = np.linalg.solve(S, y)
    got = ctx.gp_predict(X, y, alpha, ell, sigma, jitter, X, want_var=want_var)
    e = pr.max_rel(got["mean"], y - (sigma ** 2 + jitter) * a)
    print("mean at the data n = %d: %.2e" % (n, e))
    assert e <= pr.MEAN_TOL


# ---- 6. properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(60, 100), (2000, 1500)])
def test_variance_bounds_and_far_points(ctx, n, m):
    X, y, Xs = pr.inputs(n, 2, m)
    alpha, ell = 1.5, (0.2, 0.3)
    got = ctx.gp_predict(X, y, alpha, ell, 0.05, 1e-6, Xs)
    assert np.all(got["var"] <= alpha ** 2 * (1 + 1e-12))
    assert np.all(got["var"] >= -pr.VAR_TOL * alpha ** 2)
    far = Xs + 50.0 * np.asarray(ell)[None, :] + 1.0
    got = ctx.gp_predict(X, y, alpha, ell, 0.05, 1e-6, far)
    assert np.all(np.abs(got["mean"]) < 1e-12)
    assert np.all(np.abs(got["var"] - alpha ** 2) <= 1e-12 * alpha ** 2)


# ---- 7. status ---------------------------------------------------------------------------------------------------------------
def _raw(ctx, X, y, alpha, ell, sigma, jitter, Xs, mean, var, n=None, m=None, ldx=None, ldxs=None, D=None, n_ell=None,
         null=()):
    """gpmi_gp_predict with every argument as given (no checks of the Python layer in front)."""
    X = np.asfortranarray(X, dtype=float); Xs = np.asfortranarray(Xs, dtype=float)
    y = np.ascontiguousarray(y, dtype=float); ell = np.ascontiguousarray(ell, dtype=float)
    p = lambda a, nm: None if (a is None or nm in null) else C.c_void_p(a.ctypes.data)
    n = X.shape[0] if n is None else n
    m = Xs.shape[0] if m is None else m
    return ctx._lib.gpmi_gp_predict(ctx._h, p(X, "X"), int(n), int(X.shape[0] if ldx is None else ldx),
                                    int(X.shape[1] if D is None else D), p(y, "y"), C.c_double(alpha), p(ell, "ell"),
                                    int(ell.size if n_ell is None else n_ell), C.c_double(sigma), C.c_double(jitter), p(Xs, "Xs"),
                                    int(m), int(Xs.shape[0] if ldxs is None else ldxs), p(mean, "mean"), p(var, "var"))


@pytest.mark.parametrize("n,m,want_var", [(40, 30, True), (600, 200, True), (600, 200, False)])
def test_not_positive_definite_gives_status_and_nan(ctx, n, m, want_var):
    X, y, Xs = pr.inputs(n, 2, m)
    X[n // 2: n // 2 + 8] = X[n // 2 - 1]       # nine copies of one point, no noise, no jitter: singular
    got = ctx.gp_predict(X, y, 1.0, (0.3,), 0.0, 0.0, Xs, want_var=want_var)
    assert 0 < got["info"] <= n
    assert np.all(np.isnan(got["mean"]))
    if want_var:
        assert np.all(np.isnan(got["var"]))
    ok = ctx.gp_predict(X, y, 1.0, (0.3,), 0.1, 1e-6, Xs)     # the same data with noise: fine
    assert ok["info"] == 0 and np.all(np.isfinite(ok["mean"])) and np.all(np.isfinite(ok["var"]))


def test_bad_arguments_return_earg_and_leave_the_context_usable(ctx):
    X, y, Xs = pr.inputs(50, 2, 20)
    mean = np.zeros(20); var = np.zeros(20)
    good = dict(X=X, y=y, alpha=1.0, ell=[0.3, 0.4], sigma=0.1, jitter=1e-6, Xs=Xs, mean=mean, var=var)
    bad = [dict(n=0), dict(m=0), dict(n=-3), dict(D=0), dict(D=65), dict(ldx=49), dict(ldxs=19), dict(alpha=0.0),
           dict(alpha=-1.0), dict(ell=[0.3, 0.0]), dict(ell=[-0.3, 0.4]), dict(sigma=-0.1), dict(n_ell=3), dict(null=("X",)),
           dict(null=("y",)), dict(null=("Xs",)), dict(null=("mean",)), dict(null=("ell",))]
    for change in bad:
        rc = _raw(ctx, **{**good, **change})
        assert rc == -1, (change, rc)
        assert ctx._lib.gpmi_last_error()
    assert _raw(ctx, **good) == 0
    want = pr.predict(X, y, Xs, 1.0, [0.3, 0.4], 0.1, 1e-6)
    assert pr.max_rel(mean, want[0]) <= pr.MEAN_TOL and np.max(np.abs(var - want[1])) <= pr.VAR_TOL
    import gp_amd
    with pytest.raises(gp_amd.GpmiError):
        ctx.gp_predict(X, y[:-1], 1.0, [0.3, 0.4], 0.1, 1e-6, Xs)
    with pytest.raises(gp_amd.GpmiError):
        ctx.set_option("small_pr", 5000)
    with pytest.raises(gp_amd.GpmiError):
        ctx.set_option("predict_mb", -1)


# ---- 8. gpmi_seq_marginals ---------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-8):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


def _posterior(orc, n, l=0.9):
    t = np.linspace(0, 0.15 * n, n)
    return orc.p_dotXn(t, np.sin(t), 1.0, l, 0.1)


def _scenario(orc, ctx, which):
    """The three scenarios of tests/test_gpu_seq.py: (X, mn, Kn, alpha, ell, Xs)."""
    if which == "1d":
        rng = np.random.default_rng(11)
        n = 200
        X = (np.arange(n) * 1.0 + rng.uniform(-0.2, 0.2, n)).reshape(-1, 1)
        mn, Kn = _posterior(orc, n)
        return X, mn, Kn, 1.3, [0.8], np.array([[v] for v in (3.3, 150.2, 3.9, 77.0, 77.5, 12.25, 199.9, -2.0)])
    if which == "ard3d":
        rng = np.random.default_rng(5)
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
        X = g + rng.uniform(-0.15, 0.15, g.shape)
        mn, Kn = _posterior(orc, X.shape[0])
        return X, mn, Kn, 0.9, np.array([0.7, 0.9, 0.6]), rng.uniform(0, 6, size=(12, 3))
    from gp_amd import ode_gp      # R/tests.R:60-97: the N = 21 grid; cond(K_XX + 1e-6 I) ~ 1e7
    t = np.linspace(-2, 2, 21)
    f = np.exp(t)
    p = ode_gp.p_dotXn(t, f, [1.0, 1.0], 0.05, joint=True, ctx=ctx)
    ps = ode_gp.p_Xn(t, f, [1.0, 1.0], 0.05, joint=True, ctx=ctx)
    X = ps["condMean"].reshape(-1, 1)
    return X, p["condMean"], p["condVar"], 1.0, [1.0], np.linspace(0.0, 7.0, 41).reshape(-1, 1)


@pytest.mark.parametrize("which", ["1d", "ard3d", "reference"])
def test_seq_marginals_are_first_steps_of_fresh_samplers(orc, ctx, which):
    X, mn, Kn, alpha, ell, Xs = _scenario(orc, ctx, which)
    s = ctx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=4)
    mean, var = s.marginals(Xs)
    assert s.count == 0
    steps = []
    for xs in Xs:
        f = ctx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=1)
        steps.append(f.step(xs))
        f.close()
    steps = np.asarray(steps)
    print("%s: vs step mean %.2e var %.2e" % (which, np.max(np.abs(mean - steps[:, 0])), np.max(np.abs(var - steps[:, 1]))))
    assert _close(mean, steps[:, 0]) and _close(var, steps[:, 1])
    wm, wv = pr.seq_marginals(X, mn, Kn, alpha, ell, 1e-6, Xs, float)
    print("%s: vs reference mean %.2e var %.2e" % (which, np.max(np.abs(mean - wm)), np.max(np.abs(var - wv))))
    assert _close(mean, wm) and _close(var, wv)
    m2, v2 = s.marginals(Xs)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_array_equal(v2, var)


def test_seq_marginals_leave_the_sampler_alone(orc, ctx):
    X, mn, Kn, alpha, ell, Xs = _scenario(orc, ctx, "ard3d")
    a = ctx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=8)
    b = ctx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=8)
    for s in (a, b):
        for xs, dz in ((Xs[0], 0.3), (Xs[1], -0.2)):
            mu, v = s.step(xs)
            s.commit(mu + dz)
    fresh = ctx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=1).marginals(Xs)
    got = a.marginals(Xs)
    assert a.count == 2
    np.testing.assert_array_equal(got[0], fresh[0])      # no committed draw enters the marginals
    np.testing.assert_array_equal(got[1], fresh[1])
    np.testing.assert_array_equal(a.step(Xs[2]), b.step(Xs[2]))
    # a pending step survives the call as well
    a.marginals(Xs[:5])
    assert a.count == 2
    a.commit(0.4); b.commit(0.4)
    np.testing.assert_array_equal(a.step(Xs[3]), b.step(Xs[3]))
    assert a.count == 3 and b.count == 3


def test_seq_marginals_in_chunks(octx):
    from gp_amd import synth
    n, m = 2048, 300
    X, y = synth.synth(n, 3)
    mn = 0.5 * y
    rng = np.random.default_rng(8)
    A = rng.standard_normal((n, 4))
    Kn = 0.05 * np.eye(n) + 0.01 * (A @ A.T)
    alpha, ell = 1.2, [0.08, 0.1, 0.07]
    Xs = rng.uniform(-0.1, 1.1, size=(m, 3))
    s = octx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=2)
    octx.set_option("predict_mb", 0)
    one = s.marginals(Xs)
    octx.set_option("predict_mb", 128)       # 128 + 128 + 44 rows
    chunks = s.marginals(Xs)
    octx.set_option("predict_mb", 0)
    assert _close(chunks[0], one[0]) and _close(chunks[1], one[1])
    for j in (0, 127, 128, 299):
        f = octx.seq_sampler(X, mn, Kn, alpha, ell, 1e-6, max_steps=1)
        mu, v = f.step(Xs[j])
        f.close()
        assert _close(chunks[0][j], mu) and _close(chunks[1][j], v)
    assert np.all(chunks[1] > 0)      # (the Kn term adds variance: alpha^2 is no upper bound here)


# ---- 9. host layers ----------------------------------------------------------------------------------------------------------
def test_ode_gp_layers_return_what_the_context_returns(orc, ctx):
    from gp_amd import ode_gp
    X, y, Xs = pr.inputs(120, 3, 50)
    a = ode_gp.p_fXs(X, y, [1.0, list(pr.ARD3)], 0.1, Xs, jitter=1e-6, ctx=ctx)
    b = ctx.gp_predict(X, y, 1.0, pr.ARD3, 0.1, 1e-6, Xs)
    np.testing.assert_array_equal(a["mean"], b["mean"])
    np.testing.assert_array_equal(a["var"], b["var"])
    a = ode_gp.p_fXs(X, y, [1.0, 0.3], 0.1, Xs, want_var=False, ctx=ctx)
    assert a["var"] is None and a["info"] == 0
    Xq, mn, Kn, alpha, ell, Xq_s = _scenario(orc, ctx, "1d")
    f = ode_gp.create_p_dotXnS([Xq[:, 0]], mn, Kn, [alpha, ell], ctx=ctx)
    got = f.marginals(Xq_s)
    want = ctx.seq_sampler(Xq, mn, Kn, alpha, ell, 1e-6, max_steps=1).marginals(Xq_s)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    first = f(Xq_s[0], z=0.0)     # the closure still samples: its first call is the first marginal
    assert _close(first["mu"], got[0][0]) and _close(first["sigma"], got[1][0])
