"""GPU: leading dimensions across the C ABI of the host-buffer entry points, on each path a call can take (one launch through
the pinned, device-mapped buffer / the chain through the staging buffers).

Every case calls the library through gp_amd._lib.load() with raw ctypes arguments (the Python wrappers always pass packed
matrices) twice with the same data: packed (ld = rows), then with every matrix argument at leading dimension rows + 3, the
padding rows of the inputs NaN and the output arrays pre-filled with a sentinel.  The padded results must equal the packed ones
bit for bit -- outputs, gradient and return code -- and every padding row of every output must still hold the sentinel.

The bit-for-bit comparison rests on each packed call repeating itself bit for bit at its shape: every reduction of the
library has a fixed order, and the parent of the commit that added this file was checked to repeat itself on every case below
(no exception was found, so no case falls back to a tolerance).

A path is forced the way the neighbouring tests do it: a fresh Context with the relevant small_* option at 0 takes the chain,
the default takes one workgroup; the three hard-coded switches (gpmi_exact_gp_f at n <= 256, gpmi_rbf_cov_chol at n <= 64, the
interpolated models at n <= 256 with k <= 8) get one size either side.  Shapes: n = 37, D = 2, m = 5 -- no multiple of 16 or
64, far below any workload size, accepted by every chain."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, M = 37, 2, 5
PAD = 3
SENTINEL = -777.25
ALPHA, ELL, SIGMA, JIT = 1.1, np.array([0.7, 1.3]), 0.2, 1e-6
NORMAL, BERNOULLI, LOGSD, NONE = 0, 1, 2, 3


def _d(x):
    return C.c_double(float(x))


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Bufs:
    """The arguments of one call: matrices at leading dimension rows + pad."""

    def __init__(self, pad):
        self.pad = pad
        self.keep, self.outs = [], []

    def mat(self, A):
        """(pointer, ld) of an input matrix; its padding rows are NaN."""
        A = np.asarray(A, dtype=np.float64)
        A = A.reshape(A.shape[0], -1)
        buf = np.full((A.shape[0] + self.pad, A.shape[1]), np.nan, order="F")
        buf[:A.shape[0]] = A
        self.keep.append(buf)
        return _p(buf), buf.shape[0]

    def vec(self, v, dtype=np.float64):
        v = np.ascontiguousarray(v, dtype=dtype)
        self.keep.append(v)
        return _p(v)

    def out(self, rows, cols=1, want=True):
        """(valid part, pointer, ld) of an output matrix pre-filled with the sentinel; want=False: the NULL arm."""
        if not want:
            return None, None, rows + self.pad
        buf = np.full((rows + self.pad, cols), SENTINEL, order="F")
        self.outs.append((buf, rows))
        return buf[:rows], _p(buf), buf.shape[0]

    def padding_untouched(self):
        return all(np.all(buf[rows:] == SENTINEL) for buf, rows in self.outs)


def _data(n, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, D))
    y = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)
    return rng, X, y


# ---- the calls: fn(lib, h, B) -> {name: array or int} ----------------------------------------------------------------
def exact_gp_f(n):
    def fn(lib, h, B):
        rng, X, _ = _data(n)
        pX, ldx = B.mat(X)
        f = np.full(n, SENTINEL)
        rc = lib.gpmi_exact_gp_f(h, pX, n, ldx, D, _d(ALPHA), B.vec(ELL), D, _d(JIT), B.vec(rng.standard_normal(n)), _p(f))
        return {"rc": rc, "f": f}
    return fn


def logml(lib, h, B):
    _, X, y = _data(N)
    pX, ldx = B.mat(X)
    out = np.full(3, SENTINEL)
    rc = lib.gpmi_logml(h, pX, N, ldx, D, B.vec(y), _d(ALPHA), B.vec(ELL), D, _d(SIGMA), _d(JIT), _p(out))
    return {"rc": rc, "out": out}


def logml_grad(lib, h, B):
    _, X, y = _data(N)
    pX, ldx = B.mat(X)
    out = np.full(3, SENTINEL); g = np.full(2 + D, SENTINEL)
    rc = lib.gpmi_logml_grad(h, pX, N, ldx, D, B.vec(y), _d(ALPHA), B.vec(ELL), D, _d(SIGMA), _d(JIT), _p(out), _p(g))
    return {"rc": rc, "out": out, "grad": g}


def _grid_pars(G):
    q = np.arange(G)
    return 1.0 + 0.05 * q, 0.6 + 0.07 * q, 0.2 + 0.01 * q


def logml_grad_grid(G):
    def fn(lib, h, B):
        _, X, y = _data(N)
        pX, ldx = B.mat(X)
        a, r, s = _grid_pars(G)
        out = np.full((G, 3), SENTINEL); g = np.full((G, 3), SENTINEL); info = np.full(G, -1, dtype=np.int32)
        rc = lib.gpmi_logml_grad_grid(h, pX, N, ldx, D, B.vec(y), B.vec(a), B.vec(r), B.vec(s), G, _d(JIT), _p(out), _p(g), _p(info))
        return {"rc": rc, "out": out, "grad": g, "info": info}
    return fn


def logml_grid(ard):
    def fn(lib, h, B):
        G = 3
        _, X, y = _data(N)
        pX, ldx = B.mat(X)
        a, r, s = _grid_pars(G)
        out = np.full((G, 3), SENTINEL); info = np.full(G, -1, dtype=np.int32)
        if ard:
            E = np.stack([r, 1.5 * r], axis=1)
            rc = lib.gpmi_logml_grid_ard(h, pX, N, ldx, D, B.vec(y), B.vec(a), B.vec(E), B.vec(s), G, _d(JIT), _p(out), _p(info))
        else:
            rc = lib.gpmi_logml_grid(h, pX, N, ldx, D, B.vec(y), B.vec(a), B.vec(r), B.vec(s), G, _d(JIT), _p(out), _p(info))
        return {"rc": rc, "out": out, "info": info}
    return fn


def gp_condition(m=M):
    def fn(lib, h, B):
        rng = np.random.default_rng(11)
        t = np.linspace(0.0, 6.0, N); ts = np.linspace(0.1, 5.9, m); y = np.sin(t) + 0.05 * rng.standard_normal(N)
        mn = np.full(m, SENTINEL)
        Kn, pK, ldk = B.out(m, m)
        rc = lib.gpmi_gp_condition(h, B.vec(t), N, B.vec(ts), m, B.vec(y), _d(1.0), _d(0.8), _d(0.01), _d(1e-6), 0, 2, 3, 0,
                                   _p(mn), pK, ldk)
        return {"rc": rc, "mn": mn, "Kn": Kn}
    return fn


def gp_predict(want_var):
    def fn(lib, h, B):
        rng, X, y = _data(N)
        pX, ldx = B.mat(X)
        pXs, ldxs = B.mat(rng.uniform(-1.0, 1.0, (M, D)))
        mean = np.full(M, SENTINEL); var = np.full(M, SENTINEL) if want_var else None
        rc = lib.gpmi_gp_predict(h, pX, N, ldx, D, B.vec(y), _d(ALPHA), B.vec(ELL), D, _d(SIGMA), _d(JIT), pXs, M, ldxs, _p(mean),
                                 _p(var))
        res = {"rc": rc, "mean": mean}
        if want_var:
            res["var"] = var
        return res
    return fn


def exact_gp_f_vjp(want_f):
    def fn(lib, h, B):
        k = 2
        rng, X, _ = _data(N)
        pX, ldx = B.mat(X)
        pZ, ldz = B.mat(rng.standard_normal((N, k)))
        pFb, ldfb = B.mat(rng.standard_normal((N, k)))
        F, pF, ldf = B.out(N, k, want_f)
        Zb, pZb, ldzb = B.out(N, k)
        g = np.full(1 + D, SENTINEL)
        rc = lib.gpmi_exact_gp_f_vjp(h, pX, N, ldx, D, _d(ALPHA), B.vec(ELL), D, _d(JIT), pZ, k, ldz, pFb, ldfb, pF, ldf, pZb, ldzb,
                                     _p(g))
        res = {"rc": rc, "Zbar": Zb, "grad": g}
        if want_f:
            res["F"] = F
        return res
    return fn


def _head(rng, family, n):
    k = 2 if family == LOGSD else 1
    Y = rng.standard_normal((n, M))
    if family == BERNOULLI:
        Y = (Y > 0.0).astype(np.float64)
    return k, Y


def latent_gp_lp_grad(family, want_f=True, want_fbar=True):
    def fn(lib, h, B):
        rng, X, _ = _data(N)
        k, Y = _head(rng, family, N)
        pX, ldx = B.mat(X)
        pZ, ldz = B.mat(rng.standard_normal((N, k)))
        pY, ldy = B.mat(Y)
        F, pF, ldf = B.out(N, k, want_f)
        Fb, pFb, ldfb = B.out(N, k, want_fbar)
        Zb, pZb, ldzb = B.out(N, k)
        out = np.full(2, SENTINEL); g = np.full(1 + D, SENTINEL)
        rc = lib.gpmi_latent_gp_lp_grad(h, pX, N, ldx, D, _d(ALPHA), B.vec(ELL), D, _d(JIT), pZ, k, ldz, family, pY, M, ldy, _d(0.7),
                                        _p(out), pF, ldf, pFb, ldfb, pZb, ldzb, _p(g))
        res = {"rc": rc, "out": out, "Zbar": Zb, "grad": g}
        if want_f:
            res["F"] = F
        if want_fbar:
            res["Fbar"] = Fb
        return res
    return fn


def centered_gp_lp_grad(family):
    def fn(lib, h, B):
        rng, X, _ = _data(N)
        k, Y = _head(rng, family, N)
        if family == NONE:
            k = 2
        pX, ldx = B.mat(X)
        pF, ldf = B.mat(rng.standard_normal((N, k)))
        pY, ldy = (None, N) if family == NONE else B.mat(Y)
        Fg, pFg, ldfg = B.out(N, k)
        out = np.full(4, SENTINEL); g = np.full(1 + D, SENTINEL)
        rc = lib.gpmi_centered_gp_lp_grad(h, pX, N, ldx, D, _d(ALPHA), B.vec(ELL), D, _d(JIT), pF, k, ldf, family, pY,
                                          0 if family == NONE else M, ldy, _d(0.7), _p(out), pFg, ldfg, _p(g))
        return {"rc": rc, "out": out, "Fgrad": Fg, "grad": g}
    return fn


def _line(n):
    return np.linspace(0.0, 0.5 * n, n)    # about one point per length-scale: well conditioned with the 1e-10 jitter


def rbf_cov_chol(n):
    def fn(lib, h, B):
        L, pL, ldl = B.out(n, n)
        dL, pdL, lddl = B.out(n, n)
        rc = lib.gpmi_rbf_cov_chol(h, B.vec(_line(n)), n, _d(0.4), pL, ldl, pdL, lddl)
        return {"rc": rc, "L": L, "dL": dL}
    return fn


LP = np.linspace(0.3, 0.55, 4)


def tri(model, n, vjp=True, want_f=True):
    """The interpolated models' products and reverse sweeps (model "hermite" / "gp"); vjp=False: gpmi_interp_gp_Lz (F alone)."""
    def fn(lib, h, B):
        k = 2
        rng = np.random.default_rng(5)
        x = _line(n)
        if model == "gp":
            rc0 = lib.gpmi_interp_gp_build(h, B.vec(x), n, B.vec(LP), LP.size, _d(1.0), _d(1e-10))
        else:
            rc0 = lib.gpmi_interp_build(h, B.vec(x), n, B.vec(LP), LP.size)
        assert rc0 == 0, lib.gpmi_last_error()
        pZ, ldz = B.mat(rng.standard_normal((n, k)))
        F, pF, ldf = B.out(n, k, want_f)
        if not vjp:
            return {"rc": lib.gpmi_interp_gp_Lz(h, _d(0.41), pZ, k, ldz, pF, ldf), "F": F}
        pFb, ldfb = B.mat(rng.standard_normal((n, k)))
        Zb, pZb, ldzb = B.out(n, k)
        lbar = np.full(1, SENTINEL)
        call = lib.gpmi_interp_gp_Lz_vjp if model == "gp" else lib.gpmi_approx_Lz_vjp
        rc = call(h, _d(0.41), pZ, k, ldz, pFb, ldfb, pF, ldf, pZb, ldzb, _p(lbar))
        res = {"rc": rc, "Zbar": Zb, "lbar": lbar}
        if want_f:
            res["F"] = F
        return res
    return fn


def sample_derivs_batch(want_mus):
    def fn(lib, h, B):
        nb = 3
        rng = np.random.default_rng(13)
        t = np.linspace(0.0, 6.0, N); ts = np.linspace(0.1, 5.9, M)
        pY, ldy = B.mat(np.sin(t)[:, None] + 0.05 * rng.standard_normal((N, nb)))
        pZ, ldz = B.mat(rng.standard_normal((M, nb)))
        par = np.array([[0.8, 1.0, 0.1], [0.9, 1.1, 0.12], [1.0, 0.9, 0.08]])
        dr, pdr, ldd = B.out(M, nb)
        mu, pmu, ldmu = B.out(M, nb, want_mus)
        info = np.full(nb, -1, dtype=np.int32)
        rc = lib.gpmi_sample_derivs_batch(h, B.vec(t), N, B.vec(ts), M, pY, ldy, B.vec(par), nb, _d(1e-6), pZ, ldz, pdr, ldd, pmu, ldmu,
                                          _p(info))
        res = {"rc": rc, "draws": dr, "info": info}
        if want_mus:
            res["mus"] = mu
        return res
    return fn


ONE, CHAIN = "one workgroup", "chain"
# (id, {option: value} of the context, call)
CASES = [
    ("exact_gp_f-n37", {}, exact_gp_f(N)),
    ("exact_gp_f-n300", {}, exact_gp_f(300)),
    ("logml-one", {}, logml),
    ("logml-chain", {"small_n1": 0}, logml),
    ("logml_grad-one", {}, logml_grad),
    ("logml_grad-chain", {"small_ng1": 0}, logml_grad),
    ("logml_grad_grid-G3-pinned", {}, logml_grad_grid(3)),
    ("logml_grad_grid-G9-batched", {}, logml_grad_grid(9)),
    ("logml_grad_grid-G3-lanes", {"small_ng": 0}, logml_grad_grid(3)),
    ("logml_grid", {}, logml_grid(False)),
    ("logml_grid-chain", {"small_n1": 0}, logml_grid(False)),
    ("logml_grid_ard", {}, logml_grid(True)),
    ("logml_grid_ard-chain", {"small_n1": 0}, logml_grid(True)),
    ("gp_condition-one", {}, gp_condition()),
    ("gp_condition-chain", {"small_gc": 0}, gp_condition()),
    ("gp_predict-one", {}, gp_predict(True)),
    ("gp_predict-one-novar", {}, gp_predict(False)),
    ("gp_predict-chain", {"small_pr": 0}, gp_predict(True)),
    ("gp_predict-chain-novar", {"small_pr": 0}, gp_predict(False)),
    ("exact_gp_f_vjp-one", {}, exact_gp_f_vjp(True)),
    ("exact_gp_f_vjp-one-noF", {}, exact_gp_f_vjp(False)),
    ("exact_gp_f_vjp-chain", {"small_vjp": 0}, exact_gp_f_vjp(True)),
    ("exact_gp_f_vjp-chain-noF", {"small_vjp": 0}, exact_gp_f_vjp(False)),
    ("latent-normal-one", {}, latent_gp_lp_grad(NORMAL)),
    ("latent-bernoulli-one", {}, latent_gp_lp_grad(BERNOULLI)),
    ("latent-logsd-one", {}, latent_gp_lp_grad(LOGSD)),
    ("latent-logsd-one-noF-noFbar", {}, latent_gp_lp_grad(LOGSD, False, False)),
    ("latent-normal-chain", {"small_vjp": 0}, latent_gp_lp_grad(NORMAL)),
    ("latent-bernoulli-chain", {"small_vjp": 0}, latent_gp_lp_grad(BERNOULLI)),
    ("latent-logsd-chain", {"small_vjp": 0}, latent_gp_lp_grad(LOGSD)),
    ("latent-logsd-chain-noF-noFbar", {"small_vjp": 0}, latent_gp_lp_grad(LOGSD, False, False)),
    ("centered-normal-one", {}, centered_gp_lp_grad(NORMAL)),
    ("centered-logsd-one", {}, centered_gp_lp_grad(LOGSD)),
    ("centered-none-one", {}, centered_gp_lp_grad(NONE)),
    ("centered-normal-chain", {"small_cen": 0}, centered_gp_lp_grad(NORMAL)),
    ("centered-logsd-chain", {"small_cen": 0}, centered_gp_lp_grad(LOGSD)),
    ("centered-none-chain", {"small_cen": 0}, centered_gp_lp_grad(NONE)),
    ("rbf_cov_chol-n37", {}, rbf_cov_chol(N)),
    ("rbf_cov_chol-n100", {}, rbf_cov_chol(100)),
    ("approx_Lz_vjp-n37", {}, tri("hermite", N)),
    ("approx_Lz_vjp-n37-noF", {}, tri("hermite", N, want_f=False)),
    ("approx_Lz_vjp-n300", {}, tri("hermite", 300)),
    ("interp_gp_Lz_vjp-n37", {}, tri("gp", N)),
    ("interp_gp_Lz_vjp-n300", {}, tri("gp", 300)),
    ("interp_gp_Lz-n37", {}, tri("gp", N, vjp=False)),
    ("interp_gp_Lz-n300", {}, tri("gp", 300, vjp=False)),
    ("sample_derivs_batch-one", {}, sample_derivs_batch(True)),
    ("sample_derivs_batch-one-nomus", {}, sample_derivs_batch(False)),
    ("sample_derivs_batch-lanes", {"small_sd": 0}, sample_derivs_batch(True)),
    ("sample_derivs_batch-lanes-nomus", {"small_sd": 0}, sample_derivs_batch(False)),
]


def run_case(lib, h, fn, pad):
    """({name: copy of the result}, padding untouched) of one call."""
    B = Bufs(pad)
    res = fn(lib, h, B)
    return {k: np.array(v) for k, v in res.items()}, B.padding_untouched()


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def contexts():
    """One context per set of options, made on first use."""
    import gp_amd
    made = {}

    def get(opts):
        key = tuple(sorted(opts.items()))
        if key not in made:
            c = gp_amd.Context(0)
            for name, value in key:
                c.set_option(name, value)
            made[key] = c
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_leading_dimensions(contexts, case):
    _, opts, fn = case
    c = contexts(opts)
    packed, ok0 = run_case(c._lib, c._h, fn, 0)
    padded, ok1 = run_case(c._lib, c._h, fn, PAD)
    assert packed["rc"] == 0, c._lib.gpmi_last_error()
    assert ok0 and ok1, "a padding row of an output was written"
    assert packed.keys() == padded.keys()
    for name in packed:
        assert np.all(packed[name] != SENTINEL), name + " was not written"
        assert same_bits(packed[name], padded[name]), name


def test_vjp_gradient_of_nine_keeps_its_own_slot(contexts):
    """gpmi_exact_gp_f_vjp with D = 8 length-scales returns 1 + 8 gradient entries: in the one-launch layout they need a slot
    of nine doubles (a slot of eight let the last one land on F[0, 0]).  F of the one-workgroup call against F of the chain:
    both factor the same matrix backward-stably, so they differ by c cond(K) eps with K = alpha^2 K0 + 1e-6 I, cond(K) <=
    n alpha^2 / 1e-6 < 5e7 at n = 37: 100 cond eps = 1e-6 of max|F| bounds the difference."""
    d8, k = 8, 2
    rng = np.random.default_rng(17)
    X = rng.uniform(-1.0, 1.0, (N, d8)); Z = rng.standard_normal((N, k)); Fb = rng.standard_normal((N, k))
    ell = np.linspace(0.7, 1.4, d8)

    def call(c):
        B = Bufs(0)
        pX, ldx = B.mat(X); pZ, ldz = B.mat(Z); pFb, ldfb = B.mat(Fb)
        F, pF, ldf = B.out(N, k); Zb, pZb, ldzb = B.out(N, k)
        g = np.full(1 + d8, SENTINEL)
        rc = c._lib.gpmi_exact_gp_f_vjp(c._h, pX, N, ldx, d8, _d(ALPHA), B.vec(ell), d8, _d(JIT), pZ, k, ldz, pFb, ldfb, pF, ldf, pZb,
                                        ldzb, _p(g))
        assert rc == 0
        return F, g
    F1, g1 = call(contexts({}))
    F2, g2 = call(contexts({"small_vjp": 0}))
    assert np.max(np.abs(F1 - F2)) <= 1e-6 * np.max(np.abs(F2))
    assert np.all(g1 != SENTINEL) and np.all(g2 != SENTINEL)


def test_pinned_buffer_regrown():
    """A one-launch call that fits the initial 64 KiB pinned buffer, one that makes it grow (gpmi_gp_condition with m = 96:
    m * m doubles exceed 64 KiB, n + m + 1 = 134 rows stay one workgroup), and the first call again, on a path that did not arm
    its completion flag before: the fresh allocation's flag word is whatever the allocator returned."""
    import gp_amd
    c = gp_amd.Context(0)
    try:
        first, _ = run_case(c._lib, c._h, gp_condition(), 0)
        big, _ = run_case(c._lib, c._h, gp_condition(96), 0)
        again, _ = run_case(c._lib, c._h, gp_condition(), 0)
        assert first["rc"] == 0 and big["rc"] == 0 and again["rc"] == 0
        assert np.all(big["Kn"] != SENTINEL) and np.all(big["mn"] != SENTINEL)
        for name in first:
            assert same_bits(first[name], again[name]), name
    finally:
        c.close()
