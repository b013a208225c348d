"""The catalogue of calls across the C ABI that the GPU tests share (test_gpu_host_buffers.py: leading dimensions;
test_gpu_workspace_history.py: independence of what the context's scratch held before).

A call is fn(lib, h, B) -> {name: array or int}: it drives one host-buffer entry point of gp_amd._lib.load() through raw ctypes
on the context handle h, taking every matrix argument from B (a Bufs: leading dimension rows + B.pad, the padding rows of the
inputs NaN, the outputs pre-filled with a sentinel), and returns the return code and every output.  A case is
(id, {option: value} of the context, call).

CASES: n = 37, D = 2, m = 5 -- no multiple of 16 or 64, far below any workload size, accepted by every chain -- on each path a
call can take: a context with the relevant small_* option at 0 takes the chain, the default takes one workgroup; the
hard-coded switches (gpmi_exact_gp_f at n <= 256, gpmi_rbf_cov_chol at n <= 64, the interpolated models at n <= 256 with
k <= 8) get one size either side.
BLOCKED_CASES: the same calls at the smallest ragged orders that leave one panel (edge tiles, a partial last k-step, the
augmented row, odd base offsets), forced onto the blocked factorisation and the chains, on well-conditioned data: the inputs
of gp_amd.synth with a noise variance of 0.01, about ten points per length-scale for the time series."""
import ctypes as C

import numpy as np
import pytest

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

    def inout(self, A):
        """(valid part, pointer, ld) of a matrix overwritten in place: A in the valid rows, the sentinel in the padding rows."""
        A = np.asarray(A, dtype=np.float64)
        valid, ptr, ld = self.out(A.shape[0], A.shape[1])
        valid[:] = A
        return valid, ptr, ld

    def padding_untouched(self):
        return all(np.all(buf[rows:] == SENTINEL) for buf, rows in self.outs)


def _data(n, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, D))
    y = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)
    return rng, X, y


class Src:
    """Where the D-dimensional calls take their inputs and hyper-parameters from."""

    def __init__(self, data, alpha, ell, sigma):
        self.data, self.alpha, self.ell, self.sigma = data, alpha, ell, sigma


def _synth_data(n, seed=7):
    from gp_amd import synth
    X, y = synth.synth(n, D)
    return np.random.default_rng(seed), X, y


UNIFORM = Src(_data, ALPHA, ELL, SIGMA)                       # the catalogue at n = 37
SYNTH = Src(_synth_data, 1.0, np.array([0.3, 0.4]), 0.1)      # the blocked cases: noise variance 0.01


def _series(n, m, seed=11):
    """A noisy sine at about ten points per unit length-scale, n times t and m prediction times ts inside them."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 0.1 * n, n); ts = np.linspace(0.05, 0.1 * n - 0.05, m)
    return rng, t, ts, np.sin(t) + 0.05 * rng.standard_normal(n)


# ---- the calls: fn(lib, h, B) -> {name: array or int} ----------------------------------------------------------------
def exact_gp_f(n):
    def fn(lib, h, B):
        rng, X, _ = _data(n)
        pX, ldx = B.mat(X)
        f = np.full(n, SENTINEL)
        rc = lib.gpmi_exact_gp_f(h, pX, n, ldx, D, _d(ALPHA), B.vec(ELL), D, _d(JIT), B.vec(rng.standard_normal(n)), _p(f))
        return {"rc": rc, "f": f}
    return fn


def logml_at(n, src=UNIFORM):
    def fn(lib, h, B):
        _, X, y = src.data(n)
        pX, ldx = B.mat(X)
        out = np.full(3, SENTINEL)
        rc = lib.gpmi_logml(h, pX, n, ldx, D, B.vec(y), _d(src.alpha), B.vec(src.ell), D, _d(src.sigma), _d(JIT), _p(out))
        return {"rc": rc, "out": out}
    return fn


logml = logml_at(N)


def logml_grad_at(n, src=UNIFORM):
    def fn(lib, h, B):
        _, X, y = src.data(n)
        pX, ldx = B.mat(X)
        out = np.full(3, SENTINEL); g = np.full(2 + D, SENTINEL)
        rc = lib.gpmi_logml_grad(h, pX, n, ldx, D, B.vec(y), _d(src.alpha), B.vec(src.ell), D, _d(src.sigma), _d(JIT), _p(out), _p(g))
        return {"rc": rc, "out": out, "grad": g}
    return fn


logml_grad = logml_grad_at(N)


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


def logml_grid(ard, n=N, G=3, src=UNIFORM, pars=_grid_pars):
    def fn(lib, h, B):
        _, X, y = src.data(n)
        pX, ldx = B.mat(X)
        a, r, s = pars(G)
        out = np.full((G, 3), SENTINEL); info = np.full(G, -1, dtype=np.int32)
        if ard:
            E = np.stack([r, 1.5 * r], axis=1)
            rc = lib.gpmi_logml_grid_ard(h, pX, n, ldx, D, B.vec(y), B.vec(a), B.vec(E), B.vec(s), G, _d(JIT), _p(out), _p(info))
        else:
            rc = lib.gpmi_logml_grid(h, pX, n, ldx, D, B.vec(y), B.vec(a), B.vec(r), B.vec(s), G, _d(JIT), _p(out), _p(info))
        return {"rc": rc, "out": out, "info": info}
    return fn


def synth_grid_pars(G):
    q = np.arange(G)
    return 1.0 + 0.05 * q, 0.3 + 0.02 * q, 0.1 + 0.01 * q


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


def gp_condition_series(n, m):
    """The (QQ, RQ, RR) conditioning of sample_derivs on the time series of _series."""
    def fn(lib, h, B):
        _, t, ts, y = _series(n, m)
        mn = np.full(m, SENTINEL)
        Kn, pK, ldk = B.out(m, m)
        rc = lib.gpmi_gp_condition(h, B.vec(t), n, B.vec(ts), m, B.vec(y), _d(1.0), _d(1.0), _d(0.01), _d(1e-6), 0, 2, 3, 0,
                                   _p(mn), pK, ldk)
        return {"rc": rc, "mn": mn, "Kn": Kn}
    return fn


def gp_predict(want_var, n=N, m=M, src=UNIFORM):
    def fn(lib, h, B):
        rng, X, y = src.data(n)
        pX, ldx = B.mat(X)
        lo, hi = X.min(), X.max()
        pXs, ldxs = B.mat(rng.uniform(-1.0, 1.0, (m, D)) if src is UNIFORM else rng.uniform(lo, hi, (m, D)))
        mean = np.full(m, SENTINEL); var = np.full(m, SENTINEL) if want_var else None
        rc = lib.gpmi_gp_predict(h, pX, n, ldx, D, B.vec(y), _d(src.alpha), B.vec(src.ell), D, _d(src.sigma), _d(JIT), pXs, m, ldxs,
                                 _p(mean), _p(var))
        res = {"rc": rc, "mean": mean}
        if want_var:
            res["var"] = var
        return res
    return fn


def gp_predict_joint(n=N, m=M, nb=3, src=UNIFORM):
    """gpmi_gp_predict_joint with nb draws (post_jitter 1e-6: the posterior covariance of m points is factored)."""
    def fn(lib, h, B):
        rng, X, y = src.data(n)
        pX, ldx = B.mat(X)
        pXs, ldxs = B.mat(rng.uniform(X.min(), X.max(), (m, D)))
        pZ, ldz = B.mat(rng.standard_normal((m, nb)))
        mean = np.full(m, SENTINEL)
        cov, pc, ldc = B.out(m, m)
        dr, pdr, ldd = B.out(m, nb)
        rc = lib.gpmi_gp_predict_joint(h, pX, n, ldx, D, B.vec(y), _d(src.alpha), B.vec(src.ell), D, _d(src.sigma), _d(JIT), pXs, m,
                                       ldxs, _d(1e-6), _p(mean), pc, ldc, pZ, nb, ldz, pdr, ldd)
        return {"rc": rc, "mean": mean, "cov": cov, "draws": dr}
    return fn


def exact_gp_f_vjp(want_f, n=N, src=UNIFORM):
    def fn(lib, h, B):
        k = 2
        rng, X, _ = src.data(n)
        pX, ldx = B.mat(X)
        pZ, ldz = B.mat(rng.standard_normal((n, k)))
        pFb, ldfb = B.mat(rng.standard_normal((n, k)))
        F, pF, ldf = B.out(n, k, want_f)
        Zb, pZb, ldzb = B.out(n, k)
        g = np.full(1 + D, SENTINEL)
        rc = lib.gpmi_exact_gp_f_vjp(h, pX, n, ldx, D, _d(src.alpha), B.vec(src.ell), D, _d(JIT), pZ, k, ldz, pFb, ldfb, pF, ldf, pZb,
                                     ldzb, _p(g))
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


def latent_gp_lp_grad(family, want_f=True, want_fbar=True, n=N, src=UNIFORM):
    def fn(lib, h, B):
        rng, X, _ = src.data(n)
        k, Y = _head(rng, family, n)
        pX, ldx = B.mat(X)
        pZ, ldz = B.mat(rng.standard_normal((n, k)))
        pY, ldy = B.mat(Y)
        F, pF, ldf = B.out(n, k, want_f)
        Fb, pFb, ldfb = B.out(n, k, want_fbar)
        Zb, pZb, ldzb = B.out(n, k)
        out = np.full(2, SENTINEL); g = np.full(1 + D, SENTINEL)
        rc = lib.gpmi_latent_gp_lp_grad(h, pX, n, ldx, D, _d(src.alpha), B.vec(src.ell), D, _d(JIT), pZ, k, ldz, family, pY, M, ldy,
                                        _d(0.7), _p(out), pF, ldf, pFb, ldfb, pZb, ldzb, _p(g))
        res = {"rc": rc, "out": out, "Zbar": Zb, "grad": g}
        if want_f:
            res["F"] = F
        if want_fbar:
            res["Fbar"] = Fb
        return res
    return fn


def centered_gp_lp_grad(family, n=N, src=UNIFORM):
    def fn(lib, h, B):
        rng, X, _ = src.data(n)
        k, Y = _head(rng, family, n)
        if family == NONE:
            k = 2
        pX, ldx = B.mat(X)
        pF, ldf = B.mat(rng.standard_normal((n, k)))
        pY, ldy = (None, n) if family == NONE else B.mat(Y)
        Fg, pFg, ldfg = B.out(n, k)
        out = np.full(4, SENTINEL); g = np.full(1 + D, SENTINEL)
        rc = lib.gpmi_centered_gp_lp_grad(h, pX, n, ldx, D, _d(src.alpha), B.vec(src.ell), D, _d(JIT), pF, k, ldf, family, pY,
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


def interp_build_Lz_grad(n, P=4):
    """gpmi_interp_build (the table of P factors and tangents) followed by gpmi_approx_Lz_grad inside its second interval."""
    def fn(lib, h, B):
        lp = np.linspace(0.3, 0.55, P)
        rc0 = lib.gpmi_interp_build(h, B.vec(_line(n)), n, B.vec(lp), P)
        assert rc0 == 0, lib.gpmi_last_error()
        z = np.random.default_rng(5).standard_normal(n)
        f = np.full(n, SENTINEL); dfdl = np.full(n, SENTINEL)
        rc = lib.gpmi_approx_Lz_grad(h, _d(0.41), B.vec(z), _p(f), _p(dfdl))
        return {"rc": rc, "f": f, "dfdl": dfdl}
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


def _spd(n, seed=3):
    """A well-conditioned symmetric positive definite matrix: a squared-exponential covariance plus 0.01 I."""
    _, X, _ = _synth_data(n) if n > N else _data(n, seed)
    ell = SYNTH.ell if n > N else ELL
    Q = X / ell
    s = np.sum(Q * Q, axis=1)
    return np.exp(-0.5 * np.maximum(s[:, None] + s[None, :] - 2.0 * Q @ Q.T, 0.0)) + 0.01 * np.eye(n)


def potrf(n, A=None):
    """gpmi_potrf in place (A: the matrix, default _spd(n)); the factor comes back with its strict upper triangle zeroed."""
    def fn(lib, h, B):
        L, pL, ldl = B.inout(_spd(n) if A is None else A)
        return {"rc": lib.gpmi_potrf(h, pL, n, ldl), "L": L}
    return fn


def _joint_series(n, seed=17):
    """Stacked observations [y; y'] of a sine at about ten points per length-scale (l = 1)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 0.1 * n, n)
    yy = np.concatenate([np.sin(t), np.cos(t)]) + 0.05 * rng.standard_normal(2 * n)
    return rng, t, yy


def joint_logml(n, grad):
    def fn(lib, h, B):
        _, t, yy = _joint_series(n)
        out = np.full(3, SENTINEL)
        if not grad:
            return {"rc": lib.gpmi_joint_logml(h, B.vec(t), n, B.vec(yy), _d(1.0), _d(1.0), _d(0.1), _d(1e-6), _p(out)), "out": out}
        g = np.full(3, SENTINEL)
        rc = lib.gpmi_joint_logml_grad(h, B.vec(t), n, B.vec(yy), _d(1.0), _d(1.0), _d(0.1), _d(1e-6), _p(out), _p(g))
        return {"rc": rc, "out": out, "grad": g}
    return fn


def joint_predict(n, m, orders=7, nb=3):
    """gpmi_joint_predict of f, f', f'' (orders = 7) at m times with nb draws; one post-jitter per order in its own units."""
    def fn(lib, h, B):
        rng, t, yy = _joint_series(n)
        ts = np.linspace(0.05, 0.1 * n - 0.05, m)
        p = bin(orders).count("1"); pm = p * m
        pZ, ldz = B.mat(rng.standard_normal((pm, nb)))
        mean = np.full(pm, SENTINEL)
        cov, pc, ldc = B.out(pm, pm)
        dr, pdr, ldd = B.out(pm, nb)
        rc = lib.gpmi_joint_predict(h, B.vec(t), n, B.vec(yy), _d(1.0), _d(1.0), _d(0.1), _d(1e-6), B.vec(ts), m, orders,
                                    B.vec(np.full(p, 1e-4)), _p(mean), pc, ldc, pZ, nb, ldz, pdr, ldd)
        return {"rc": rc, "mean": mean, "cov": cov, "draws": dr}
    return fn


def sample_derivs(n, m):
    def fn(lib, h, B):
        rng, t, ts, y = _series(n, m)
        draw = np.full(m, SENTINEL); mu = np.full(m, SENTINEL)
        rc = lib.gpmi_sample_derivs(h, B.vec(t), n, B.vec(ts), m, B.vec(y), _d(1.0), _d(1.0), _d(0.1), _d(1e-6),
                                    B.vec(rng.standard_normal(m)), _p(draw), _p(mu))
        return {"rc": rc, "draw": draw, "mu": mu}
    return fn


def seq_marginals(n=21, m=41):
    """A sampler over the n = 21 states exp(t) of the reference's scenario (R/tests.R:60-97), the first-step moments at m = 41
    new states, and the sampler destroyed again: create factors in the context's workspace and staging buffers."""
    def fn(lib, h, B):
        t = np.linspace(-2.0, 2.0, n)
        pX, ldx = B.mat(np.exp(t))
        Kn = 0.3 * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2) + 0.01 * np.eye(n)
        pK, ldk = B.mat(Kn)
        q = C.c_void_p()
        rc0 = lib.gpmi_seq_create(h, C.byref(q), pX, n, ldx, 1, B.vec(np.exp(t)), pK, ldk, _d(1.0), B.vec([1.0]), 1, _d(1e-6), 4)
        assert rc0 == 0, lib.gpmi_last_error()
        try:
            pXs, ldxs = B.mat(np.linspace(0.1, 7.5, m))
            mean = np.full(m, SENTINEL); var = np.full(m, SENTINEL)
            rc = lib.gpmi_seq_marginals(q, pXs, m, ldxs, _p(mean), _p(var))
        finally:
            lib.gpmi_seq_destroy(q)
        return {"rc": rc, "mean": mean, "var": var}
    return fn


def logml_loo(want_all):
    """gpmi_logml_loo at n = 37; want_all=False: the nullable mu, var, lpd and grad all NULL."""
    def fn(lib, h, B):
        _, X, y = _data(N)
        pX, ldx = B.mat(X)
        out = np.full(3, SENTINEL); loo = np.full(1, SENTINEL); g = np.full(2 + D, SENTINEL)
        mu, var, lpd = np.full(N, SENTINEL), np.full(N, SENTINEL), np.full(N, SENTINEL)
        opt = (mu, var, lpd, g) if want_all else (None,) * 4
        rc = lib.gpmi_logml_loo(h, pX, N, ldx, D, B.vec(y), _d(ALPHA), B.vec(ELL), D, _d(SIGMA), _d(JIT), _p(out), _p(loo), *map(_p, opt))
        res = {"rc": rc, "out": out, "loo": loo}
        if want_all:
            res.update(mu=mu, var=var, lpd=lpd, grad=g)
        return res
    return fn


def logml_hess(n_ell, want_grad=True):
    """gpmi_logml_hess at n = 37 with one length-scale or one per dimension: the Hessian is (2 + n_ell) x (2 + n_ell)."""
    def fn(lib, h, B):
        _, X, y = _data(N)
        pX, ldx = B.mat(X)
        q = 2 + n_ell
        out = np.full(3, SENTINEL); g = np.full(q, SENTINEL)
        H, pH, ldh = B.out(q, q)
        rc = lib.gpmi_logml_hess(h, pX, N, ldx, D, B.vec(y), _d(ALPHA), B.vec(ELL[:n_ell]), n_ell, _d(SIGMA), _d(JIT), _p(out),
                                 _p(g) if want_grad else None, pH, ldh)
        res = {"rc": rc, "out": out, "hess": H}
        if want_grad:
            res["grad"] = g
        return res
    return fn


LR_M, LR_SCALE, LR_AMP, LR_L = 8, 0.25, 1.3, 0.3


def _lowrank_data(seed=23):
    """x sorted in [-0.5, 0.5] (the basis is scaled for that interval), y, the M coefficients z and replicate columns Y."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-0.5, 0.5, N))
    return x, np.sin(3.0 * x) + 0.3 * rng.standard_normal(N), rng.standard_normal(LR_M), rng.standard_normal((N, M))


def hermite_basis(want_dl):
    def fn(lib, h, B):
        x = _lowrank_data()[0]
        P, pP, ldp = B.out(N, LR_M)
        dP, pdP, lddp = B.out(N, LR_M, want_dl)
        rc = lib.gpmi_hermite_basis(h, B.vec(x), N, LR_M, _d(LR_SCALE), _d(LR_AMP), _d(LR_L), pP, ldp, pdP, lddp)
        res = {"rc": rc, "Phi": P}
        if want_dl:
            res["dPhi_dl"] = dP
        return res
    return fn


def lowrank_logml_grad(want_grad):
    def fn(lib, h, B):
        x, y, _, _ = _lowrank_data()
        out = np.full(3, SENTINEL); g = np.full(3, SENTINEL)
        rc = lib.gpmi_lowrank_logml_grad(h, B.vec(x), N, B.vec(y), LR_M, _d(LR_SCALE), _d(LR_AMP), _d(LR_L), _d(SIGMA), _p(out),
                                         _p(g) if want_grad else None)
        res = {"rc": rc, "out": out}
        if want_grad:
            res["grad"] = g
        return res
    return fn


def lowrank_latent_lp_grad(want_q):
    """The NORMAL head on M replicate columns; want_q=False: the nullable q and qbar NULL."""
    def fn(lib, h, B):
        x, _, z, Y = _lowrank_data()
        pY, ldy = B.mat(Y)
        out = np.full(2, SENTINEL); zb = np.full(LR_M, SENTINEL); g = np.full(2, SENTINEL)
        q, qb = np.full(N, SENTINEL), np.full(N, SENTINEL)
        rc = lib.gpmi_lowrank_latent_lp_grad(h, B.vec(x), N, LR_M, _d(LR_SCALE), _d(LR_AMP), _d(LR_L), B.vec(z), NORMAL, pY, M, ldy,
                                             _d(0.7), _p(out), _p(q) if want_q else None, _p(qb) if want_q else None, _p(zb), _p(g))
        res = {"rc": rc, "out": out, "zbar": zb, "grad": g}
        if want_q:
            res.update(q=q, qbar=qb)
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
    # the factorisation alone, the joint [y; y'] model, the joint posteriors, one draw, the sampler's sweep, the Hermite table
    ("potrf-one", {}, potrf(N)),
    ("potrf-chain", {"small_m": 0}, potrf(N)),
    ("joint_logml-one", {}, joint_logml(N, False)),
    ("joint_logml-chain", {"small_m": 0}, joint_logml(N, False)),
    ("joint_logml_grad-one", {}, joint_logml(N, True)),
    ("joint_logml_grad-chain", {"small_ng1": 0, "small_m": 0}, joint_logml(N, True)),
    ("gp_predict_joint-one", {}, gp_predict_joint()),
    ("gp_predict_joint-chain", {"small_pj": 0}, gp_predict_joint()),
    ("joint_predict-one", {}, joint_predict(N, M)),
    ("joint_predict-chain", {"small_jp": 0}, joint_predict(N, M)),
    ("sample_derivs-one", {}, sample_derivs(N, M)),
    ("sample_derivs-chain", {"small_sd": 0}, sample_derivs(N, M)),
    ("seq_marginals-n21-m41", {}, seq_marginals()),
    # 16 + 16 + 9 rows of Xs.  On its own context this case is also the regression test of gpmi_seq_create's scratch for the
    # inverse diagonal blocks (once sized for the n x n matrix: at n = 21 some 90 KiB were written past the end of a staging
    # buffer that no larger call had grown, and the SECOND sampler made on the context came out wrong)
    ("seq_marginals-n21-m41-chunks", {"predict_mb": 16}, seq_marginals()),
    ("interp_build-approx_Lz_grad-n37", {}, interp_build_Lz_grad(N)),
    ("interp_build-approx_Lz_grad-n300", {}, interp_build_Lz_grad(300)),
    # leave-one-out and the Hessian (one route each: the chain), the low-rank model (one launch chain whatever the size)
    ("logml_loo", {}, logml_loo(True)),
    ("logml_loo-nulls", {}, logml_loo(False)),
    ("logml_hess-nell1", {}, logml_hess(1)),
    ("logml_hess-nell2", {}, logml_hess(2)),
    ("logml_hess-nell2-nograd", {}, logml_hess(2, False)),
    ("hermite_basis", {}, hermite_basis(True)),
    ("hermite_basis-nodl", {}, hermite_basis(False)),
    ("lowrank_logml_grad", {}, lowrank_logml_grad(True)),
    ("lowrank_logml_grad-nograd", {}, lowrank_logml_grad(False)),
    ("lowrank_latent-normal", {}, lowrank_latent_lp_grad(True)),
    ("lowrank_latent-normal-noq", {}, lowrank_latent_lp_grad(False)),
]

# Every option that sends a call to the blocked factorisation and the launch chains, whatever its size
_CHAIN = {"small_m": 0, "small_n1": 0, "small_gc": 0, "small_pr": 0, "small_pj": 0, "small_jp": 0, "small_ng1": 0, "small_vjp": 0,
          "small_cen": 0, "small_sd": 0}


def _chain(**more):
    opts = dict(_CHAIN)
    opts.update(more)
    return opts


BLOCKED_CASES = (
    [("potrf-n%d-nbo%d" % (n, nbo), _chain(nb_outer=nbo), potrf(n)) for n in (257, 300, 511, 640) for nbo in (128, 256)]
    + [("logml-n%d" % n, _chain(), logml_at(n, SYNTH)) for n in (257, 300, 511)]
    + [
        ("logml_grid-G5-n300-lanes", _chain(), logml_grid(False, 300, 5, SYNTH, synth_grid_pars)),
        ("logml_grad-n300-aug", _chain(), logml_grad_at(300, SYNTH)),
        ("logml_grad-n300-noaug", _chain(grad_aug_n=0), logml_grad_at(300, SYNTH)),
        ("gp_condition-n300-m259", _chain(), gp_condition_series(300, 259)),
        ("gp_predict-n300-m259", _chain(), gp_predict(True, 300, 259, SYNTH)),
        ("gp_predict_joint-n300-m259-B3", _chain(), gp_predict_joint(300, 259, 3, SYNTH)),
        ("joint_logml-n199", _chain(), joint_logml(199, False)),
        ("joint_logml_grad-n199", _chain(), joint_logml(199, True)),
        ("joint_predict-n199-m150", _chain(), joint_predict(199, 150)),
        ("sample_derivs-n301-m200", _chain(), sample_derivs(301, 200)),
        ("rbf_cov_chol-n300", _chain(), rbf_cov_chol(300)),
        ("interp_build-n150-P5", _chain(), interp_build_Lz_grad(150, 5)),
        ("exact_gp_f_vjp-chain-n300-k2", _chain(), exact_gp_f_vjp(True, 300, SYNTH)),
        ("latent-logsd-chain-n300-k2", _chain(), latent_gp_lp_grad(LOGSD, n=300, src=SYNTH)),
        ("centered-logsd-chain-n300-k2", _chain(), centered_gp_lp_grad(LOGSD, n=300, src=SYNTH)),
    ])


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
