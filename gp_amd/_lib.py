"""ctypes binding of libgpmi.so (include/gpmi.h) -- the only way this package computes.

There is no CPU fallback: if the shared library is missing or no gfx950 device is
visible, construction of a Context raises GpmiError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgpmi.so")
PROBES_LIB_PATH = os.path.join(_HERE, "csrc", "libgpmi_probes.so")

KINDS = ("QQ", "QR", "RQ", "RR", "QT", "TQ", "RT", "TR", "TT")
FULL, LOWER, COMPAT_RR = 0, 1, 2

# every symbol include/gpmi.h declares (checked by tests/test_abi.py)
SYMBOLS = (
    "gpmi_version", "gpmi_last_error", "gpmi_device_count", "gpmi_create", "gpmi_destroy",
    "gpmi_set_stream", "gpmi_reset_stream", "gpmi_sync", "gpmi_reserve", "gpmi_set_option",
    "gpmi_se_cov", "gpmi_se_cov_dev", "gpmi_deriv_cov", "gpmi_deriv_cov_dev", "gpmi_deriv_elem",
    "gpmi_joint_cov", "gpmi_potrf", "gpmi_potrf_dev", "gpmi_trmv_lower", "gpmi_trsv_lower", "gpmi_exact_gp_f",
    "gpmi_trmv_lower_t", "gpmi_exact_gp_f_vjp", "gpmi_exact_gp_f_vjp_dev", "gpmi_latent_gp_lp_grad", "gpmi_latent_gp_lp_grad_dev",
    "gpmi_centered_gp_lp_grad", "gpmi_centered_gp_lp_grad_dev",
    "gpmi_logml", "gpmi_logml_dev", "gpmi_logml_grid", "gpmi_logml_grid_dev", "gpmi_logml_grid_ard", "gpmi_logml_grid_ard_dev",
    "gpmi_joint_logml", "gpmi_joint_logml_dev", "gpmi_joint_logml_grid_dev", "gpmi_rbf_cov_chol", "gpmi_gp_condition", "gpmi_sample_derivs", "gpmi_sample_derivs_batch",
    "gpmi_interp_build", "gpmi_interp_load", "gpmi_approx_L", "gpmi_approx_Lz", "gpmi_approx_Lz_dev", "gpmi_approx_Lz_grad", "gpmi_approx_Lz_grad_dev",
    "gpmi_interp_free", "gpmi_logml_grad", "gpmi_logml_grad_grid",
    "gpmi_logml_grad_dev", "gpmi_logml_grad_grid_dev", "gpmi_logml_grad_grid_ard", "gpmi_logml_grad_grid_ard_dev",
    "gpmi_logml_loo", "gpmi_logml_loo_dev", "gpmi_logml_hess", "gpmi_logml_hess_dev",
    "gpmi_joint_logml_grad", "gpmi_joint_logml_grad_dev", "gpmi_joint_logml_grad_grid",
    "gpmi_approx_Lz_vjp", "gpmi_approx_Lz_vjp_dev", "gpmi_interp_gp_build", "gpmi_interp_gp_load", "gpmi_interp_gp_L",
    "gpmi_interp_gp_Lz", "gpmi_interp_gp_Lz_vjp", "gpmi_interp_gp_Lz_vjp_dev", "gpmi_interp_gp_free",
    "gpmi_seq_create", "gpmi_seq_step", "gpmi_seq_commit", "gpmi_seq_count", "gpmi_seq_destroy", "gpmi_seq_marginals",
    "gpmi_gp_predict", "gpmi_gp_predict_dev", "gpmi_gp_predict_joint", "gpmi_gp_predict_joint_dev",
    "gpmi_joint_predict", "gpmi_joint_predict_dev",
    "gpmi_hermite_basis", "gpmi_hermite_basis_dev", "gpmi_lowrank_logml_grad", "gpmi_lowrank_logml_grad_dev",
    "gpmi_lowrank_latent_lp_grad", "gpmi_lowrank_latent_lp_grad_dev",
    "gpmi_last_timing", "gpmi_kernel_timing", "gpmi_kernel_timing_ex", "gpmi_debug_fill", "gpmi_debug_counters",
)
# additionally exported by the probe build (libgpmi_probes.so, -DGPMI_PROBES; tools/ only)
PROBE_SYMBOLS = ("gpmi_probe_syrk", "gpmi_probe_mfma", "gpmi_probe_mfma_peak", "gpmi_probe_clock", "gpmi_probe_fused", "gpmi_probe_small", "gpmi_probe_body",
                 "gpmi_probe_tril_draws", "gpmi_probe_joint_star")


class GpmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libgpmi error %d: %s" % (code, msg))
        self.code = code


class NotPositiveDefinite(GpmiError):
    """info = k > 0: the leading minor of order k is not positive definite
    (base-R chol() error / Stan cholesky_decompose domain_error)."""

    def __init__(self, k):
        RuntimeError.__init__(self, "the leading minor of order %d is not positive definite" % k)
        self.code = k
        self.order = k


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so (same SONAME as ROCm's).  If libgpmi pulls in
    ROCm's copy first and torch is imported later, the process ends up with two HIP/HSA runtimes and
    torch finds no GPU.  When torch is installed but not yet loaded, map ITS runtime first so that
    both libraries share one; without torch (e.g. under R) libgpmi uses ROCm's as linked."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libgpmi.so; loud failure when it has not been built.  GPMI_USE_PROBES=1 (tools/ only)
    loads the probe build instead: same library plus the instruments and gpmi_probe_* entry points."""
    global _lib
    if _lib is not None:
        return _lib
    probes = os.environ.get("GPMI_USE_PROBES", "") == "1"
    path = PROBES_LIB_PATH if probes else LIB_PATH
    if not os.path.exists(path):
        raise GpmiError(-4, "%s not found: build it with `python -m gp_amd._build%s` "
                        "(hipcc --offload-arch=gfx950); gp_amd has no CPU fallback" % (path, " --probes" if probes else ""))
    _share_hip_runtime_with_torch()
    lib = C.CDLL(path)
    lib.gpmi_last_error.restype = C.c_char_p
    for name in SYMBOLS + (PROBE_SYMBOLS if probes else ()):
        fn = getattr(lib, name)
        if name != "gpmi_last_error":
            fn.restype = C.c_int
    lib.gpmi_debug_fill.argtypes = (C.c_void_p, C.c_int)
    lib.gpmi_debug_counters.argtypes = (C.c_void_p, C.POINTER(C.c_int))
    _lib = lib
    return lib


def _chk(rc, allow_info=False):
    if rc == 0:
        return 0
    if rc > 0:
        if allow_info:
            return rc
        raise NotPositiveDefinite(rc)
    raise GpmiError(rc, load().gpmi_last_error().decode())


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _d(x):
    return C.c_double(float(x))


def _vp(ptr):
    """a raw (device) address as a pointer argument; 0 / None: NULL"""
    return C.c_void_p(ptr) if ptr else None


def _vec(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())


def _mat(X):
    """2-D column-major float64 view/copy (R's native layout)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    return np.asfortranarray(X)


LIK_FAMILIES = {"normal": 0, "bernoulli_logit": 1, "normal_logsd": 2}   # GPMI_LIK_*
LIK_NONE = 3    # GPMI_LIK_NONE ("none"): no head, the prior part alone -- gpmi_centered_gp_lp_grad[_dev] only


def lik_family(family):
    """GPMI_LIK_* of a family name; integers pass through (the library rejects unknown ones)."""
    if isinstance(family, str):
        if family == "none":
            return LIK_NONE
        if family not in LIK_FAMILIES:
            raise GpmiError(-1, "unknown likelihood family %r" % (family,))
        return LIK_FAMILIES[family]
    return int(family)


def _kind(k):
    return KINDS.index(k) if isinstance(k, str) else int(k)


def device_count():
    n = C.c_int(0)
    rc = load().gpmi_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class Context:
    """One gpmi_ctx: bound to one GPU and to this process."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self._lib = load()
        _chk(self._lib.gpmi_create(C.byref(self._h), int(device)))
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gpmi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing -----------------------------------------------------------
    def set_stream(self, stream_handle):
        """Run on the caller's hipStream_t (handle 0 = the legacy null stream, torch's default
        stream); None goes back to the context's own stream."""
        if stream_handle is None:
            _chk(self._lib.gpmi_reset_stream(self._h))
        else:
            _chk(self._lib.gpmi_set_stream(self._h, C.c_void_p(int(stream_handle))))

    def sync(self):
        _chk(self._lib.gpmi_sync(self._h))

    def reserve(self, n_max):
        _chk(self._lib.gpmi_reserve(self._h, int(n_max)))

    def set_option(self, name, value):
        _chk(self._lib.gpmi_set_option(self._h, name.encode(), int(value)))

    def last_timing(self):
        out = np.zeros(3)
        _chk(self._lib.gpmi_last_timing(self._h, _p(out)))
        return out

    def kernel_timing(self, reset=True):
        """{category: (launches, total_ms, total_work)}: 'build' (bytes), 'syrk' and 'panel' (flops), 'syrk_multi_round'
        (the trailing-update launches of more than one round of tiles, a subset of 'syrk')."""
        out = np.zeros(12)
        _chk(self._lib.gpmi_kernel_timing_ex(self._h, int(bool(reset)), _p(out)))
        return {"build": tuple(out[0:3]), "syrk": tuple(out[3:6]), "panel": tuple(out[6:9]), "syrk_multi_round": tuple(out[9:12])}

    def debug_fill(self, byte):
        """Test hook: set every byte of the context's (and its lanes') floating-point scratch to `byte` (0..255), synchronised
        on both sides; counters, info words, the completion flag and the interpolation tables are left alone."""
        _chk(self._lib.gpmi_debug_fill(self._h, int(byte)))

    def debug_counters(self):
        """Number of non-zero device counters of the context and its lanes (0 between calls), read back with a copy."""
        n = C.c_int(-1)
        _chk(self._lib.gpmi_debug_counters(self._h, C.byref(n)))
        return n.value

    # ---- covariance builders (host buffers) ----------------------------------
    def se_cov(self, X, Y, alpha, ell, diag_add=0.0, flags=FULL):
        X = _mat(X)
        n, D = X.shape
        ell = _vec(ell)
        if Y is None:
            K = np.empty((n, n), order="F")
            _chk(self._lib.gpmi_se_cov(self._h, _p(X), n, max(n, 1), None, n, max(n, 1), D, _d(alpha), _p(ell),
                                       int(ell.size), _d(diag_add), int(flags), _p(K), max(n, 1)))
            return K
        Y = _mat(Y)
        if Y.shape[1] != D:
            raise GpmiError(-1, "X and Y must have the same number of columns")
        m = Y.shape[0]
        K = np.empty((n, m), order="F")
        _chk(self._lib.gpmi_se_cov(self._h, _p(X), n, max(n, 1), _p(Y), m, max(m, 1), D, _d(alpha), _p(ell),
                                   int(ell.size), _d(diag_add), int(flags), _p(K), max(n, 1)))
        return K

    def deriv_cov(self, kind, x, y, alpha, l, flags=FULL):
        x = _vec(x); y = _vec(y)
        K = np.empty((x.size, y.size), order="F")
        _chk(self._lib.gpmi_deriv_cov(self._h, _kind(kind), _p(x), int(x.size), _p(y), int(y.size), _d(alpha),
                                      _d(l), int(flags), _p(K), max(int(x.size), 1)))
        return K

    def deriv_elem(self, kind, tj, tk, l):
        tj, tk = np.broadcast_arrays(np.asarray(tj, dtype=np.float64), np.asarray(tk, dtype=np.float64))
        shape = tj.shape
        a = _vec(tj); b = _vec(tk)
        out = np.empty(a.size)
        _chk(self._lib.gpmi_deriv_elem(self._h, _kind(kind), _p(a), _p(b), C.c_size_t(a.size), _d(l), _p(out)))
        return out.reshape(shape)

    def joint_cov(self, t, alpha, l, sigma, jitter=1e-6, flags=FULL):
        t = _vec(t); n = t.size
        K = np.empty((2 * n, 2 * n), order="F")
        _chk(self._lib.gpmi_joint_cov(self._h, _p(t), n, _d(alpha), _d(l), _d(sigma), _d(jitter), int(flags),
                                      _p(K), max(2 * n, 1)))
        return K

    # ---- factorisation --------------------------------------------------------
    def potrf(self, A):
        """Lower Cholesky factor of A (copy); raises NotPositiveDefinite."""
        L = np.array(A, dtype=np.float64, order="F", copy=True)
        n = L.shape[0]
        if L.ndim != 2 or L.shape[1] != n:
            raise GpmiError(-1, "matrix must be square")
        _chk(self._lib.gpmi_potrf(self._h, _p(L), n, max(n, 1)))
        return L

    def trmv_lower(self, L, z):
        L = _mat(L); z = _vec(z); f = np.empty_like(z)
        _chk(self._lib.gpmi_trmv_lower(self._h, _p(L), L.shape[0], max(L.shape[0], 1), _p(z), _p(f)))
        return f

    def trmv_lower_t(self, L, u):
        """w = L^T u for lower-triangular L (the transpose of trmv_lower)."""
        L = _mat(L); u = _vec(u); w = np.empty_like(u)
        if L.shape[0] != u.size:
            raise GpmiError(-1, "L and u disagree on N")
        _chk(self._lib.gpmi_trmv_lower_t(self._h, _p(L), L.shape[0], max(L.shape[0], 1), _p(u), _p(w)))
        return w

    def trsv_lower(self, L, b):
        L = _mat(L); b = _vec(b); z = np.empty_like(b)
        _chk(self._lib.gpmi_trsv_lower(self._h, _p(L), L.shape[0], max(L.shape[0], 1), _p(b), _p(z)))
        return z

    def exact_gp_f(self, X, alpha, ell, z, jitter=1e-10):
        """f = chol(cov_exp_quad(X, alpha, ell) + jitter I) z (models/exact_gp.stan:17-25), fused on the device; raises
        NotPositiveDefinite."""
        X = _mat(X); z = _vec(z); ell = _vec(ell)
        n, D = X.shape
        if z.size != n:
            raise GpmiError(-1, "X and z disagree on N")
        f = np.empty(n)
        _chk(self._lib.gpmi_exact_gp_f(self._h, _p(X), n, n, D, _d(alpha), _p(ell), int(ell.size), _d(jitter), _p(z), _p(f)))
        return f

    def exact_gp_f_vjp(self, X, alpha, ell, Z, Fbar, jitter=1e-10):
        """(F, Zbar, grad) of F = chol(cov_exp_quad(X, alpha, ell) + jitter I) Z with upstream adjoint Fbar:
        Zbar = L^T Fbar, grad = (d/dalpha, d/dell...) of sum(Fbar * F).  Z and Fbar are 1-D (one column) or n x k;
        F and Zbar come back in the same shape.  Raises NotPositiveDefinite."""
        X = _mat(X); ell = _vec(ell)
        n, D = X.shape
        one = np.ndim(Z) == 1
        Zm = _mat(Z); Fb = _mat(Fbar)
        if Zm.shape[0] != n or Fb.shape != Zm.shape:
            raise GpmiError(-1, "X, Z and Fbar disagree on the shape")
        k = Zm.shape[1]
        F = np.empty((n, k), order="F"); Zb = np.empty((n, k), order="F"); g = np.empty(1 + ell.size)
        ld = max(n, 1)
        _chk(self._lib.gpmi_exact_gp_f_vjp(self._h, _p(X), n, ld, D, _d(alpha), _p(ell), int(ell.size), _d(jitter), _p(Zm), k, ld,
                                           _p(Fb), ld, _p(F), ld, _p(Zb), ld, _p(g)))
        if one:
            return F[:, 0], Zb[:, 0], g
        return F, Zb, g

    def latent_gp_lp_grad(self, X, alpha, ell, Z, family, Y, sigma=None, jitter=1e-10, want_f=True, want_fbar=False,
                          raise_not_pd=True):
        """The likelihood part of a latent exact-GP model's lp__ and its gradient with one factorisation
        (gpmi_latent_gp_lp_grad): F = chol(cov_exp_quad(X, alpha, ell) + jitter I) Z, the head `family` ("normal",
        "bernoulli_logit", "normal_logsd") on F against the columns of Y (n or n x m), Fbar = d lik / d F, Zbar = L^T Fbar and
        grad = (d/dalpha, d/dell...) of lik.  Returns a dict: lik, dlik_dsigma, F, Fbar (None unless asked for), Zbar, grad,
        info.  Z is 1-D or n x 1 (n x 2 for "normal_logsd"); F, Fbar and Zbar come back in Z's shape.  sigma is required by
        "normal" alone.  Not positive definite: raises NotPositiveDefinite, or with raise_not_pd=False returns the NaN outputs
        and info = the minor's order."""
        X = _mat(X); ell = _vec(ell)
        n, D = X.shape
        one = np.ndim(Z) == 1
        Zm = _mat(Z); Ym = _mat(Y)
        if Zm.shape[0] != n or Ym.shape[0] != n:
            raise GpmiError(-1, "X, Z and Y disagree on N")
        k = Zm.shape[1]; m = Ym.shape[1]
        fam = lik_family(family)
        if fam == LIK_FAMILIES["normal"] and sigma is None:
            raise GpmiError(-1, "the normal head needs sigma")
        F = np.empty((n, k), order="F") if want_f else None
        Fb = np.empty((n, k), order="F") if want_fbar else None
        Zb = np.empty((n, k), order="F"); g = np.empty(1 + ell.size); out = np.empty(2)
        ld = max(n, 1)
        info = _chk(self._lib.gpmi_latent_gp_lp_grad(self._h, _p(X), n, ld, D, _d(alpha), _p(ell), int(ell.size), _d(jitter), _p(Zm), k,
                                                     ld, fam, _p(Ym), m, ld, _d(0.0 if sigma is None else sigma), _p(out),
                                                     _p(F) if want_f else None, ld, _p(Fb) if want_fbar else None, ld, _p(Zb), ld,
                                                     _p(g)), allow_info=not raise_not_pd)
        sq = (lambda A: None if A is None else (A[:, 0] if one else A))
        return {"lik": float(out[0]), "dlik_dsigma": float(out[1]), "F": sq(F), "Fbar": sq(Fb), "Zbar": sq(Zb), "grad": g,
                "info": int(info)}

    # ---- low-rank (Hermite-eigenfunction) GP ------------------------------------------------------------------------------
    def hermite_basis(self, x, M, scale, amp, l, want_dl=False):
        """approx_L(M, scale, x, amp, l) of models/westbrook.stan:2-30 (gpmi_hermite_basis): Phi (n x M) with Phi Phi^T ->
        amp^2 exp(-(x_i - x_j)^2 / (2 l^2)) as M grows; with want_dl also dPhi / dl.  x is 1-D."""
        x = _vec(x)
        n = x.size
        Phi = np.empty((n, int(M)), order="F")
        dPhi = np.empty((n, int(M)), order="F") if want_dl else None
        ld = max(n, 1)
        _chk(self._lib.gpmi_hermite_basis(self._h, _p(x), n, int(M), _d(scale), _d(amp), _d(l), _p(Phi), ld,
                                          _p(dPhi) if want_dl else None, ld))
        return (Phi, dPhi) if want_dl else Phi

    def lowrank_logml_grad(self, x, y, M, scale, amp, l, sigma, want_grad=True, raise_not_pd=True):
        """Log marginal likelihood of y ~ N(0, Phi Phi^T + sigma^2 I), Phi = hermite_basis(x, M, scale, amp, l), and its gradient
        in (amp, l, sigma) (gpmi_lowrank_logml_grad).  Returns (out3, grad, info): out3 laid out as logml's.  A not positive
        definite: raises NotPositiveDefinite, or with raise_not_pd=False returns the NaN outputs and info = the order."""
        x = _vec(x); y = _vec(y)
        if x.size != y.size:
            raise GpmiError(-1, "x and y disagree on N")
        out3 = np.empty(3)
        g = np.empty(3) if want_grad else None
        info = _chk(self._lib.gpmi_lowrank_logml_grad(self._h, _p(x), int(x.size), _p(y), int(M), _d(scale), _d(amp), _d(l), _d(sigma),
                                                      _p(out3), _p(g) if want_grad else None), allow_info=not raise_not_pd)
        return out3, g, int(info)

    def lowrank_latent_lp_grad(self, x, M, scale, amp, l, z, family, Y, sigma=None, want_q=True, want_qbar=False):
        """The likelihood part of a low-rank latent model's lp__ and its gradient (gpmi_lowrank_latent_lp_grad): q = Phi z, the
        head `family` ("normal", "bernoulli_logit") on q against the columns of Y (n or n x m).  Returns a dict: lik,
        dlik_dsigma, q, qbar (None unless asked for), zbar = Phi^T qbar, grad = (d lik / d amp, d lik / d l)."""
        x = _vec(x); z = _vec(z)
        n = x.size
        Ym = _mat(Y)
        if Ym.shape[0] != n or z.size != int(M):
            raise GpmiError(-1, "x, z and Y disagree on N or M")
        fam = lik_family(family)
        if fam == LIK_FAMILIES["normal"] and sigma is None:
            raise GpmiError(-1, "the normal head needs sigma")
        out = np.empty(2); g = np.empty(2); zb = np.empty(int(M))
        q = np.empty(n) if want_q else None
        qb = np.empty(n) if want_qbar else None
        _chk(self._lib.gpmi_lowrank_latent_lp_grad(self._h, _p(x), n, int(M), _d(scale), _d(amp), _d(l), _p(z), fam, _p(Ym),
                                                   int(Ym.shape[1]), max(n, 1), _d(0.0 if sigma is None else sigma), _p(out),
                                                   _p(q) if want_q else None, _p(qb) if want_qbar else None, _p(zb), _p(g)))
        return {"lik": float(out[0]), "dlik_dsigma": float(out[1]), "q": q, "qbar": qb, "zbar": zb, "grad": g}

    def centered_gp_lp_grad(self, X, alpha, ell, F, family, Y=None, sigma=None, jitter=1e-9, raise_not_pd=True):
        """The centred latent GP's log-density and gradient with one factorisation (gpmi_centered_gp_lp_grad): the columns of F
        (n or n x k) are parameters with the prior multi_normal_cholesky(0, chol(cov_exp_quad(X, alpha, ell) + jitter I)), and the
        head `family` ("normal", "bernoulli_logit", "normal_logsd", or "none": the prior alone, any k) is evaluated on F against
        the columns of Y (n or n x m).  Returns a dict: lp = prior + lik, prior = -quad / 2 - k sum_log_diag, lik, dlik_dsigma,
        sum_log_diag, quad = sum_c f_c' Sigma^-1 f_c, Fgrad = d lp / d F (in F's shape), grad = (d/dalpha, d/dell...) of the prior,
        info.  Not positive definite: raises NotPositiveDefinite, or with raise_not_pd=False returns the NaN outputs and info =
        the minor's order."""
        X = _mat(X); ell = _vec(ell)
        n, D = X.shape
        one = np.ndim(F) == 1
        Fm = _mat(F)
        fam = lik_family(family)
        none = fam == LIK_NONE
        if not none and Y is None:
            raise GpmiError(-1, "the %s head needs Y" % family)
        Ym = None if none else _mat(Y)
        if Fm.shape[0] != n or (Ym is not None and Ym.shape[0] != n):
            raise GpmiError(-1, "X, F and Y disagree on N")
        k = Fm.shape[1]; m = 0 if none else Ym.shape[1]
        if fam == LIK_FAMILIES["normal"] and sigma is None:
            raise GpmiError(-1, "the normal head needs sigma")
        Fg = np.empty((n, k), order="F"); g = np.empty(1 + ell.size); out = np.empty(4)
        ld = max(n, 1)
        info = _chk(self._lib.gpmi_centered_gp_lp_grad(self._h, _p(X), n, ld, D, _d(alpha), _p(ell), int(ell.size), _d(jitter), _p(Fm),
                                                       k, ld, fam, None if none else _p(Ym), m, ld, _d(0.0 if sigma is None else sigma),
                                                       _p(out), _p(Fg), ld, _p(g)), allow_info=not raise_not_pd)
        prior = -0.5 * out[3] - k * out[2]
        return {"lp": float(out[0]), "prior": float(prior), "lik": float(out[0] - prior), "dlik_dsigma": float(out[1]),
                "sum_log_diag": float(out[2]), "quad": float(out[3]), "Fgrad": Fg[:, 0] if one else Fg, "grad": g, "info": int(info)}

    # ---- marginal likelihood -------------------------------------------------
    def logml(self, X, y, alpha, ell, sigma, jitter=0.0):
        """(logml, sum log L_ii, z'z); raises NotPositiveDefinite."""
        X = _mat(X); y = _vec(y); ell = _vec(ell)
        n, D = X.shape
        if y.size != n:
            raise GpmiError(-1, "X and y disagree on N")
        out = np.empty(3)
        _chk(self._lib.gpmi_logml(self._h, _p(X), n, n, D, _p(y), _d(alpha), _p(ell), int(ell.size), _d(sigma),
                                  _d(jitter), _p(out)))
        return out[0], out[1], out[2]

    def logml_grid(self, X, y, alpha, rho, sigma, jitter=0.0):
        """Arrays (G,3) of (logml, sum log L_ii, z'z) and info (G,) for G hyper-parameter points."""
        X = _mat(X); y = _vec(y)
        n, D = X.shape
        alpha, rho, sigma = np.broadcast_arrays(np.asarray(alpha, float), np.asarray(rho, float), np.asarray(sigma, float))
        a = _vec(alpha); r = _vec(rho); s = _vec(sigma)
        G = a.size
        out = np.empty((G, 3)); info = np.zeros(G, dtype=np.int32)
        _chk(self._lib.gpmi_logml_grid(self._h, _p(X), n, n, D, _p(y), _p(a), _p(r), _p(s), G, _d(jitter), _p(out),
                                       _p(info)))
        return out, info

    def logml_grid_ard(self, X, y, alpha, ell, sigma, jitter=0.0):
        """ARD grid: ell is (G, D), one length-scale per dimension and point; returns (G, 3), info (G,)."""
        X = _mat(X); y = _vec(y)
        n, D = X.shape
        E = np.ascontiguousarray(np.asarray(ell, dtype=np.float64).reshape(-1, D))
        G = E.shape[0]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, float), (G,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, float), (G,)))
        out = np.empty((G, 3)); info = np.zeros(G, dtype=np.int32)
        _chk(self._lib.gpmi_logml_grid_ard(self._h, _p(X), n, n, D, _p(y), _p(a), _p(E), _p(s), G, _d(jitter), _p(out),
                                           _p(info)))
        return out, info

    def joint_logml(self, t, yy, alpha, l, sigma, jitter=1e-6):
        t = _vec(t); yy = _vec(yy)
        if yy.size != 2 * t.size:
            raise GpmiError(-1, "yy must stack [y; y'] (length 2N)")
        out = np.empty(3)
        _chk(self._lib.gpmi_joint_logml(self._h, _p(t), int(t.size), _p(yy), _d(alpha), _d(l), _d(sigma),
                                        _d(jitter), _p(out)))
        return out[0], out[1], out[2]

    def rbf_cov_chol(self, x, l):
        x = _vec(x); n = x.size
        L = np.empty((n, n), order="F"); dL = np.empty((n, n), order="F")
        _chk(self._lib.gpmi_rbf_cov_chol(self._h, _p(x), n, _d(l), _p(L), max(n, 1), _p(dL), max(n, 1)))
        return L, dL

    def logml_grad(self, X, y, alpha, ell, sigma, jitter=0.0):
        """((logml, sum log L_ii, z'z), grad) with grad = (d/dalpha, d/dell..., d/dsigma)."""
        X = _mat(X); y = _vec(y); ell = _vec(ell)
        n, D = X.shape
        if y.size != n:
            raise GpmiError(-1, "X and y disagree on N")
        out = np.empty(3); g = np.empty(2 + ell.size)
        _chk(self._lib.gpmi_logml_grad(self._h, _p(X), n, max(n, 1), D, _p(y), _d(alpha), _p(ell), ell.size, _d(sigma),
                                       _d(jitter), _p(out), _p(g)))
        return out, g

    def logml_loo(self, X, y, alpha, ell, sigma, jitter=0.0, want_grad=True, outputs=("mu", "var", "lpd")):
        """Exact leave-one-out cross-validation (gpmi_logml_loo): a dict of out3 (3,), loo (sum_i lpd_i), mu, var, lpd (n each:
        mean, variance -- of the observation, noise included -- and log density of y_i given all the others), grad
        (d loo / d(alpha, ell.., sigma); None without want_grad) and info (k > 0: not positive definite, every LOO output NaN;
        nothing is raised for that status).  outputs: which of mu, var, lpd to compute (the others are None)."""
        X = _mat(X); y = _vec(y); ell = _vec(ell)
        n, D = X.shape
        if y.size != n:
            raise GpmiError(-1, "X and y disagree on N")
        out = np.empty(3); loo = np.empty(1)
        vec = {k: (np.empty(n) if k in outputs else None) for k in ("mu", "var", "lpd")}
        g = np.empty(2 + ell.size) if want_grad else None
        opt = lambda a: None if a is None else _p(a)
        info = _chk(self._lib.gpmi_logml_loo(self._h, _p(X), n, max(n, 1), D, _p(y), _d(alpha), _p(ell), ell.size, _d(sigma),
                                             _d(jitter), _p(out), _p(loo), opt(vec["mu"]), opt(vec["var"]), opt(vec["lpd"]), opt(g)),
                    allow_info=True)
        return {"out3": out, "loo": float(loo[0]), "mu": vec["mu"], "var": vec["var"], "lpd": vec["lpd"], "grad": g, "info": info}

    def logml_hess(self, X, y, alpha, ell, sigma, jitter=0.0, want_grad=True):
        """Value, gradient and exact Hessian of the log marginal likelihood in theta = (alpha, ell.., sigma) (gpmi_logml_hess): a
        dict of out3 (3,), grad (q = 2 + len(ell); None without want_grad), hess (q x q, symmetric, natural parameters) and info
        (k > 0: not positive definite, grad and hess all NaN; nothing is raised for that status).  One length-scale for any D, or
        one per dimension up to D = 8."""
        X = _mat(X); y = _vec(y); ell = _vec(ell)
        n, D = X.shape
        if y.size != n:
            raise GpmiError(-1, "X and y disagree on N")
        q = 2 + ell.size
        out = np.empty(3); H = np.empty((q, q), order="F")
        g = np.empty(q) if want_grad else None
        info = _chk(self._lib.gpmi_logml_hess(self._h, _p(X), n, max(n, 1), D, _p(y), _d(alpha), _p(ell), ell.size, _d(sigma),
                                              _d(jitter), _p(out), None if g is None else _p(g), _p(H), q), allow_info=True)
        return {"out3": out, "grad": g, "hess": H, "info": info}

    def logml_grad_grid(self, X, y, alpha, rho, sigma, jitter=0.0):
        """(out (G, 3), grad (G, 3), info (G,)): value and (d/dalpha, d/drho, d/dsigma) at G points, on the lanes."""
        X = _mat(X); y = _vec(y)
        n, D = X.shape
        alpha, rho, sigma = np.broadcast_arrays(np.asarray(alpha, float), np.asarray(rho, float), np.asarray(sigma, float))
        a = _vec(alpha); r = _vec(rho); s = _vec(sigma)
        G = a.size
        out = np.empty((G, 3)); g = np.empty((G, 3)); info = np.zeros(G, dtype=np.int32)
        _chk(self._lib.gpmi_logml_grad_grid(self._h, _p(X), n, max(n, 1), D, _p(y), _p(a), _p(r), _p(s), G, _d(jitter),
                                            _p(out), _p(g), _p(info)))
        return out, g, info

    def logml_grad_grid_ard(self, X, y, alpha, ell, sigma, jitter=0.0):
        """(out (G, 3), grad (G, D + 2), info (G,)): value and (d/dalpha, d/dell_0 .. d/dell_{D-1}, d/dsigma) at G points with
        one length-scale per dimension each (ell: (G, D)); alpha and sigma broadcast as in logml_grid_ard."""
        X = _mat(X); y = _vec(y)
        n, D = X.shape
        if y.size != n:
            raise GpmiError(-1, "X and y disagree on N")
        E = np.ascontiguousarray(np.asarray(ell, dtype=np.float64).reshape(-1, D))
        G = E.shape[0]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, float), (G,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, float), (G,)))
        out = np.empty((G, 3)); g = np.empty((G, D + 2)); info = np.zeros(G, dtype=np.int32)
        _chk(self._lib.gpmi_logml_grad_grid_ard(self._h, _p(X), n, max(n, 1), D, _p(y), _p(a), _p(E), _p(s), G, _d(jitter),
                                                _p(out), _p(g), _p(info)))
        return out, g, info

    def joint_logml_grad(self, t, yy, alpha, l, sigma, jitter=1e-6):
        """((logml, sum log L_ii, z'z), grad) of the joint [y; y'] model, grad = (d/dalpha, d/dl, d/dsigma) of logml;
        raises NotPositiveDefinite."""
        t = _vec(t); yy = _vec(yy)
        if yy.size != 2 * t.size:
            raise GpmiError(-1, "yy must stack [y; y'] (length 2N)")
        out = np.empty(3); g = np.empty(3)
        _chk(self._lib.gpmi_joint_logml_grad(self._h, _p(t), int(t.size), _p(yy), _d(alpha), _d(l), _d(sigma), _d(jitter),
                                             _p(out), _p(g)))
        return out, g

    def joint_logml_grad_grid(self, t, yy, alpha, l, sigma, jitter=1e-6):
        """(out (G, 3), grad (G, 3), info (G,)): joint_logml_grad at G points (alpha, l, sigma) on the same data, on the lanes;
        a point that is not positive definite has info > 0 and a NaN gradient."""
        t = _vec(t); yy = _vec(yy)
        if yy.size != 2 * t.size:
            raise GpmiError(-1, "yy must stack [y; y'] (length 2N)")
        alpha, l, sigma = np.broadcast_arrays(np.asarray(alpha, float), np.asarray(l, float), np.asarray(sigma, float))
        a = _vec(alpha); r = _vec(l); s = _vec(sigma)
        G = a.size
        out = np.empty((G, 3)); g = np.empty((G, 3)); info = np.zeros(G, dtype=np.int32)
        _chk(self._lib.gpmi_joint_logml_grad_grid(self._h, _p(t), int(t.size), _p(yy), _p(a), _p(r), _p(s), G, _d(jitter),
                                                  _p(out), _p(g), _p(info)))
        return out, g, info

    # ---- Cholesky-factor interpolation over the length-scale ------------------
    def interp_build(self, x, lp):
        """Table of L(lp[p]), dL/dl(lp[p]) built and kept on the device (test_interpolate.R:9-19)."""
        x = _vec(x); lp = _vec(lp)
        _chk(self._lib.gpmi_interp_build(self._h, _p(x), x.size, _p(lp), lp.size))
        self._itp_n = x.size

    def interp_load(self, lp, Ls, dLdls):
        """Upload a caller-supplied table: sequences of P n x n matrices."""
        lp = _vec(lp)
        n = np.asarray(Ls[0]).shape[0]
        A = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(a, dtype=np.float64)).ravel(order="F") for a in Ls]))
        B = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(a, dtype=np.float64)).ravel(order="F") for a in dLdls]))
        if A.shape != (lp.size, n * n) or B.shape != A.shape:
            raise GpmiError(-1, "lp, Ls and dLdls disagree on the table shape")
        _chk(self._lib.gpmi_interp_load(self._h, _p(lp), lp.size, _p(A), _p(B), n, n))
        self._itp_n = n

    def approx_L(self, l):
        n = getattr(self, "_itp_n", 0)
        out = np.empty((n, n), order="F")
        _chk(self._lib.gpmi_approx_L(self._h, _d(l), _p(out), max(n, 1)))
        return out

    def approx_Lz(self, l, z):
        z = _vec(z)
        if z.size != getattr(self, "_itp_n", -1):
            raise GpmiError(-1, "z must have the table's order")
        f = np.empty(z.size)
        _chk(self._lib.gpmi_approx_Lz(self._h, _d(l), _p(z), _p(f)))
        return f

    def approx_Lz_grad(self, l, z):
        """(f, dfdl): approx_L(l) z and its partial in l (the `var` overload of build_output,
        models/cubic_interpolated_gp.hpp:6-32)."""
        z = _vec(z)
        if z.size != getattr(self, "_itp_n", -1):
            raise GpmiError(-1, "z must have the table's order")
        f = np.empty(z.size); g = np.empty(z.size)
        _chk(self._lib.gpmi_approx_Lz_grad(self._h, _d(l), _p(z), _p(f), _p(g)))
        return f, g

    def approx_Lz_grad_dev(self, l, dz_ptr, df_ptr, dg_ptr):
        _chk(self._lib.gpmi_approx_Lz_grad_dev(self._h, _d(l), C.c_void_p(dz_ptr), C.c_void_p(df_ptr), C.c_void_p(dg_ptr)))

    def approx_Lz_dev(self, l, dz_ptr, df_ptr):
        _chk(self._lib.gpmi_approx_Lz_dev(self._h, _d(l), C.c_void_p(dz_ptr), C.c_void_p(df_ptr)))

    def interp_free(self):
        _chk(self._lib.gpmi_interp_free(self._h))
        self._itp_n = 0

    # ---- reverse mode of the interpolated models ------------------------------
    def _tri_vjp(self, fn, n, l, Z, Fbar, want_f):
        one = np.ndim(Z) == 1
        Zm = _mat(Z); Fb = _mat(Fbar)
        if Zm.shape[0] != n or Fb.shape != Zm.shape:
            raise GpmiError(-1, "Z and Fbar must be n x k with the table's n")
        k = Zm.shape[1]; ld = max(n, 1)
        F = np.empty((n, k), order="F") if want_f else None
        Zb = np.empty((n, k), order="F"); lb = np.empty(1)
        _chk(fn(self._h, _d(l), _p(Zm), k, ld, _p(Fb), ld, _p(F) if want_f else None, ld, _p(Zb), ld, _p(lb)))
        if one:
            F = F[:, 0] if want_f else None
            Zb = Zb[:, 0]
        return F, Zb, float(lb[0])

    def approx_Lz_vjp(self, l, Z, Fbar, want_f=True):
        """(F, Zbar, lbar) of F = approx_L(l) Z with upstream adjoint Fbar (models/cubic_interpolated_gp.hpp:6-32,38-73 under
        reverse mode): Zbar = approx_L(l)^T Fbar, lbar = sum(Fbar * (dv/dl) Z).  Z and Fbar are 1-D (one column) or n x k;
        F (None when want_f is False) and Zbar come back in the same shape.  F is approx_Lz's, bit for bit."""
        return self._tri_vjp(self._lib.gpmi_approx_Lz_vjp, getattr(self, "_itp_n", 0), l, Z, Fbar, want_f)

    def approx_Lz_vjp_dev(self, l, dZ_ptr, k, ldz, dFbar_ptr, ldfb, dF_ptr, ldf, dZbar_ptr, ldzb, dlbar_ptr):
        """gpmi_approx_Lz_vjp_dev on device pointers (dF_ptr may be None); enqueued, not synchronised."""
        _chk(self._lib.gpmi_approx_Lz_vjp_dev(self._h, _d(l), C.c_void_p(dZ_ptr), int(k), int(ldz), C.c_void_p(dFbar_ptr),
                                              int(ldfb), C.c_void_p(dF_ptr) if dF_ptr else None, int(ldf),
                                              C.c_void_p(dZbar_ptr), int(ldzb), C.c_void_p(dlbar_ptr)))

    def interp_gp_build(self, x, lp, rho=1.0, jitter=1e-10):
        """lookup = (Sigma_P \\ exact)^T of models/interpolated_gp.stan:9-27, the P exact factors of x built on the device."""
        x = _vec(x); lp = _vec(lp)
        _chk(self._lib.gpmi_interp_gp_build(self._h, _p(x), x.size, _p(lp), lp.size, _d(rho), _d(jitter)))
        self._igp_n = x.size

    def interp_gp_load(self, lp, Ls, rho=1.0, jitter=1e-10):
        """The same table from caller-supplied exact factors (a sequence of P n x n matrices)."""
        lp = _vec(lp)
        n = np.asarray(Ls[0]).shape[0]
        A = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(a, dtype=np.float64)).ravel(order="F") for a in Ls]))
        if A.shape != (lp.size, n * n):
            raise GpmiError(-1, "lp and Ls disagree on the table shape")
        _chk(self._lib.gpmi_interp_gp_load(self._h, _p(lp), lp.size, _d(rho), _d(jitter), _p(A), n, n))
        self._igp_n = n

    def interp_gp_L(self, l):
        """L(l) = to_matrix(lookup * Kp(l), N, N) (interpolated_gp.stan:40-42), lower triangular."""
        n = getattr(self, "_igp_n", 0)
        out = np.empty((n, n), order="F")
        _chk(self._lib.gpmi_interp_gp_L(self._h, _d(l), _p(out), max(n, 1)))
        return out

    def interp_gp_Lz(self, l, Z):
        """F = L(l) Z (interpolated_gp.stan:44); Z 1-D or n x k."""
        n = getattr(self, "_igp_n", 0)
        one = np.ndim(Z) == 1
        Zm = _mat(Z)
        if Zm.shape[0] != n:
            raise GpmiError(-1, "Z must have the table's n rows")
        k = Zm.shape[1]; ld = max(n, 1)
        F = np.empty((n, k), order="F")
        _chk(self._lib.gpmi_interp_gp_Lz(self._h, _d(l), _p(Zm), k, ld, _p(F), ld))
        return F[:, 0] if one else F

    def interp_gp_Lz_vjp(self, l, Z, Fbar, want_f=True):
        """(F, Zbar, lbar) of F = L(l) Z with upstream adjoint Fbar: Zbar = L(l)^T Fbar, lbar = sum(Fbar * (dL/dl) Z)."""
        return self._tri_vjp(self._lib.gpmi_interp_gp_Lz_vjp, getattr(self, "_igp_n", 0), l, Z, Fbar, want_f)

    def interp_gp_Lz_vjp_dev(self, l, dZ_ptr, k, ldz, dFbar_ptr, ldfb, dF_ptr, ldf, dZbar_ptr, ldzb, dlbar_ptr):
        """gpmi_interp_gp_Lz_vjp_dev on device pointers (dF_ptr may be None); enqueued, not synchronised."""
        _chk(self._lib.gpmi_interp_gp_Lz_vjp_dev(self._h, _d(l), C.c_void_p(dZ_ptr), int(k), int(ldz), C.c_void_p(dFbar_ptr),
                                                 int(ldfb), C.c_void_p(dF_ptr) if dF_ptr else None, int(ldf),
                                                 C.c_void_p(dZbar_ptr), int(ldzb), C.c_void_p(dlbar_ptr)))

    def interp_gp_free(self):
        _chk(self._lib.gpmi_interp_gp_free(self._h))
        self._igp_n = 0

    def gp_condition(self, t, ts, y, alpha, l, s2, jitter, kindK, kindS, kindSS, flags=FULL):
        t = _vec(t); ts = _vec(ts); y = _vec(y)
        n, m = t.size, ts.size
        mn = np.empty(m); Kn = np.empty((m, m), order="F")
        _chk(self._lib.gpmi_gp_condition(self._h, _p(t), n, _p(ts), m, _p(y), _d(alpha), _d(l), _d(s2), _d(jitter),
                                         _kind(kindK), _kind(kindS), _kind(kindSS), int(flags), _p(mn), _p(Kn),
                                         max(m, 1)))
        return mn, Kn

    def gp_predict(self, X, y, alpha, ell, sigma, jitter, Xs, want_var=True):
        """Pointwise posterior of the latent function at the rows of Xs (m x D) given (X, y) under the ARD squared-exponential
        model of logml: {"mean" (m,), "var" (m,) or None, "info"}.  var is alpha^2 - k^T Sigma^-1 k as computed (not clamped, no
        sigma^2); info = k > 0: Sigma is not positive definite at order k (mean, var all NaN)."""
        X = _mat(X); y = _vec(y); ell = _vec(ell); Xs = _mat(Xs)
        n, D = X.shape
        m = Xs.shape[0]
        if y.size != n or Xs.shape[1] != D:
            raise GpmiError(-1, "X, y and Xs disagree on N or D")
        mean = np.empty(m); var = np.empty(m) if want_var else None
        info = _chk(self._lib.gpmi_gp_predict(self._h, _p(X), n, max(n, 1), D, _p(y), _d(alpha), _p(ell), int(ell.size), _d(sigma),
                                              _d(jitter), _p(Xs), m, max(m, 1), _p(mean), _p(var) if want_var else None),
                    allow_info=True)
        return {"mean": mean, "var": var, "info": int(info)}

    def gp_predict_joint(self, X, y, alpha, ell, sigma, jitter, Xs, post_jitter=0.0, Z=None, want_cov=True):
        """Joint posterior of the latent function at the rows of Xs (m x D) given (X, y) under the model of gp_predict:
        {"mean" (m,), "cov" (m, m) or None, "draws" (m, B) or None, "info"}.  cov = K(Xs, Xs) - Ks Sigma^-1 Ks^T + post_jitter I as
        computed (both triangles, bit-for-bit symmetric); draws[:, b] = mean + chol(cov) Z[:, b] for the caller's standard-normal
        Z (m, B).  info = k in 1..n: Sigma is not positive definite at order k (everything NaN); n + k: cov is not (draws NaN)."""
        X = _mat(X); y = _vec(y); ell = _vec(ell); Xs = _mat(Xs)
        n, D = X.shape
        m = Xs.shape[0]
        if y.size != n or Xs.shape[1] != D:
            raise GpmiError(-1, "X, y and Xs disagree on N or D")
        B = 0
        if Z is not None:
            Z = np.asarray(Z, dtype=np.float64)
            Z = np.asfortranarray(Z.reshape(m, -1) if Z.ndim != 2 else Z)
            if Z.shape[0] != m:
                raise GpmiError(-1, "Z must have one row per row of Xs")
            B = Z.shape[1]
        mean = np.empty(m)
        cov = np.empty((m, m), order="F") if want_cov else None
        draws = np.empty((m, B), order="F") if B else None
        info = _chk(self._lib.gpmi_gp_predict_joint(self._h, _p(X), n, max(n, 1), D, _p(y), _d(alpha), _p(ell), int(ell.size),
                                                    _d(sigma), _d(jitter), _p(Xs), m, max(m, 1), _d(post_jitter), _p(mean),
                                                    _p(cov) if want_cov else None, max(m, 1), _p(Z) if B else None, B, max(m, 1),
                                                    _p(draws) if B else None, max(m, 1)), allow_info=True)
        return {"mean": mean, "cov": cov, "draws": draws, "info": int(info)}

    def joint_predict(self, t, yy, alpha, l, sigma, jitter, ts, orders, post_jitter, Z=None, want_cov=True):
        """Posterior of f, f', f'' at the m times ts given yy = [y; y'] at the n times t under the joint model of joint_logml:
        {"mean" (p m,), "cov" (p m, p m) or None, "draws" (p m, B) or None, "info"}, stacked by derivative order (m rows each) for
        the p orders in the bit mask `orders` (1: f, 2: f', 4: f'').  cov = Kss - Ks S^-1 Ks^T + post_jitter[a] on the diagonal of
        block a (both triangles, bit-for-bit symmetric); draws[:, b] = mean + chol(cov) Z[:, b] for the caller's standard-normal
        Z (p m, B).  info = k in 1..2n: S is not positive definite at order k (everything NaN); 2n + k: cov is not (draws NaN)."""
        t = _vec(t); yy = _vec(yy); ts = _vec(ts); post_jitter = _vec(post_jitter)
        n, m, orders = t.size, ts.size, int(orders)
        p = bin(orders & 7).count("1") if 1 <= orders <= 7 else 1
        if yy.size != 2 * n:
            raise GpmiError(-1, "yy must hold 2 n values")
        if post_jitter.size != p:
            raise GpmiError(-1, "post_jitter must hold one value per requested order")
        pm = p * m
        B = 0
        if Z is not None:
            Z = np.asarray(Z, dtype=np.float64)
            Z = np.asfortranarray(Z.reshape(pm, -1) if Z.ndim != 2 else Z)
            if Z.shape[0] != pm:
                raise GpmiError(-1, "Z must have one row per requested order and time")
            B = Z.shape[1]
        mean = np.empty(pm)
        cov = np.empty((pm, pm), order="F") if want_cov else None
        draws = np.empty((pm, B), order="F") if B else None
        info = _chk(self._lib.gpmi_joint_predict(self._h, _p(t), n, _p(yy), _d(alpha), _d(l), _d(sigma), _d(jitter), _p(ts), m, orders,
                                                 _p(post_jitter), _p(mean), _p(cov) if want_cov else None, max(pm, 1),
                                                 _p(Z) if B else None, B, max(pm, 1), _p(draws) if B else None, max(pm, 1)),
                    allow_info=True)
        return {"mean": mean, "cov": cov, "draws": draws, "info": int(info)}

    def joint_predict_dev(self, dt_ptr, n, dyy_ptr, alpha, l, sigma, jitter, dts_ptr, m, orders, post_jitter, dmean_ptr, dcov_ptr, ldc,
                          dZ_ptr, B, ldz, ddraws_ptr, ldd, dinfo_ptr):
        """gpmi_joint_predict_dev on device pointers (post_jitter: host values, one per requested order; dcov_ptr may be None;
        dZ_ptr / ddraws_ptr may be None when B == 0); enqueued, not synchronised."""
        post_jitter = _vec(post_jitter)
        _chk(self._lib.gpmi_joint_predict_dev(self._h, C.c_void_p(dt_ptr), int(n), C.c_void_p(dyy_ptr), _d(alpha), _d(l), _d(sigma),
                                              _d(jitter), C.c_void_p(dts_ptr), int(m), int(orders), _p(post_jitter),
                                              C.c_void_p(dmean_ptr), _vp(dcov_ptr), int(ldc), _vp(dZ_ptr), int(B), int(ldz),
                                              _vp(ddraws_ptr), int(ldd), C.c_void_p(dinfo_ptr)))

    def sample_derivs(self, t, ts, y, l, a, sy, jitter, z):
        """(draw, mu): mu + chol(cov) z of sample_derivs (pendulum_fit.R:227-255), fused on the device."""
        t = _vec(t); ts = _vec(ts); y = _vec(y); z = _vec(z)
        if y.size != t.size or z.size != ts.size:
            raise GpmiError(-1, "y must match t and z must match ts")
        draw = np.empty(ts.size); mu = np.empty(ts.size)
        _chk(self._lib.gpmi_sample_derivs(self._h, _p(t), int(t.size), _p(ts), int(ts.size), _p(y), _d(l), _d(a), _d(sy),
                                          _d(jitter), _p(z), _p(draw), _p(mu)))
        return draw, mu

    def sample_derivs_batch(self, t, ts, Y, params, jitter, Z):
        """(draws (m, B), mus (m, B), info (B,)): B independent draws on the lanes; Y (n, B), params (B, 3) rows
        (l, a, sy), Z (m, B)."""
        t = _vec(t); ts = _vec(ts)
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64).reshape(t.size, -1))
        B = Y.shape[1]
        Z = np.asfortranarray(np.asarray(Z, dtype=np.float64).reshape(ts.size, -1))
        P = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, 3))
        if Z.shape[1] != B or P.shape[0] != B:
            raise GpmiError(-1, "Y, params and Z disagree on the batch size")
        draws = np.empty((ts.size, B), order="F"); mus = np.empty((ts.size, B), order="F"); info = np.zeros(B, dtype=np.int32)
        _chk(self._lib.gpmi_sample_derivs_batch(self._h, _p(t), int(t.size), _p(ts), int(ts.size), _p(Y), max(int(t.size), 1),
                                                _p(P), B, _d(jitter), _p(Z), max(int(ts.size), 1), _p(draws), max(int(ts.size), 1),
                                                _p(mus), max(int(ts.size), 1), _p(info)))
        return draws, mus, info

    def seq_sampler(self, X, mn, Kn, alpha, ell, jitter=1e-6, max_steps=256):
        """Sequential conditional sampler (create_p_dotXnS, R/ode_gp_library.R:43-93)."""
        return SeqSampler(self, X, mn, Kn, alpha, ell, jitter, max_steps)

    # ---- device-pointer API (torch tensors own the memory; plumbing only) -----
    def logml_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dout_ptr, dinfo_ptr):
        ell = _vec(ell)
        _chk(self._lib.gpmi_logml_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), C.c_void_p(dy_ptr),
                                      _d(alpha), _p(ell), int(ell.size), _d(sigma), _d(jitter),
                                      C.c_void_p(dout_ptr), C.c_void_p(dinfo_ptr)))

    def gp_predict_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dXs_ptr, m, ldxs, dmean_ptr, dvar_ptr, dinfo_ptr):
        """gpmi_gp_predict_dev on device pointers (dvar_ptr may be None: mean only); enqueued, not synchronised."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_gp_predict_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), C.c_void_p(dy_ptr), _d(alpha),
                                           _p(ell), int(ell.size), _d(sigma), _d(jitter), C.c_void_p(dXs_ptr), int(m), int(ldxs),
                                           C.c_void_p(dmean_ptr), C.c_void_p(dvar_ptr) if dvar_ptr else None,
                                           C.c_void_p(dinfo_ptr)))

    def gp_predict_joint_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dXs_ptr, m, ldxs, post_jitter, dmean_ptr,
                             dcov_ptr, ldc, dZ_ptr, B, ldz, ddraws_ptr, ldd, dinfo_ptr):
        """gpmi_gp_predict_joint_dev on device pointers (dcov_ptr may be None; dZ_ptr / ddraws_ptr may be None when B == 0);
        enqueued, not synchronised."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_gp_predict_joint_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), C.c_void_p(dy_ptr), _d(alpha),
                                                 _p(ell), int(ell.size), _d(sigma), _d(jitter), C.c_void_p(dXs_ptr), int(m), int(ldxs),
                                                 _d(post_jitter), C.c_void_p(dmean_ptr), _vp(dcov_ptr), int(ldc), _vp(dZ_ptr), int(B),
                                                 int(ldz), _vp(ddraws_ptr), int(ldd), C.c_void_p(dinfo_ptr)))

    def exact_gp_f_vjp_dev(self, dX_ptr, n, ldx, D, alpha, ell, jitter, dZ_ptr, k, ldz, dFbar_ptr, ldfb, dF_ptr, ldf, dZbar_ptr,
                           ldzb, dgrad_ptr, dinfo_ptr):
        """gpmi_exact_gp_f_vjp_dev on device pointers (dF_ptr may be None); enqueued, not synchronised."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_exact_gp_f_vjp_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), _d(alpha), _p(ell),
                                               int(ell.size), _d(jitter), C.c_void_p(dZ_ptr), int(k), int(ldz),
                                               C.c_void_p(dFbar_ptr), int(ldfb), C.c_void_p(dF_ptr) if dF_ptr else None, int(ldf),
                                               C.c_void_p(dZbar_ptr), int(ldzb), C.c_void_p(dgrad_ptr), C.c_void_p(dinfo_ptr)))

    def latent_gp_lp_grad_dev(self, dX_ptr, n, ldx, D, alpha, ell, jitter, dZ_ptr, k, ldz, family, dY_ptr, m, ldy, sigma, dout_ptr,
                              dF_ptr, ldf, dFbar_ptr, ldfb, dZbar_ptr, ldzb, dgrad_ptr, dinfo_ptr):
        """gpmi_latent_gp_lp_grad_dev on device pointers (dF_ptr and dFbar_ptr may be None); enqueued, not synchronised."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_latent_gp_lp_grad_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), _d(alpha), _p(ell),
                                                  int(ell.size), _d(jitter), C.c_void_p(dZ_ptr), int(k), int(ldz), lik_family(family),
                                                  C.c_void_p(dY_ptr), int(m), int(ldy), _d(0.0 if sigma is None else sigma),
                                                  C.c_void_p(dout_ptr), C.c_void_p(dF_ptr) if dF_ptr else None, int(ldf),
                                                  C.c_void_p(dFbar_ptr) if dFbar_ptr else None, int(ldfb), C.c_void_p(dZbar_ptr),
                                                  int(ldzb), C.c_void_p(dgrad_ptr), C.c_void_p(dinfo_ptr)))

    def hermite_basis_dev(self, dx_ptr, n, M, scale, amp, l, dPhi_ptr, ldp, ddPhi_ptr=None, lddp=0):
        """gpmi_hermite_basis_dev on device pointers (ddPhi_ptr may be None); enqueued, not synchronised."""
        _chk(self._lib.gpmi_hermite_basis_dev(self._h, _vp(dx_ptr), int(n), int(M), _d(scale), _d(amp), _d(l), _vp(dPhi_ptr), int(ldp),
                                              _vp(ddPhi_ptr), int(lddp)))

    def lowrank_logml_grad_dev(self, dx_ptr, n, dy_ptr, M, scale, amp, l, sigma, dout_ptr, dgrad_ptr, dinfo_ptr):
        """gpmi_lowrank_logml_grad_dev on device pointers: d_out3 (3), d_grad (3; may be None) and d_info (1 int) are written by the
        device (NaN and info = k when A is not positive definite); enqueued, not synchronised, nothing is raised for that status."""
        _chk(self._lib.gpmi_lowrank_logml_grad_dev(self._h, _vp(dx_ptr), int(n), _vp(dy_ptr), int(M), _d(scale), _d(amp), _d(l),
                                                   _d(sigma), _vp(dout_ptr), _vp(dgrad_ptr), _vp(dinfo_ptr)))

    def lowrank_latent_lp_grad_dev(self, dx_ptr, n, M, scale, amp, l, dz_ptr, family, dY_ptr, m, ldy, sigma, dout_ptr, dq_ptr, dqbar_ptr,
                                   dzbar_ptr, dgrad_ptr):
        """gpmi_lowrank_latent_lp_grad_dev on device pointers (dq_ptr and dqbar_ptr may be None); enqueued, not synchronised."""
        _chk(self._lib.gpmi_lowrank_latent_lp_grad_dev(self._h, _vp(dx_ptr), int(n), int(M), _d(scale), _d(amp), _d(l), _vp(dz_ptr),
                                                       lik_family(family), _vp(dY_ptr), int(m), int(ldy),
                                                       _d(0.0 if sigma is None else sigma), _vp(dout_ptr), _vp(dq_ptr), _vp(dqbar_ptr),
                                                       _vp(dzbar_ptr), _vp(dgrad_ptr)))

    def centered_gp_lp_grad_dev(self, dX_ptr, n, ldx, D, alpha, ell, jitter, dF_ptr, k, ldf, family, dY_ptr, m, ldy, sigma, dout_ptr,
                                dFgrad_ptr, ldfg, dgrad_ptr, dinfo_ptr):
        """gpmi_centered_gp_lp_grad_dev on device pointers (dY_ptr may be None with "none"; dout: 4 doubles); enqueued, not
        synchronised."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_centered_gp_lp_grad_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), _d(alpha), _p(ell),
                                                    int(ell.size), _d(jitter), C.c_void_p(dF_ptr), int(k), int(ldf), lik_family(family),
                                                    C.c_void_p(dY_ptr) if dY_ptr else None, int(m), int(ldy),
                                                    _d(0.0 if sigma is None else sigma), C.c_void_p(dout_ptr), C.c_void_p(dFgrad_ptr),
                                                    int(ldfg), C.c_void_p(dgrad_ptr), C.c_void_p(dinfo_ptr)))

    def logml_grid_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, rho, sigma, jitter, dout_ptr, dinfo_ptr):
        a = _vec(alpha); r = _vec(rho); s = _vec(sigma)
        _chk(self._lib.gpmi_logml_grid_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D),
                                           C.c_void_p(dy_ptr), _p(a), _p(r), _p(s), int(a.size), _d(jitter),
                                           C.c_void_p(dout_ptr), C.c_void_p(dinfo_ptr)))

    def logml_grid_ard_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dout_ptr, dinfo_ptr):
        E = np.ascontiguousarray(np.asarray(ell, dtype=np.float64).reshape(-1, int(D)))
        G = E.shape[0]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, float), (G,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, float), (G,)))
        _chk(self._lib.gpmi_logml_grid_ard_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx), int(D), C.c_void_p(dy_ptr),
                                               _p(a), _p(E), _p(s), G, _d(jitter), C.c_void_p(dout_ptr), C.c_void_p(dinfo_ptr)))

    def joint_logml_dev(self, dt_ptr, n, dyy_ptr, alpha, l, sigma, jitter, dout_ptr, dinfo_ptr):
        _chk(self._lib.gpmi_joint_logml_dev(self._h, C.c_void_p(dt_ptr), int(n), C.c_void_p(dyy_ptr), _d(alpha),
                                            _d(l), _d(sigma), _d(jitter), C.c_void_p(dout_ptr), C.c_void_p(dinfo_ptr)))

    def joint_logml_grad_dev(self, dt_ptr, n, dyy_ptr, alpha, l, sigma, jitter, dout_ptr, dgrad_ptr, dinfo_ptr):
        """Enqueued on the context's stream: d_out3 (3), d_grad (3) and d_info (1 int) are written by the device (NaN gradient and
        info = k when the matrix is not positive definite); nothing is raised for that status."""
        _chk(self._lib.gpmi_joint_logml_grad_dev(self._h, C.c_void_p(dt_ptr), int(n), C.c_void_p(dyy_ptr), _d(alpha), _d(l),
                                                 _d(sigma), _d(jitter), C.c_void_p(dout_ptr), C.c_void_p(dgrad_ptr),
                                                 C.c_void_p(dinfo_ptr)))

    def logml_grad_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dout_ptr, dgrad_ptr, dinfo_ptr):
        """gpmi_logml_grad_dev on device pointers: d_out3 (3), d_grad (2 + len(ell)) and d_info (1 int) are written by the device
        (NaN gradient and info = k when the matrix is not positive definite); enqueued, not synchronised, nothing is raised for
        that status."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_logml_grad_dev(self._h, _vp(dX_ptr), int(n), int(ldx), int(D), _vp(dy_ptr), _d(alpha), _p(ell),
                                           int(ell.size), _d(sigma), _d(jitter), _vp(dout_ptr), _vp(dgrad_ptr), _vp(dinfo_ptr)))

    def logml_loo_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dout_ptr, dloo_ptr, dmu_ptr, dvar_ptr, dlpd_ptr,
                      dgrad_ptr, dinfo_ptr):
        """gpmi_logml_loo_dev on device pointers: d_out3 (3), d_loo (1), d_mu, d_var, d_lpd (n each), d_grad (2 + len(ell)) and
        d_info (1 int) are written by the device (NaN LOO outputs and info = k when the matrix is not positive definite);
        d_mu, d_var, d_lpd, d_grad may be 0 / None.  Enqueued, not synchronised, nothing is raised for that status."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_logml_loo_dev(self._h, _vp(dX_ptr), int(n), int(ldx), int(D), _vp(dy_ptr), _d(alpha), _p(ell),
                                          int(ell.size), _d(sigma), _d(jitter), _vp(dout_ptr), _vp(dloo_ptr), _vp(dmu_ptr),
                                          _vp(dvar_ptr), _vp(dlpd_ptr), _vp(dgrad_ptr), _vp(dinfo_ptr)))

    def logml_hess_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dout_ptr, dgrad_ptr, dhess_ptr, ldh, dinfo_ptr):
        """gpmi_logml_hess_dev on device pointers: d_out3 (3), d_grad (2 + len(ell); may be 0 / None), d_hess (q x q, leading
        dimension ldh) and d_info (1 int) are written by the device (NaN grad and hess and info = k when the matrix is not positive
        definite).  Enqueued, not synchronised, nothing is raised for that status."""
        ell = _vec(ell)
        _chk(self._lib.gpmi_logml_hess_dev(self._h, _vp(dX_ptr), int(n), int(ldx), int(D), _vp(dy_ptr), _d(alpha), _p(ell),
                                           int(ell.size), _d(sigma), _d(jitter), _vp(dout_ptr), _vp(dgrad_ptr), _vp(dhess_ptr),
                                           int(ldh), _vp(dinfo_ptr)))

    def logml_grad_grid_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, rho, sigma, jitter, dout_ptr, dgrad_ptr, dinfo_ptr):
        """gpmi_logml_grad_grid_dev: d_out3 (3 G), d_grad (3 G), d_info (G ints); alpha, rho, sigma: host arrays of one length."""
        a = _vec(alpha); r = _vec(rho); s = _vec(sigma)
        if not (a.size == r.size == s.size):
            raise GpmiError(-1, "alpha, rho and sigma disagree on G")
        _chk(self._lib.gpmi_logml_grad_grid_dev(self._h, _vp(dX_ptr), int(n), int(ldx), int(D), _vp(dy_ptr), _p(a), _p(r), _p(s),
                                                int(a.size), _d(jitter), _vp(dout_ptr), _vp(dgrad_ptr), _vp(dinfo_ptr)))

    def logml_grad_grid_ard_dev(self, dX_ptr, n, ldx, D, dy_ptr, alpha, ell, sigma, jitter, dout_ptr, dgrad_ptr, dinfo_ptr):
        """gpmi_logml_grad_grid_ard_dev: ell (G, D); d_out3 (3 G), d_grad (G (D + 2), point-major), d_info (G ints)."""
        E = np.ascontiguousarray(np.asarray(ell, dtype=np.float64).reshape(-1, int(D)))
        G = E.shape[0]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, float), (G,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, float), (G,)))
        _chk(self._lib.gpmi_logml_grad_grid_ard_dev(self._h, _vp(dX_ptr), int(n), int(ldx), int(D), _vp(dy_ptr), _p(a), _p(E), _p(s),
                                                    G, _d(jitter), _vp(dout_ptr), _vp(dgrad_ptr), _vp(dinfo_ptr)))

    def joint_logml_grid_dev(self, dt_ptr, n, dyy_ptr, alpha, l, sigma, jitter, dout_ptr, dinfo_ptr):
        a = _vec(alpha); r = _vec(l); s = _vec(sigma)
        _chk(self._lib.gpmi_joint_logml_grid_dev(self._h, C.c_void_p(dt_ptr), int(n), C.c_void_p(dyy_ptr), _p(a), _p(r), _p(s),
                                                 int(a.size), _d(jitter), C.c_void_p(dout_ptr), C.c_void_p(dinfo_ptr)))

    def se_cov_dev(self, dX_ptr, n, ldx, dY_ptr, m, ldy, D, alpha, ell, diag_add, flags, dK_ptr, ldk):
        ell = _vec(ell)
        _chk(self._lib.gpmi_se_cov_dev(self._h, C.c_void_p(dX_ptr), int(n), int(ldx),
                                       C.c_void_p(dY_ptr) if dY_ptr else None, int(m), int(ldy), int(D), _d(alpha),
                                       _p(ell), int(ell.size), _d(diag_add), int(flags), C.c_void_p(dK_ptr), int(ldk)))

    def potrf_dev(self, dA_ptr, n, lda, dinfo_ptr):
        _chk(self._lib.gpmi_potrf_dev(self._h, C.c_void_p(dA_ptr), int(n), int(lda), C.c_void_p(dinfo_ptr)))

    # ---- probes (libgpmi_probes.so only: GPMI_USE_PROBES=1, tools/) -------------
    def _probe(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise GpmiError(-1, "%s exists in the probe build only (GPMI_USE_PROBES=1, python -m gp_amd._build --probes)" % name)
        return fn

    def probe_mfma(self, A, B):
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        out = np.empty((16, 16))
        _chk(self._probe("gpmi_probe_mfma")(self._h, _p(A), _p(B), _p(out)))
        return out

    def probe_syrk(self, m, k, reps=5):
        """(avg ms per launch, TFLOP/s at m(m+1)k algorithmic flops)."""
        ms = C.c_double(0.0)
        _chk(self._probe("gpmi_probe_syrk")(self._h, int(m), int(k), int(reps), C.byref(ms)))
        return ms.value, m * (m + 1.0) * k / (ms.value * 1e-3) / 1e12

    def probe_clock(self, reset=True):
        """(avg shader clock MHz, avg cycles per SYRK workgroup, workgroups) since the last reset."""
        out = np.zeros(3)
        _chk(self._probe("gpmi_probe_clock")(self._h, int(bool(reset)), _p(out)))
        if out[2] == 0:
            return 0.0, 0.0, 0
        return out[0] / max(out[1], 1.0) * 100.0, out[0] / out[2], int(out[2])

    def probe_fused(self):
        out = np.zeros(8)
        _chk(self._probe("gpmi_probe_fused")(self._h, _p(out)))
        return out

    def probe_body(self):
        """(loads, loop, stores, factor16, factor-wave wait, bodies): cycles of the diagonal-block bodies since the last call."""
        out = np.zeros(6)
        _chk(self._probe("gpmi_probe_body")(self._h, _p(out)))
        return out

    def probe_small(self):
        """(build, diagonal blocks, rows below, launches, trailing tiles, finalize): cycles since the last call."""
        out = np.zeros(6)
        _chk(self._probe("gpmi_probe_small")(self._h, _p(out)))
        return out

    def probe_mfma_peak(self, iters=20000):
        t = C.c_double(0.0); mhz = C.c_double(0.0)
        _chk(self._probe("gpmi_probe_mfma_peak")(self._h, int(iters), C.byref(t), C.byref(mhz)))
        return t.value, mhz.value


class SeqSampler:
    """One gpmi_seq: step(xs) -> (condMean, condVar) of the new point given the committed draws,
    commit(dot_xs) appends the draw."""

    def __init__(self, ctx, X, mn, Kn, alpha, ell, jitter=1e-6, max_steps=256):
        X = _mat(X); mn = _vec(mn); Kn = _mat(Kn); ell = _vec(ell)
        n, D = X.shape
        if mn.size != n or Kn.shape != (n, n):
            raise GpmiError(-1, "X, mn and Kn disagree on N")
        self._ctx = ctx  # keeps the context alive
        self._lib = ctx._lib
        self._h = C.c_void_p()
        self.D = D
        _chk(self._lib.gpmi_seq_create(ctx._h, C.byref(self._h), _p(X), n, max(n, 1), D, _p(mn), _p(Kn), max(n, 1),
                                       _d(alpha), _p(ell), int(ell.size), _d(jitter), int(max_steps)))

    def step(self, xs):
        xs = _vec(xs)
        if xs.size != self.D:
            raise GpmiError(-1, "xs must have D = %d entries" % self.D)
        out = np.empty(2)
        _chk(self._lib.gpmi_seq_step(self._h, _p(xs), _p(out)))
        return out[0], out[1]

    def marginals(self, Xs):
        """(mean (m,), var (m,)): for each row of Xs what step() would return on a sampler with no committed draws
        (R/tests.R:89-97 in one call); the sampler itself is left as it was."""
        Xs = _mat(Xs)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise GpmiError(-1, "Xs must have D = %d columns" % self.D)
        m = Xs.shape[0]
        mean = np.empty(m); var = np.empty(m)
        _chk(self._lib.gpmi_seq_marginals(self._h, _p(Xs), m, max(m, 1), _p(mean), _p(var)))
        return mean, var

    def commit(self, dot_xs):
        _chk(self._lib.gpmi_seq_commit(self._h, _d(dot_xs)))

    @property
    def count(self):
        return self._lib.gpmi_seq_count(self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gpmi_seq_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = {}


def default_context(device=None):
    """Process-wide lazily created context (one per device).  In a forked child of a process that
    already used the GPU the library answers GPMI_EFORK (HIP cannot be re-initialised there): the
    parent's context is never handed out and none is created behind the caller's back."""
    if device is None:
        device = int(os.environ.get("GPMI_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    key = (os.getpid(), device)
    if key not in _default:
        _default[key] = Context(device)  # raises GpmiError(-5) in a forked child of a GPU process
    return _default[key]
