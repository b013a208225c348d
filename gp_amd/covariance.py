"""Mirror of the Rcpp exports in covariance.cpp (rbf_cov_chol :9-47, approx_L :49-96), of the Stan
external function approx_Lz (models/cubic_interpolated_gp.hpp:38-73) and of the GP-regression interpolation of
models/interpolated_gp.stan:9-47."""
import numpy as np

from ._lib import default_context


def rbf_cov_chol(x1, l_, ctx=None):
    """list(L=, dLdl=): Sigma_ij = exp(-(xi-xj)^2/(2 l^2)) + 1e-10 I, L = lower Cholesky,
    dLdl = exact dL/dl (the reference gets it by forward-mode AD, fvar<double>)."""
    L, dL = (ctx or default_context()).rbf_cov_chol(x1, float(l_))
    return {"L": L, "dLdl": dL}


def _neighbours(l, lp):
    """Interval rule of covariance.cpp:57-61 (first p with lp[p+1] >= l), clamped to the last interval."""
    lp = np.asarray(lp, dtype=np.float64)
    k = 0
    while k < lp.size - 1 and not lp[k + 1] >= l:
        k += 1
    return min(k, lp.size - 2)


def approx_L(l, lp, Ls, dLdls, ctx=None):
    """approx_L(l, lp, Ls, dLdls): cubic Hermite blend of the tabulated Cholesky factors at length-scale l
    (covariance.cpp:49-96).  Only the two neighbouring table entries travel to the device."""
    c = ctx or default_context()
    k = _neighbours(l, lp)
    c.interp_load([lp[k], lp[k + 1]], [Ls[k], Ls[k + 1]], [dLdls[k], dLdls[k + 1]])
    return c.approx_L(l)


def approx_Lz(l, lp, Ls, dLdls, z, ctx=None):
    """approx_Lz(l, lp, Ls, dLdls, z) = approx_L(l, ...) %*% z (models/cubic_interpolated_gp.hpp:38-73)."""
    c = ctx or default_context()
    k = _neighbours(l, lp)
    c.interp_load([lp[k], lp[k + 1]], [Ls[k], Ls[k + 1]], [dLdls[k], dLdls[k + 1]])
    return c.approx_Lz(l, z)


def approx_Lz_grad(l, lp, Ls, dLdls, z, ctx=None):
    """(f, dfdl) of approx_Lz: the value and the partial with respect to l that the `var` overload of
    build_output attaches under Stan's reverse mode (models/cubic_interpolated_gp.hpp:6-32, dvdl :67)."""
    c = ctx or default_context()
    k = _neighbours(l, lp)
    c.interp_load([lp[k], lp[k + 1]], [Ls[k], Ls[k + 1]], [dLdls[k], dLdls[k + 1]])
    return c.approx_Lz_grad(l, z)


def approx_Lz_vjp(l, lp, Ls, dLdls, z, fbar, ctx=None):
    """(f, zbar, lbar): approx_Lz and its vector-Jacobian product under Stan's reverse mode
    (models/cubic_interpolated_gp.hpp:6-32,38-73): zbar = approx_L(l)^T fbar, lbar = sum(fbar * (dv/dl) z).
    z and fbar are vectors or n x k matrices."""
    c = ctx or default_context()
    k = _neighbours(l, lp)
    c.interp_load([lp[k], lp[k + 1]], [Ls[k], Ls[k + 1]], [dLdls[k], dLdls[k + 1]])
    return c.approx_Lz_vjp(l, z, fbar)


class FactorInterpolator:
    """Device-resident table for repeated queries: what test_interpolate.R:9-19 builds with P calls of
    rbf_cov_chol and cubic_interpolated_gp.stan consumes once per leapfrog step."""

    def __init__(self, x, lp, ctx=None):
        self.ctx = ctx or default_context()
        self.lp = np.asarray(lp, dtype=np.float64)
        self.ctx.interp_build(x, self.lp)

    def L(self, l):
        return self.ctx.approx_L(l)

    def Lz(self, l, z):
        return self.ctx.approx_Lz(l, z)

    def Lz_grad(self, l, z):
        return self.ctx.approx_Lz_grad(l, z)

    def Lz_vjp(self, l, z, fbar):
        """(f, zbar, lbar) of f = L(l) z with upstream adjoint fbar (see approx_Lz_vjp)."""
        return self.ctx.approx_Lz_vjp(l, z, fbar)


class GPFactorInterpolator:
    """The transformed data of models/interpolated_gp.stan:9-28 on the device: lookup = (Sigma_P \\ exact)^T with
    Sigma_P = cov_exp_quad(lp, 1, rho) + jitter I and exact the P factors chol(cov_exp_quad(x, 1, lp[p]) + 1e-10 I),
    kept as P lower triangles; L(l) = sum_p exp(-(l - lp_p)^2 / (2 rho^2)) M_p (:39-42).  Lives beside the Hermite
    table of FactorInterpolator in the same context."""

    def __init__(self, x, lp, rho=1.0, jitter=1e-10, ctx=None):
        self.ctx = ctx or default_context()
        self.lp = np.asarray(lp, dtype=np.float64)
        self.rho = float(rho)
        self.jitter = float(jitter)
        self.ctx.interp_gp_build(x, self.lp, self.rho, self.jitter)

    def L(self, l):
        return self.ctx.interp_gp_L(l)

    def Lz(self, l, z):
        return self.ctx.interp_gp_Lz(l, z)

    def Lz_vjp(self, l, z, fbar):
        """(f, zbar, lbar): f = L(l) z, zbar = L(l)^T fbar, lbar = sum(fbar * (dL/dl) z)."""
        return self.ctx.interp_gp_Lz_vjp(l, z, fbar)
