"""CPU: the restatements of tests/interp_vjp_reference.py -- the analytic gradients of the cubic Hermite and the
GP-regression latent models (test_interpolate.R) against central differences of their own lp__, and the resource
usage of the kernels that compute them on the device (no spills, no scratch)."""
import os
import re
import subprocess

import numpy as np

import interp_vjp_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fd_check(L, dL, y, z, l, sigma, lo, hi, h=1e-6):
    lp0, g = ref.log_prob_grad(L, dL, y, l, sigma, z, lo, hi)
    assert np.isfinite(lp0)
    f = lambda l_, s_, z_: ref.log_prob(L, y, l_, s_, z_, lo, hi)
    fd_l = (f(l + h, sigma, z) - f(l - h, sigma, z)) / (2 * h)
    fd_s = (f(l, sigma + h, z) - f(l, sigma - h, z)) / (2 * h)
    assert abs(g[0] - fd_l) <= 1e-6 * max(1.0, abs(fd_l)), (g[0], fd_l)
    assert abs(g[1] - fd_s) <= 1e-6 * max(1.0, abs(fd_s)), (g[1], fd_s)
    for i in (0, z.size // 3, z.size - 1):
        e = np.zeros_like(z); e[i] = h
        fd = (f(l, sigma, z + e) - f(l, sigma, z - e)) / (2 * h)
        assert abs(g[2 + i] - fd) <= 1e-6 * max(1.0, abs(fd)), (i, g[2 + i], fd)


def test_cubic_hermite_model_gradient_by_central_differences(orc):
    x = np.linspace(0.0, 8.0, 12)
    lp = np.linspace(0.6, 1.1, 5)
    Ls, dLs = zip(*[orc.rbf_cov_chol(x, l) for l in lp])
    L, dL = ref.hermite_model(orc, lp, list(Ls), list(dLs))
    rng = np.random.default_rng(3)
    z = rng.standard_normal(12); y = np.sin(x) + 0.1 * rng.standard_normal(12)
    for l in (0.66, 0.83, 1.02):   # inside intervals (the blend is C1 only across knots)
        _fd_check(L, dL, y, z, l, 0.4, lp.min(), lp.max())


def test_gp_regression_model_gradient_by_central_differences(orc):
    x = np.linspace(0.0, 8.0, 12)
    lp = np.array([0.5, 1.5, 2.5, 3.5])
    exact = [orc.rbf_cov_chol(x, l)[0] for l in lp]
    M = ref.gp_lookup(lp, exact)
    # at a knot the lookup reproduces that knot's factor up to the jitter's effect
    for p, l in enumerate(lp):
        assert np.max(np.abs(ref.gp_L(l, lp, M) - exact[p])) <= 1e-9
    L, dL = ref.gp_model(lp, M)
    rng = np.random.default_rng(4)
    z = rng.standard_normal(12); y = np.cos(x) + 0.1 * rng.standard_normal(12)
    for l in (0.7, 1.5, 2.2, 3.3):
        _fd_check(L, dL, y, z, l, 0.3, lp.min(), lp.max())


def test_kernels_do_not_spill():
    """Every kernel of interp_kernels.hip keeps its state in registers and LDS: 0 VGPRs spilled, 0 bytes of scratch."""
    from gp_amd import _build
    src = os.path.join(_build.CSRC, "interp_kernels.hip")
    assert os.path.exists(src), src
    out = os.path.join(ROOT, "build", "resource_check")
    os.makedirs(out, exist_ok=True)
    cmd = [_build.hipcc(), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++20", "-fPIC", "-c", src, "-o",
           os.path.join(out, "interp_kernels.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=_build.CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    for must in ("k_tri_vjp_small", "k_tri_vjp", "k_tri_vjp_fin", "k_tri_vjp_lsum", "k_gp_blend", "k_gp_lookup"):
        assert any(must in k for k in kernels), (must, list(kernels))
    for k, v in kernels.items():
        assert v.get("VGPRs Spill") == 0, (k, v)
        assert v.get("ScratchSize [bytes/lane]") == 0, (k, v)
