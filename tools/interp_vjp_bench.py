"""Microseconds per call of the interpolated models' reverse mode next to the value + l-partial call and the exact model's
vector-Jacobian product, k = 1: approx_Lz_grad, approx_Lz_vjp (cubic Hermite, 4 triangles), interp_gp_Lz_vjp (GP regression,
P triangles) and exact_gp_f_vjp, host buffers and _dev calls (device pointers, timed by a stream synchronisation per
batch).  Effective bandwidth = triangles read x n(n+1)/2 x 8 B / time.  n = 100 (P = 10, x = linspace(0, 10, 100), the
reference's grid of test_interpolate.R:9), 1024, 4096, 8192 (x at unit spacing).
python tools/interp_vjp_bench.py [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402


def per_call(fn, reps, sync=None):
    fn()
    if sync:
        sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    if sync:
        sync()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    ctx = gp_amd.Context(0)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    P = 10
    for n in (100, 1024, 4096, 8192):
        lp = np.linspace(0.34, 1.94, P)   # qgamma(0.05 .. 0.95, 4, 4), rounded
        # n = 100: the reference's x; larger n: unit spacing (positive definite with the 1e-10 jitter at every knot)
        x = np.linspace(0.0, 10.0, n) if n == 100 else np.arange(float(n))
        ctx.interp_build(x, lp)
        ctx.interp_gp_build(x, lp)
        z = rng.standard_normal(n); u = rng.standard_normal(n)
        r = reps if n <= 1024 else max(reps // 10, 5)
        l = l2 = 0.5 * (lp[3] + lp[4])
        dz = torch.from_numpy(z).to(dev); du = torch.from_numpy(u).to(dev)
        df = torch.zeros(n, dtype=torch.float64, device=dev); dg = torch.zeros_like(df); dzb = torch.zeros_like(df)
        dl = torch.zeros(1, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        tri = n * (n + 1) / 2 * 8
        res = {
            "approx_Lz_grad": (per_call(lambda: ctx.approx_Lz_grad(l2, z), r),
                               per_call(lambda: ctx.approx_Lz_grad_dev(l2, dz.data_ptr(), df.data_ptr(), dg.data_ptr()), r, ctx.sync), 4),
            "approx_Lz_vjp": (per_call(lambda: ctx.approx_Lz_vjp(l2, z, u), r),
                              per_call(lambda: ctx.approx_Lz_vjp_dev(l2, dz.data_ptr(), 1, n, du.data_ptr(), n, df.data_ptr(), n,
                                                                     dzb.data_ptr(), n, dl.data_ptr()), r, ctx.sync), 4),
            "interp_gp_Lz_vjp": (per_call(lambda: ctx.interp_gp_Lz_vjp(l, z, u), r),
                                 per_call(lambda: ctx.interp_gp_Lz_vjp_dev(l, dz.data_ptr(), 1, n, du.data_ptr(), n, df.data_ptr(), n,
                                                                           dzb.data_ptr(), n, dl.data_ptr()), r, ctx.sync), P),
        }
        for name, (th, td, T) in res.items():
            print("n=%5d %-17s host %9.1f us   dev %9.1f us   %6.2f TB/s (dev)" % (n, name, th, td, T * tri / (td * 1e-6) / 1e12),
                  flush=True)
        if n <= 4096:
            xe = np.linspace(0.0, 10.0 * n / 100, n).reshape(-1, 1)
            te = per_call(lambda: ctx.exact_gp_f_vjp(xe, 1.0, [1.0], z, u, 1e-6), max(r // 4, 3))
            print("n=%5d %-17s host %9.1f us" % (n, "exact_gp_f_vjp", te), flush=True)
        ctx.interp_free(); ctx.interp_gp_free()


if __name__ == "__main__":
    main()
