"""Microseconds per call of gpmi_exact_gp_f_vjp (value + vector-Jacobian product of models/exact_gp.stan:17-25) next to
gpmi_exact_gp_f (value only), host buffers, one column, isotropic D = 1 at the reference's spacing (x on [0, 10] scaled with n),
and for n <= 256 also the blocked chain (small_vjp = 0).  python tools/exact_gp_vjp_bench.py [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402


def per_call(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    ctx = gp_amd.Context(0)
    chain = gp_amd.Context(0)
    chain.set_option("small_vjp", 0)
    rng = np.random.default_rng(0)
    for n in (30, 100, 256, 1000, 4096):
        x = np.linspace(0, 10 * n / 100, n).reshape(-1, 1)
        z = rng.standard_normal(n); u = rng.standard_normal(n)
        r = reps if n <= 1000 else max(reps // 5, 3)
        tv = per_call(lambda: ctx.exact_gp_f(x, 1.0, [1.0], z, 1e-6), r)
        tg = per_call(lambda: ctx.exact_gp_f_vjp(x, 1.0, [1.0], z, u, 1e-6), r)
        line = "n=%5d: exact_gp_f %9.1f us   exact_gp_f_vjp %9.1f us" % (n, tv, tg)
        if n <= 256:
            line += "   (blocked chain %9.1f us)" % per_call(lambda: chain.exact_gp_f_vjp(x, 1.0, [1.0], z, u, 1e-6), r)
        print(line, flush=True)


if __name__ == "__main__":
    main()
