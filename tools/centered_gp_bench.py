"""Microseconds per host-buffer call of gpmi_centered_gp_lp_grad (the centred latent GP of models/heteroscedastic_centered.stan:
k = 2 columns, the normal_logsd head on m = 5 replicates, one factorisation) on the default path and on the blocked chain
(small_cen = 0), next to what the library offered before it: k calls of gpmi_logml_grad (sigma = 0) on the same data -- the value
and the hyper-gradient, but no gradient in the columns -- and, for scale, the non-centred gpmi_latent_gp_lp_grad.
Isotropic D = 1 at the reference's spacing (x on [0, 10] scaled with n), jitter 1e-6.
python tools/centered_gp_bench.py [reps] [--passes P] [--sizes n,n,...]   (P passes over the sizes: the spread between them)"""
import argparse
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
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=50)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--sizes", default="10,100,256,700,2048,4096")
    a = ap.parse_args()
    ctx = gp_amd.Context(0)
    chain = gp_amd.Context(0)
    chain.set_option("small_cen", 0)
    rng = np.random.default_rng(0)
    k, m = 2, 5
    for ps in range(a.passes):
        for n in [int(t) for t in a.sizes.split(",")]:
            x = np.linspace(0, 10 * n / 100, n).reshape(-1, 1)
            F = rng.standard_normal((n, k)) * 0.3
            Y = rng.standard_normal((n, m))
            r = a.reps if n <= 1000 else max(a.reps // 5, 3)
            tc = per_call(lambda: ctx.centered_gp_lp_grad(x, 1.0, [1.0], F, "normal_logsd", Y, None, 1e-6), r)
            tn = per_call(lambda: ctx.centered_gp_lp_grad(x, 1.0, [1.0], F, "none", None, None, 1e-6), r)
            tch = per_call(lambda: chain.centered_gp_lp_grad(x, 1.0, [1.0], F, "normal_logsd", Y, None, 1e-6), r)

            def k_logml_grads():
                for c in range(k):
                    ctx.logml_grad(x, F[:, c], 1.0, [1.0], 0.0, 1e-6)
            tl = per_call(k_logml_grads, r)
            tlat = per_call(lambda: ctx.latent_gp_lp_grad(x, 1.0, [1.0], F, "normal_logsd", Y, None, 1e-6, want_f=False), r)
            print("pass %d n=%5d: centered (default path) %9.1f us   head none %9.1f us   blocked chain %9.1f us   %d x logml_grad %9.1f us"
                  "   latent_gp_lp_grad %9.1f us" % (ps, n, tc, tn, tch, k, tl, tlat), flush=True)


if __name__ == "__main__":
    main()
