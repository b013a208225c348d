"""Microseconds per host-buffer call of gpmi_latent_gp_lp_grad (forward product, likelihood head, its adjoint and the reverse
sweep with one factorisation) per family -- normal (k = 1, m = 1: models/exact_gp.stan), bernoulli_logit (k = 1, m = 1:
models/westbrook_exact.stan), normal_logsd (k = 2, m = 5: models/heteroscedastic.stan) -- next to gpmi_exact_gp_f,
gpmi_exact_gp_f_vjp and their host-glued composition (value, ubar in numpy, VJP: what exact_gp_log_prob_grad does by default).
Isotropic D = 1 at the reference's spacing (x on [0, 10] scaled with n), jitter 1e-6.
python tools/latent_lik_bench.py [reps] [--passes P] [--sizes n,n,...]   (P passes over the sizes: the spread between them)"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402

FAMILIES = (("normal", 1, 1), ("bernoulli_logit", 1, 1), ("normal_logsd", 2, 5))


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
    ap.add_argument("--sizes", default="30,100,256,1000,1438,4096")
    a = ap.parse_args()
    ctx = gp_amd.Context(0)
    rng = np.random.default_rng(0)
    sigma = 0.5
    for ps in range(a.passes):
        for n in [int(t) for t in a.sizes.split(",")]:
            x = np.linspace(0, 10 * n / 100, n).reshape(-1, 1)
            z = rng.standard_normal(n); u = rng.standard_normal(n)
            r = a.reps if n <= 1000 else max(a.reps // 5, 3)
            tv = per_call(lambda: ctx.exact_gp_f(x, 1.0, [1.0], z, 1e-6), r)
            tg = per_call(lambda: ctx.exact_gp_f_vjp(x, 1.0, [1.0], z, u, 1e-6), r)

            def glued():
                f = ctx.exact_gp_f(x, 1.0, [1.0], z, 1e-6)
                ctx.exact_gp_f_vjp(x, 1.0, [1.0], z, (u - f) / (sigma * sigma), 1e-6)
            tc = per_call(glued, r)
            line = "pass %d n=%5d: exact_gp_f %9.1f us   exact_gp_f_vjp %9.1f us   value + vjp glued %9.1f us  " % (ps, n, tv, tg, tc)
            for family, k, m in FAMILIES:
                Z = rng.standard_normal((n, k)) * (1.0 if k == 1 else 0.3)
                Y = (rng.uniform(size=(n, m)) < 0.4).astype(float) if family == "bernoulli_logit" else rng.standard_normal((n, m))
                sg = sigma if family == "normal" else None
                t = per_call(lambda: ctx.latent_gp_lp_grad(x, 1.0, [1.0], Z, family, Y, sg, 1e-6, want_f=False), r)
                line += " %s %9.1f us" % (family, t)
            print(line, flush=True)


if __name__ == "__main__":
    main()
