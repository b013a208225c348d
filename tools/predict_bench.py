"""gpmi_gp_predict / gpmi_seq_marginals: wall time per call of the host-buffer entry points (they block until the results are
back, so the host clock brackets finished device work) on the PRODUCT library.  Every shape is warmed up, then the median of
`--reps` calls is reported.

  the reference's sizes (n = 21 / m = 41, n = 100 / m = 64, ...) on both paths: what sets the default of "small_pr";
  n = 1438, 4096 and 16384 with m = n, with and without the variance, next to the same calls at ONE test point (the
      factorisation and the fixed costs) and to gpmi_logml: the solve's rate is n^2 m flops and the mean-only kernel's rate n m
      exponentials over the time beyond the one-point call;
  gpmi_seq_marginals at n = 21 / m = 41 against 41 x (gpmi_seq_create + first gpmi_seq_step).

    python tools/predict_bench.py [--reps 5] [--max-n 16384] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402
from gp_amd import ode_gp, synth  # noqa: E402


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=16384)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = gp_amd.Context(0)
    rows = []

    def rec(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    rng = np.random.default_rng(1)
    # ---- the reference's sizes: one workgroup against the chain -------------------------------------------------------------
    for n, m, D in ((21, 41, 1), (100, 64, 1), (100, 64, 3), (128, 128, 3), (200, 200, 3)):
        X, y = synth.synth(n, D)
        Xs = rng.uniform(-0.1, 1.1, size=(m, D))
        for path, spr in (("one_workgroup", 1024), ("chain", 0)):
            ctx.set_option("small_pr", spr)
            for wv in (True, False):
                ms, mn = med(lambda: ctx.gp_predict(X, y, 1.0, [0.3], 0.1, 1e-6, Xs, want_var=wv), max(a.reps, 20))
                rec(what="gp_predict", n=n, m=m, D=D, path=path, var=wv, ms_median=ms, ms_min=mn)
    ctx.set_option("small_pr", 180)
    # ---- the chain at size ---------------------------------------------------------------------------------------------------
    for n in (1438, 4096, 16384):
        if n > a.max_n:
            continue
        X, y = synth.synth(n, 3)
        Xs = rng.uniform(-0.1, 1.1, size=(n, 3))
        t_var, _ = med(lambda: ctx.gp_predict(X, y, 1.0, [0.3], 0.1, 1e-6, Xs), a.reps)
        t_mean, _ = med(lambda: ctx.gp_predict(X, y, 1.0, [0.3], 0.1, 1e-6, Xs, want_var=False), a.reps)
        t_var1, _ = med(lambda: ctx.gp_predict(X, y, 1.0, [0.3], 0.1, 1e-6, Xs[:1]), a.reps)
        t_mean1, _ = med(lambda: ctx.gp_predict(X, y, 1.0, [0.3], 0.1, 1e-6, Xs[:1], want_var=False), a.reps)
        t_fac, _ = med(lambda: ctx.logml(X, y, 1.0, [0.3], 0.1, 1e-6), a.reps)
        d_var = max(t_var - t_var1, 1e-6)
        d_mean = max(t_mean - t_mean1, 1e-6)
        rec(what="gp_predict", n=n, m=n, D=3, ms_var=t_var, ms_mean_only=t_mean, ms_var_one_point=t_var1,
            ms_mean_only_one_point=t_mean1, ms_logml=t_fac,
            solve_tflops_beyond_one_point=float(n) * n * n / (d_var * 1e-3) / 1e12,
            mean_only_gexp_per_s_beyond_one_point=float(n) * n / (d_mean * 1e-3) / 1e9,
            mean_only_cheaper=bool(t_mean < t_var))
    # ---- the sweep of R/tests.R:89-97 ---------------------------------------------------------------------------------------
    t = np.linspace(-2, 2, 21)
    f = np.exp(t)
    p = ode_gp.p_dotXn(t, f, [1.0, 1.0], 0.05, joint=True, ctx=ctx)
    ps = ode_gp.p_Xn(t, f, [1.0, 1.0], 0.05, joint=True, ctx=ctx)
    X = ps["condMean"].reshape(-1, 1)
    Xs = np.linspace(0.0, 7.0, 41).reshape(-1, 1)
    smp = ctx.seq_sampler(X, p["condMean"], p["condVar"], 1.0, [1.0], 1e-6, max_steps=2)

    def sweep():
        out = []
        for xs in Xs:
            s = ctx.seq_sampler(X, p["condMean"], p["condVar"], 1.0, [1.0], 1e-6, max_steps=1)
            out.append(s.step(xs))
            s.close()
        return out

    t_m, _ = med(lambda: smp.marginals(Xs), max(a.reps, 20))
    t_s, _ = med(sweep, a.reps)
    rec(what="seq_marginals", n=21, m=41, ms_marginals=t_m, ms_41_create_plus_step=t_s)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
