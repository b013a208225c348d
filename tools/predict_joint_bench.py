"""gpmi_gp_predict_joint: wall time per call of the host-buffer entry point (it blocks until the results are back, so the host
clock brackets finished device work) on the PRODUCT library, and the product kernel against the loop it replaced.

  routes:  (n, m) = (21, 41), (100, 64), (199, 199), (300, 259), (1438, 500), (4096, 1024), D = 3, B = 0 / 1 / 64 / 200, without the
           covariance coming back (want_cov = False: what a sampler asks for) -- the one-workgroup kernel ("small_pj" = 1024)
           where n + m + 1 <= 1024 and the blocked chain ("small_pj" = 0).  The two routes of a shape are measured in ALTERNATING
           windows (wg, chain, wg, chain, ...: three windows each, the median of a window's calls, then the median of the three),
           so that clock and neighbour drift hits both alike.  The default of "small_pj" is the crossover in rows at B = 1.
  product: `--product` (needs the probe build, GPMI_USE_PROBES=1): gpmi_probe_tril_draws at m = 1024 / 4096, B = 16 / 64 / 200 --
           the triangular matrix-matrix kernel (k_tril_draws) beside a loop of B launch_trmv_lower calls on the same factor, HIP
           events around 20 repetitions each, three windows, median.

    python tools/predict_joint_bench.py [--crossover] [--reps 20] [--max-n 4096] [--json out.json]
    GPMI_USE_PROBES=1 python tools/predict_joint_bench.py --product [--json out.json]

Measured on one MI355X (the full table is in DESIGN.md section 8), one workgroup / chain, microseconds per call:
  (21, 41):    B = 0: 43 / 112    B = 1: 61 / 156    B = 64: 401 / 180    B = 200: 1133 / 186
  (100, 64):   B = 0: 96 / 149    B = 1: 116 / 196   B = 64: 559 / 215    B = 200: 1517 / 225
  (199, 199):  B = 0: 320 / 189   B = 1: 406 / 300   B = 64: 1613 / 319   B = 200: 4205 / 331
  (300, 259):  B = 0: 639 / 193   B = 1: 802 / 333   B = 64: 3523 / 384   B = 200: 9382 / 400
  (1438, 500), chain: 521 / 719 / 818 / 851;  (4096, 1024), chain: 1900 / 2258 / 2434 / 2499
  --crossover, B = 1: n = m = 140 (281 rows): 237 / 243, 150 (301 rows): 255 / 254, 160: 261 / 253 -> "small_pj" = 300
  --product: m = 1024, B = 16 / 64 / 200: kernel 0.081 / 0.196 / 0.197 ms, loop 0.93 / 3.72 / 11.6 ms (11 / 19 / 59 x);
             m = 4096: kernel 0.318 / 0.773 / 0.778 ms, loop 2.28 / 9.13 / 28.6 ms (7 / 12 / 37 x)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402

SHAPES = ((21, 41), (100, 64), (199, 199), (300, 259), (1438, 500), (4096, 1024))
BS = (0, 1, 64, 200)


def window(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-n", type=int, default=4096)
    ap.add_argument("--product", action="store_true")
    ap.add_argument("--crossover", action="store_true", help="n = m = 90 ... 170 in steps of 10 at B = 1 only: where the routes cross")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = gp_amd.Context(0)
    rows = []

    def rec(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    if a.product:
        ms2 = (C.c_double * 2)()
        for m in (1024, 4096):
            for B in (16, 64, 200):
                w = []
                for _ in range(3):
                    rc = ctx._lib.gpmi_probe_tril_draws(ctx._h, m, B, 20, ms2)
                    if rc:
                        raise SystemExit("gpmi_probe_tril_draws failed: %d" % rc)
                    w.append((ms2[0], ms2[1]))
                k, lp = float(np.median([x[0] for x in w])), float(np.median([x[1] for x in w]))
                rec(what="product", m=m, B=B, ms_tril_draws=k, ms_trmv_loop=lp, loop_over_kernel=lp / k)
    else:
        rng = np.random.default_rng(1)
        for n, m in (tuple((k, k) for k in range(90, 171, 10)) if a.crossover else SHAPES):
            if n > a.max_n:
                continue
            X = np.asfortranarray(rng.uniform(size=(n, 3)))
            y = np.sin(2 * np.pi * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
            Xs = np.asfortranarray(rng.uniform(-0.1, 1.1, size=(m, 3)))
            routes = (("one_workgroup", 1024), ("chain", 0)) if n + m + 1 <= 1024 else (("chain", 0),)
            reps = a.reps if n <= 300 else max(a.reps // 4, 3)
            for B in ((1,) if a.crossover else BS):
                Z = rng.standard_normal((m, B)) if B else None
                w = {r: [] for r, _ in routes}
                for _ in range(3):
                    for r, spj in routes:
                        ctx.set_option("small_pj", spj)
                        w[r].append(window(lambda: ctx.gp_predict_joint(X, y, 1.0, (0.3, 0.5, 0.8), 0.1, 1e-6, Xs, post_jitter=1e-6,
                                                                        Z=Z, want_cov=False), reps))
                rec(what="route", n=n, m=m, rows=n + m + 1, B=B, **{"ms_" + r: float(np.median(v)) for r, v in w.items()})
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
