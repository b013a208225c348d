"""gpmi_joint_predict: wall time per call of the host-buffer entry point (it blocks until the results are back, so the host
clock brackets finished device work) on the PRODUCT library, and the fused star-block builder against the launches it replaced.

  routes:  n = m = 21 / 199 / 350 / 2048, orders = 7 (p = 3: 5 n + 1 rows), B = 0 / 1 / 64, without the covariance coming back
           (want_cov = False: what a sampler asks for) -- the one-workgroup kernel ("small_jp" = 1024) where 5 n + 1 <= 1024 and
           the chain ("small_jp" = 0).  The two routes of a shape are measured in ALTERNATING windows (wg, chain, wg, chain, ...:
           three windows each, the median of a window's calls, then the median of the three), so that clock and neighbour
           drift hits both alike.  `--crossover`: n = m = 30 ... 100 in steps of 10 at B = 1 only (151 ... 501 rows).
  builder: `--builder` (needs the probe build, GPMI_USE_PROBES=1): gpmi_probe_joint_star at the same four sizes, p = 3 -- the
           fused builder (k_joint_star, one launch) beside the 12 launch_deriv_cov launches that write the same blocks, HIP
           events around 20 repetitions each, three windows, median.

    python tools/joint_predict_bench.py [--crossover] [--reps 20] [--max-n 2048] [--json out.json]
    GPMI_USE_PROBES=1 python tools/joint_predict_bench.py --builder [--json out.json]

Measured on one MI355X (the tables are in DESIGN.md section 8), one workgroup / chain, microseconds per call:
  n = m = 21:   B = 0: 82 / 105     B = 1: 102 / 142    B = 64: 547 / 180
  n = m = 199:  B = 0: 2133 / 228   B = 1: 2880 / 464   B = 64: 9730 / 596
  n = m = 350, chain: 325 / 733 / 946;  n = m = 2048, chain: 5730 / 8926 / 10200
  --crossover, B = 1: n = m = 40 (201 rows): 165 / 187, 50 (251 rows): 265 / 228, 60: 304 / 256 -> "small_jp" = 220
  --builder: n = m = 21 / 199 / 350 / 2048: fused 12.3 / 18.1 / 19.2 / 83.7 us, 12 launches 100 / 112 / 113 / 218 us
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

SIZES = (21, 199, 350, 2048)
BS = (0, 1, 64)
ORDERS = 7


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
    ap.add_argument("--max-n", type=int, default=2048)
    ap.add_argument("--builder", action="store_true")
    ap.add_argument("--crossover", action="store_true", help="n = m = 30 ... 100 in steps of 10 at B = 1 only: where the routes cross")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = gp_amd.Context(0)
    rows = []

    def rec(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    if a.builder:
        ms2 = (C.c_double * 2)()
        for n in SIZES:
            if n > a.max_n:
                continue
            w = []
            for _ in range(3):
                rc = ctx._lib.gpmi_probe_joint_star(ctx._h, n, n, ORDERS, 20, ms2)
                if rc:
                    raise SystemExit("gpmi_probe_joint_star failed: %d" % rc)
                w.append((ms2[0], ms2[1]))
            k, lp = float(np.median([x[0] for x in w])), float(np.median([x[1] for x in w]))
            rec(what="builder", n=n, m=n, orders=ORDERS, ms_joint_star=k, ms_deriv_cov_x12=lp, launches_over_fused=lp / k)
    else:
        rng = np.random.default_rng(1)
        for n in (tuple(range(30, 101, 10)) if a.crossover else SIZES):
            if n > a.max_n:
                continue
            m, l = n, max(2.0 / n, 0.02)   # a few points per length-scale: S stays well inside double precision
            t = np.sort(rng.uniform(-1, 1, n))
            yy = np.concatenate([np.sin(3 * t), 3 * np.cos(3 * t)]) + 0.1 * rng.standard_normal(2 * n)
            ts = rng.uniform(-1.1, 1.1, m)
            pj = [1e-4 / l ** (2 * k) for k in range(3)]
            nrows = 2 * n + 3 * m + 1
            routes = (("one_workgroup", 1024), ("chain", 0)) if nrows <= 1024 else (("chain", 0),)
            reps = a.reps if n <= 350 else max(a.reps // 4, 3)
            for B in ((1,) if a.crossover else BS):
                Z = rng.standard_normal((3 * m, B)) if B else None
                w = {r: [] for r, _ in routes}
                status = 0   # reported, not fatal: the time of a factorisation does not depend on its pivots' signs
                for _ in range(3):
                    for r, sjp in routes:
                        ctx.set_option("small_jp", sjp)
                        res = {}

                        def call():
                            res["info"] = ctx.joint_predict(t, yy, 1.0, l, 0.1, 1e-3, ts, ORDERS, pj, Z=Z, want_cov=False)["info"]
                        w[r].append(window(call, reps))
                        status = max(status, res["info"])
                rec(what="route", n=n, m=m, rows=nrows, B=B, status=status, **{"ms_" + r: float(np.median(v)) for r, v in w.items()})
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
