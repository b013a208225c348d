"""Exact leave-one-out cross-validation (gpmi_logml_loo) with and without its gradient, beside gpmi_logml_grad on the same
context: what the extra symmetric product and the O(n^2) passes cost.  Host-buffer calls, every timed window ends in the call's
own synchronise; every shape is warmed up first; the three contenders alternate in the same process in windows of at least
--window seconds, and the median over the rounds is reported.  At n <= 128 gpmi_logml_grad runs as one workgroup (the
context's default), gpmi_logml_loo as the launch chain at every n.

    python tools/loo_bench.py [--sizes 21,128,...] [--window 0.3] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402

SIZES = (21, 128, 1438, 4096)   # 1438: the reference's largest fit
D, ALPHA, SIGMA, JITTER = 3, 1.1, 0.1, 1e-6


def inputs(n):
    """About one point per length-scale in D = 3 dimensions."""
    rng = np.random.default_rng(7000 + n)
    ell = np.array([0.8])
    X = rng.random((n, D)) * (0.8 * n ** (1.0 / D))
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(D)) + 0.1 * rng.standard_normal(n)
    return X, y, ell


def window(fn, seconds):
    """Seconds per call of fn over a window of at least `seconds` (at least two calls)."""
    calls = 0
    t0 = time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds and calls >= 2:
            return dt / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    ctx = gp_amd.Context(0)
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        X, y, ell = inputs(n)
        fns = {"loo_grad": lambda: ctx.logml_loo(X, y, ALPHA, ell, SIGMA, JITTER),
               "loo": lambda: ctx.logml_loo(X, y, ALPHA, ell, SIGMA, JITTER, want_grad=False),
               "logml_grad": lambda: ctx.logml_grad(X, y, ALPHA, ell, SIGMA, JITTER)}
        assert fns["loo_grad"]()["info"] == 0
        for fn in fns.values():
            fn()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn, args.window))
        row = {"n": n, "D": D}
        for k in fns:
            row[k + "_us"] = 1e6 * statistics.median(times[k])
            row[k + "_us_all"] = [1e6 * x for x in times[k]]
        row["loo_grad_over_logml_grad"] = row["loo_grad_us"] / row["logml_grad_us"]
        row["loo_over_logml_grad"] = row["loo_us"] / row["logml_grad_us"]
        rows.append(row)
        print("n=%5d: loo + gradient %.0f us (x %.2f); loo alone %.0f us (x %.2f); logml_grad %.0f us" % (
            n, row["loo_grad_us"], row["loo_grad_over_logml_grad"], row["loo_us"], row["loo_over_logml_grad"], row["logml_grad_us"]),
            flush=True)
    print(json.dumps({"loo_bench": rows}))


if __name__ == "__main__":
    main()
