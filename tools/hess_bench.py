"""The exact Hessian of the log marginal likelihood (gpmi_logml_hess) beside what it replaces: ONE gpmi_logml_grad call on the
same context, and the 2 q of them (q = 2 + n_ell) that central differences of the gradient cost (optim(..., hessian = TRUE)).
One length-scale and one per dimension (D = 3).  Host-buffer calls, every timed window ends in the call's own synchronise;
every shape is warmed up first; the contenders alternate in the same process in windows of at least --window seconds, and the
median over the rounds is reported.  At n <= 128 gpmi_logml_grad runs as one workgroup (the context's default),
gpmi_logml_hess as the launch chain at every n.

    python tools/hess_bench.py [--sizes 21,128,...] [--window 0.3] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402
from loo_bench import D, ALPHA, SIGMA, JITTER, SIZES, inputs, window  # noqa: E402

ELLS = {"iso": np.array([0.8]), "ard": np.array([0.8, 0.7, 0.9])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    ctx = gp_amd.Context(0)
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        X, y, _ = inputs(n)
        for kind, ell in ELLS.items():
            q = 2 + ell.size
            fns = {"hess": lambda: ctx.logml_hess(X, y, ALPHA, ell, SIGMA, JITTER),
                   "logml_grad": lambda: ctx.logml_grad(X, y, ALPHA, ell, SIGMA, JITTER)}
            assert fns["hess"]()["info"] == 0
            for fn in fns.values():
                fn()
            times = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    times[k].append(window(fn, args.window))
            row = {"n": n, "D": D, "ell": kind, "q": q}
            for k in fns:
                row[k + "_us"] = 1e6 * statistics.median(times[k])
                row[k + "_us_all"] = [1e6 * x for x in times[k]]
            row["fd_us"] = 2 * q * row["logml_grad_us"]
            row["hess_over_logml_grad"] = row["hess_us"] / row["logml_grad_us"]
            row["hess_over_fd"] = row["hess_us"] / row["fd_us"]
            rows.append(row)
            print("n=%5d %s: hess %.0f us; logml_grad %.0f us (hess = x %.2f); %d gradient calls %.0f us (hess = x %.2f)" % (
                n, kind, row["hess_us"], row["logml_grad_us"], row["hess_over_logml_grad"], 2 * q, row["fd_us"], row["hess_over_fd"]),
                flush=True)
    print(json.dumps({"hess_bench": rows}))


if __name__ == "__main__":
    main()
