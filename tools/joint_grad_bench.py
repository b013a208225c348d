"""Value + gradient of the joint [y; y'] model (gpmi_joint_logml_grad) beside six gpmi_joint_logml calls: what central
differences in (alpha, l, sigma) cost without it.  Host-buffer calls, every timed window ends in the call's own synchronise;
every shape is warmed up first; the two contenders alternate in the same process in windows of at least --window seconds, and the
median over the rounds is reported.

    python tools/joint_grad_bench.py [--sizes 21,199,...] [--window 0.3] [--rounds 3] [--only grad|value]

--only runs one contender alone (for a kernel trace of its own)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402

SIZES = (21, 199, 719, 1536, 2048, 4096, 8192)   # orders 42 .. 16384; 1536: the last order on the augmented route
ALPHA, L_PER_POINT, SIGMA, JITTER = 1.1, 3.0, 0.1, 1e-3


def inputs(n):
    """t: a perturbed regular grid on [-1, 1]; the length-scale follows the spacing (about three points per length-scale)."""
    rng = np.random.default_rng(9000 + n)
    t = np.linspace(-1.0, 1.0, n) + (0.6 / n) * rng.uniform(-1.0, 1.0, n)
    yy = np.concatenate([np.sin(3 * t), 3 * np.cos(3 * t)]) + 0.1 * rng.standard_normal(2 * n)
    return t, yy, max(L_PER_POINT * 2.0 / n, 1e-3) if n > 6 else 0.5


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
    ap.add_argument("--only", choices=("grad", "value"), default=None)
    args = ap.parse_args()
    ctx = gp_amd.Context(0)
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        t, yy, l = inputs(n)
        h = 1e-5

        def grad():
            return ctx.joint_logml_grad(t, yy, ALPHA, l, SIGMA, JITTER)

        def six_values():
            for d in ((h, 0, 0), (-h, 0, 0), (0, h, 0), (0, -h, 0), (0, 0, h), (0, 0, -h)):
                ctx.joint_logml(t, yy, ALPHA + d[0], l + d[1], SIGMA + d[2], JITTER)

        if args.only != "value":
            grad()
        if args.only != "grad":
            six_values()
        tg, tv = [], []
        for _ in range(args.rounds):
            if args.only != "value":
                tg.append(window(grad, args.window))
            if args.only != "grad":
                tv.append(window(six_values, args.window))
        row = {"n": n, "order": 2 * n, "l": l,
               "grad_ms": 1e3 * statistics.median(tg) if tg else None, "grad_ms_all": [1e3 * x for x in tg],
               "six_values_ms": 1e3 * statistics.median(tv) if tv else None, "six_values_ms_all": [1e3 * x for x in tv]}
        rows.append(row)
        print("n=%5d (order %5d): value + gradient %s ms; 6 x value %s ms%s" % (
            n, 2 * n, "%.3f" % row["grad_ms"] if tg else "-", "%.3f" % row["six_values_ms"] if tv else "-",
            "; ratio %.2f" % (row["six_values_ms"] / row["grad_ms"]) if tg and tv else ""), flush=True)
    print(json.dumps({"joint_grad_bench": rows}))


if __name__ == "__main__":
    main()
