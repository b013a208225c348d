"""The Hermite-eigenfunction low-rank GP beside the exact one, on the product library: microseconds per call of
gpmi_lowrank_logml_grad (host-buffer form, and the _dev form enqueued back to back on resident data) and of
gpmi_lowrank_latent_lp_grad for both heads, and gpmi_logml_grad (D = 1) at the n the exact path can hold, in the same run.
Host-buffer calls end in their own synchronise; a _dev window is `calls` enqueues and one synchronise.  Every shape is warmed up
first; the contenders of a shape alternate in windows of at least --window seconds and the median over the rounds is reported.

The rate column counts the f64 MFMA flops the Gram kernel actually ISSUES -- every 16 x 16 x 4 instruction of every lower tile
pair (three per pair and step: G and the two halves of S), padded columns and padded rows included, 2048 flops each -- over the
time of the whole _dev call (Gram kernel + finishing kernel): a lower bound on the Gram kernel's own rate, not a kernel time.

    python tools/lowrank_bench.py [--window 0.5] [--rounds 3] [--quick]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402

MARGINAL = ((1438, 10), (1438, 40), (16384, 64), (1000000, 10), (1000000, 128))
EXACT = (1438, 16384)
LATENT = ((1438, 10),)
SCALE, AMP, L, SIGMA = 0.25, 1.3, 0.3, 0.35


def inputs(n, M):
    rng = np.random.default_rng(9000 + n + M)
    x = np.sort(rng.uniform(-0.5, 0.5, n))
    y = np.sin(3 * x) + 0.3 * rng.standard_normal(n)
    return x, y, rng.standard_normal(M), (rng.uniform(size=n) < 0.5).astype(float)


def issued_mfma_flops(n, M):
    """The chunk rule and sub-block sizes of csrc/lowrank_kernels.hip (lr_gram_rows, LrGram)."""
    mt = (M + 15) // 16
    rb = 256 if mt <= 2 else (128 if mt <= 4 else 64)
    rows = -(-(-(-n // 256)) // rb) * rb
    pairs = mt * (mt + 1) // 2
    steps = 0
    for r0 in range(0, n, rows):
        steps += -(-(min(n, r0 + rows) - r0) // rb) * (rb // 4)
    return steps * pairs * 3 * 2048.0


def window(fn, seconds, sync=None):
    calls = 0
    t0 = time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 16 == 0 or sync is None:
            if sync is not None:
                sync()
            dt = time.perf_counter() - t0
            if dt >= seconds and calls >= 2:
                return dt / calls


def median_us(fns, seconds, rounds, syncs):
    for k, fn in fns.items():
        fn()
        if syncs.get(k):
            syncs[k]()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, seconds, syncs.get(k)))
    return {k: 1e6 * statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="skip n = 1e6 and the exact call at n = 16384")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    ctx = gp_amd.Context(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    rows = []
    for n, M in MARGINAL:
        if args.quick and n > 20000:
            continue
        x, y, _, _ = inputs(n, M)
        dx, dy = up(x), up(y)
        o = torch.zeros(8, dtype=torch.float64, device=dev)
        di = torch.zeros(1, dtype=torch.int32, device=dev)
        fns = {"host": lambda: ctx.lowrank_logml_grad(x, y, M, SCALE, AMP, L, SIGMA),
               "dev": lambda: ctx.lowrank_logml_grad_dev(dx.data_ptr(), n, dy.data_ptr(), M, SCALE, AMP, L, SIGMA, o.data_ptr(),
                                                         o.data_ptr() + 24, di.data_ptr())}
        us = median_us(fns, args.window, args.rounds, {"dev": ctx.sync})
        fl = issued_mfma_flops(n, M)
        row = {"call": "lowrank_logml_grad", "n": n, "M": M, "host_us": us["host"], "dev_us": us["dev"], "mfma_flops_issued": fl,
               "tflops_issued_over_dev_call": fl / us["dev"] * 1e-6}
        rows.append(row)
        print("lowrank_logml_grad n=%7d M=%3d: host %.0f us, _dev %.0f us, %.2f TFLOP/s issued over the _dev call" % (
            n, M, us["host"], us["dev"], row["tflops_issued_over_dev_call"]), flush=True)
    for n, M in LATENT:
        x, _, z, yb = inputs(n, M)
        y = np.sin(3 * x)
        dx, dz, dyb, dyn = up(x), up(z), up(yb), up(y)
        o = torch.zeros(8 + M, dtype=torch.float64, device=dev)
        for fam, Yh, Yd in (("normal", y, dyn), ("bernoulli_logit", yb, dyb)):
            fns = {"host": lambda: ctx.lowrank_latent_lp_grad(x, M, SCALE, AMP, L, z, fam, Yh, SIGMA, want_q=False),
                   "dev": lambda: ctx.lowrank_latent_lp_grad_dev(dx.data_ptr(), n, M, SCALE, AMP, L, dz.data_ptr(), fam, Yd.data_ptr(), 1, n,
                                                                 SIGMA, o.data_ptr(), None, None, o.data_ptr() + 64, o.data_ptr() + 32)}
            us = median_us(fns, args.window, args.rounds, {"dev": ctx.sync})
            rows.append({"call": "lowrank_latent_lp_grad", "head": fam, "n": n, "M": M, "host_us": us["host"], "dev_us": us["dev"]})
            print("lowrank_latent_lp_grad n=%d M=%d %s: host %.0f us, _dev %.0f us" % (n, M, fam, us["host"], us["dev"]), flush=True)
    for n in EXACT:
        if args.quick and n > 2000:
            continue
        x, y, _, _ = inputs(n, 0)
        X = x[:, None]
        dX, dy = up(x), up(y)
        o = torch.zeros(8, dtype=torch.float64, device=dev)
        di = torch.zeros(1, dtype=torch.int32, device=dev)
        fns = {"host": lambda: ctx.logml_grad(X, y, AMP, [L], SIGMA, 0.0),
               "dev": lambda: ctx.logml_grad_dev(dX.data_ptr(), n, n, 1, dy.data_ptr(), AMP, [L], SIGMA, 0.0, o.data_ptr(), o.data_ptr() + 24,
                                                 di.data_ptr())}
        us = median_us(fns, args.window, args.rounds, {"dev": ctx.sync})
        rows.append({"call": "logml_grad", "n": n, "D": 1, "host_us": us["host"], "dev_us": us["dev"]})
        print("logml_grad (exact, D=1) n=%d: host %.0f us, _dev %.0f us" % (n, us["host"], us["dev"]), flush=True)
    print(json.dumps({"lowrank_bench": rows}))


if __name__ == "__main__":
    main()
