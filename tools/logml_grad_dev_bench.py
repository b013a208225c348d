"""The forms of the log-ml gradient that the device finishes itself, beside the host forms they extend.

  * gpmi_logml_grad (host buffers: X, y up, one synchronisation, the results down) against gpmi_logml_grad_dev on torch
    tensors (enqueue only; the window ends in ONE synchronisation, as a caller whose next kernel consumes the gradient sees it),
    D = 3, default options;
  * gpmi_logml_grad_grid_ard at G ARD points in one call against G gpmi_logml_grad calls.

Every shape is warmed up first; the contenders alternate in the same process in windows of at least --window seconds, and the
median over the rounds is reported.  Runs on libgpmi.so (no probes).

    python tools/logml_grad_dev_bench.py [--sizes 21,128,1438,4096] [--grid 100,3,16] [--window 0.3] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_amd  # noqa: E402

SIZES = (21, 128, 1438, 4096)   # R/tests.R, the one-workgroup limit, westbrook.R, the blocked chains
D = 3
ALPHA, SIGMA, JITTER = 1.1, 0.1, 1e-6


def inputs(n, d):
    """About one point per length-scale: X = U(0, 1)^d * 0.8 n^(1/d)."""
    rng = np.random.default_rng(7000 + 10 * n + d)
    X = rng.random((n, d)) * (0.8 * n ** (1.0 / d))
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(d)) + 0.1 * rng.standard_normal(n)
    return np.asfortranarray(X), y, 0.6 + 0.4 * rng.random(d)


def window(fn, seconds, end=None):
    """Seconds per call of fn over a window of at least `seconds` (at least two calls); `end` runs once, inside the window."""
    calls = 0
    t0 = time.perf_counter()
    while True:
        fn()
        calls += 1
        if time.perf_counter() - t0 >= seconds and calls >= 2:
            if end:
                end()
            return (time.perf_counter() - t0) / calls


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--grid", default="100,3,16", help="n,D,G of the ARD grid")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = gp_amd.Context(0)
    rows = []
    for n in (int(s) for s in args.sizes.split(",") if s):
        X, y, ell = inputs(n, D)
        dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
        dy = torch.from_numpy(y).to(dev)
        do = torch.zeros(3, dtype=torch.float64, device=dev)
        dg = torch.zeros(2 + D, dtype=torch.float64, device=dev)
        di = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def host():
            return ctx.logml_grad(X, y, ALPHA, ell, SIGMA, JITTER)

        def device():
            ctx.logml_grad_dev(dX.data_ptr(), n, n, D, dy.data_ptr(), ALPHA, ell, SIGMA, JITTER, do.data_ptr(), dg.data_ptr(), di.data_ptr())

        out, g = host()
        device()
        ctx.sync()
        assert int(di.item()) == 0 and np.array_equal(dg.cpu().numpy(), g) and np.array_equal(do.cpu().numpy(), out), n
        th, td = [], []
        for _ in range(args.rounds):
            th.append(window(host, args.window))
            td.append(window(device, args.window, ctx.sync))
        row = {"n": n, "D": D, "host_us": 1e6 * statistics.median(th), "dev_us": 1e6 * statistics.median(td),
               "host_us_all": [1e6 * v for v in th], "dev_us_all": [1e6 * v for v in td]}
        rows.append(row)
        print("n=%5d D=%d: gpmi_logml_grad %.1f us; gpmi_logml_grad_dev %.1f us per call (enqueued back to back)"
              % (n, D, row["host_us"], row["dev_us"]), flush=True)
    n, d, G = (int(v) for v in args.grid.split(","))
    X, y, ell = inputs(n, d)
    rng = np.random.default_rng(16)
    A, E, S = 0.8 + 0.4 * rng.random(G), 0.6 + 0.4 * rng.random((G, d)), 0.05 + 0.2 * rng.random(G)

    def grid():
        return ctx.logml_grad_grid_ard(X, y, A, E, S, JITTER)

    def singles():
        return [ctx.logml_grad(X, y, A[k], E[k], S[k], JITTER) for k in range(G)]

    out, g, info = grid()
    one = singles()
    assert np.all(info == 0) and all(np.array_equal(g[k], one[k][1]) for k in range(G))
    tg, ts = [], []
    for _ in range(args.rounds):
        tg.append(window(grid, args.window))
        ts.append(window(singles, args.window))
    grid_row = {"n": n, "D": d, "G": G, "grid_us": 1e6 * statistics.median(tg), "singles_us": 1e6 * statistics.median(ts),
                "grid_us_all": [1e6 * v for v in tg], "singles_us_all": [1e6 * v for v in ts]}
    print("ARD grid n=%d D=%d G=%d: gpmi_logml_grad_grid_ard %.1f us; %d x gpmi_logml_grad %.1f us"
          % (n, d, G, grid_row["grid_us"], G, grid_row["singles_us"]), flush=True)
    print(json.dumps({"logml_grad_dev_bench": rows, "ard_grid": grid_row}))


if __name__ == "__main__":
    main()
