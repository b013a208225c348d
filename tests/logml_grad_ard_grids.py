"""The ARD grids of tests/test_gpu_logml_grad_dev.py and their long-double references (helper: no test_ prefix): the data of
logml_grad_reference.case_inputs, G points (alpha, ell_0 .. ell_{D-1}, sigma) drawn per grid, and -- where a grid has one -- the
point test_gpu_grad.py::test_grad_grid_on_lanes_equals_single_calls rejects (every length-scale 50, sigma 1e-9: with jitter 0
the matrix is numerically singular) in its middle.  tests/test_logml_grad_ard_reference.py checks on the CPU every point that
the GPU tests compare with a reference."""
import functools

import numpy as np

import logml_grad_reference as lg

PTS_PER_LAUNCH = 128      # GPMI_SMALL_GRAD_DEV_PTS (gp_amd/csrc/gpmi_internal.h): points per launch of k_logml_grad_batch_dev
BAD_ELL, BAD_SIGMA = 50.0, 1e-9

# name: (case of lg.case_inputs, G, the rejected point or None, jitters, the points compared with the reference)
GRIDS = {
    "n65-D3-dup": ((65, 3, True, 0.15, "dup"), 5, 2, (0.0, 1e-6), (0, 1, 3, 4)),
    # one more point than a launch holds: first, last of the first launch, first (and last) of the second
    "n21-D8-dup": ((21, 8, True, 0.15, "dup"), PTS_PER_LAUNCH + 1, PTS_PER_LAUNCH // 2, (0.0,),
                   (0, PTS_PER_LAUNCH - 1, PTS_PER_LAUNCH)),
    "n129-D9-dup": ((129, 9, True, 0.15, "dup"), 5, 2, (0.0,), (0, 1, 3, 4)),
    "n129-D17-dup": ((129, 17, True, 0.15, "dup"), 5, 2, (0.0,), (0, 1, 3, 4)),
    # the largest one-workgroup problem, and the first size past it (the lanes at D <= 8: k_grad_partial)
    "n256-D8-ard": ((256, 8, True, 0.15, ""), 2, None, (1e-6,), (0, 1)),
    "n257-D2-ard": ((257, 2, True, 0.15, ""), 2, None, (1e-6,), (0, 1)),
}

# the single evaluations whose device-resident form is compared with the host form (and the host form with the reference)
ONE_WG_SINGLE = ((1, 1, False, 0.15, ""), (65, 3, True, 0.15, "dup"), (256, 8, True, 1e-3, ""))
CHAIN_SINGLE = ((129, 9, False, 0.0, ""), (257, 2, True, 0.15, ""), (385, 17, True, 1e-3, ""))


def grid_data(name):
    """(X, y) of the grid's case."""
    return lg.case_inputs(*GRIDS[name][0])[:2]


def grid_points(name):
    """(alpha (G,), ell (G, D), sigma (G,)): alpha = 0.8 + 0.4 u, ell = 0.6 + 0.4 u per dimension, sigma = 0.05 + 0.2 u, the
    rejected point overwritten afterwards; deterministic in the grid."""
    (n, D, _, _, _), G, bad, _, _ = GRIDS[name]
    rng = np.random.default_rng(1000 * n + D)
    a = 0.8 + 0.4 * rng.random(G)
    E = 0.6 + 0.4 * rng.random((G, D))
    s = 0.05 + 0.2 * rng.random(G)
    if bad is not None:
        a[bad], E[bad], s[bad] = 1.0, BAD_ELL, BAD_SIGMA
    return a, E, s


def checked_points():
    """Every (grid, point, jitter) that a GPU test compares with the long-double reference."""
    return [(name, k, jit) for name, (_, _, _, jitters, pts) in GRIDS.items() for jit in jitters for k in pts]


@functools.lru_cache(maxsize=None)
def point_reference(name, k, jitter, longdouble=True):
    """(reference dict, cond_2(S)) of point k of the grid, computed once per process."""
    X, y = grid_data(name)
    a, E, s = grid_points(name)
    ref = lg.logml_grad_reference(X, y, float(a[k]), E[k], float(s[k]), jitter, np.longdouble if longdouble else float)
    return ref, lg.cond2(X, float(a[k]), E[k], float(s[k]), jitter)
