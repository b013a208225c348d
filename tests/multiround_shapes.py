"""The shapes and routes of tests/test_gpu_multiround.py, and the trailing updates they launch.

A route is a set of context options; "debug_ncu" makes the trailing-update planner see that many compute units (slots = 2 x
debug_ncu workgroup slots), so that launches of a few dozen tiles take the multi-round paths that start at n > 4100 on the
device's own count.  tests/test_syrk_walk_host.py feeds every update listed here to the planner on the CPU
(tests/syrk_walk_host.cpp) and asserts that the table reaches every path class; the GPU tests run the same table.
"""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"debug_ncu": 0, "syrk_order": 2, "ksplit": 1, "fuse_diag": 15, "nb_outer": 0}
KSPLIT_MAX = 100        # gpmi_tuning_defaults; "ksplit" 0 / 1 leaves it
DEVICE_SLOTS = 512      # 2 x 256 compute units: what debug_ncu = 0 plans for on an MI355X

# gpmi_potrf at these orders.  With nb_outer = 128 the first update has M = n - 128:
#   769   6 tile rows, the last one of ONE row (thin)        833   last row of 65        896   last row of 128 (full)
#   1228  9 tile rows: two bands of the band walk            1345  10 tile rows
POTRF_N = (769, 833, 896, 1228, 1345)
# gpmi_logml on the chain: M = n + 1 rows over n columns -- every update is a trapezoid (T = TN + 1) that ends in a thin row
LOGML_N = (768, 1280)
# gpmi_gp_condition on the chain: n + m + 1 rows over n + m columns, the first n factored.  n + m = 1280 is the shape whose
# updates are trapezoids (T = TN + 1); the other two have T = TN and end in the Schur complement's update
COND_NM = ((300, 900), (641, 700), (300, 980))
# gpmi_logml_grid under four lanes (row-major walk whatever syrk_order says)
LANES_N = 897

YARDSTICK = "defaults"


def _route(ncu, order, ksplit, fuse, nbo):
    return {"debug_ncu": ncu, "syrk_order": order, "ksplit": ksplit, "fuse_diag": fuse, "nb_outer": nbo}


def route_id(ncu, order, ksplit, fuse, nbo):
    return "ncu%d-walk%d-ks%d-fd%d-nbo%d" % (ncu, order, ksplit, fuse, nbo)


# The routes kept are those whose path classes over the table differ (test_syrk_walk_host.py asserts that no two of them
# agree on every update, and that together they reach every class); the all-defaults route is the single-round yardstick.
ROUTES = {YARDSTICK: {}}
for _r in ((8, 2, 1, 15, 128), (8, 0, 1, 15, 128), (8, 2, 0, 0, 128), (8, 0, 0, 0, 128), (8, 2, 1, 8, 128), (8, 0, 1, 8, 128),
           (8, 2, 1, 2, 256), (8, 0, 1, 2, 256), (12, 2, 1, 15, 128), (12, 0, 1, 15, 128), (12, 2, 1, 15, 256), (12, 0, 0, 2, 256)):
    ROUTES[route_id(*_r)] = _route(*_r)
# the routes of test 2: nothing fused, no quadrants -- every element by the whole-tile routine, the walk alone differs
ROUTES[route_id(0, 2, 0, 0, 128)] = _route(0, 2, 0, 0, 128)
SAME_SUMS = (route_id(0, 2, 0, 0, 128), route_id(8, 2, 0, 0, 128), route_id(8, 0, 0, 0, 128))
SAME_SUMS_N = (833, 896, 1228, 1345)   # 769 ends every update in a thin row, which the band walk takes as quadrants


def options(route):
    o = dict(DEFAULTS)
    o.update(ROUTES[route])
    return o


def updates(M, ncol, nfac, nbo):
    """(M', N', K, diag offered) of every trailing update of launch_potrf_partial(M, ncol, nfac) at outer width nbo
    (0: the automatic width, 128 below order 3584)."""
    nbo = nbo or 128
    assert ncol < 3584
    out = []
    for ko in range(0, nfac, nbo):
        ke = min(ko + nbo, nfac)
        if ke >= M or ke >= ncol:
            continue
        out.append((M - ke, ncol - ke, ke - ko, ke < nfac))
    return out


def calls():
    """{label: (M, ncol, nfac, lanes_active)} of every factorisation the GPU tests run."""
    out = {}
    for n in POTRF_N:
        out["potrf-%d" % n] = (n, n, n, 0)
    for n in LOGML_N:
        out["logml-%d" % n] = (n + 1, n, n, 0)
    for n, m in COND_NM:
        out["cond-%d-%d" % (n, m)] = (n + m + 1, n + m, n, 0)
    out["lanes-%d" % LANES_N] = (LANES_N + 1, LANES_N, LANES_N, 1)
    return out


def multi_round_updates(route, label):
    """How many trailing updates of one call hold more tiles than the route's workgroup slots (what gpmi_kernel_timing_ex
    counts as multi-round launches); tests/test_syrk_walk_host.py holds this count to the planner's own flag."""
    o = options(route)
    slots = 2 * o["debug_ncu"] if o["debug_ncu"] else DEVICE_SLOTS
    M, ncol, nfac, _ = calls()[label]
    count = 0
    for m, n, _, _ in updates(M, ncol, nfac, o["nb_outer"]):
        T = (m + 127) // 128
        TN = min((n + 127) // 128, T)
        count += TN * (TN + 1) // 2 + (T - TN) * TN > slots
    return count


def plan_lines(route):
    """[(label, index of the update, input line of `syrk_walk_host classify`)] of one route over every call."""
    o = options(route)
    slots = 2 * o["debug_ncu"] if o["debug_ncu"] else DEVICE_SLOTS
    lines = []
    for label, (M, ncol, nfac, lanes) in calls().items():
        for i, (m, n, k, diag) in enumerate(updates(M, ncol, nfac, o["nb_outer"])):
            lines.append((label, i, "%d %d %d %d %d %d %d %d %d %d" % (m, n, k, slots, o["syrk_order"], o["ksplit"], KSPLIT_MAX,
                                                                      o["fuse_diag"], lanes, int(diag))))
    return lines


@functools.lru_cache(maxsize=None)
def host_program():
    """tests/syrk_walk_host.cpp compiled with the host compiler (as tests/test_abi.py compiles its C client)."""
    out = os.path.join(ROOT, "build", "syrk_walk_host")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "syrk_walk_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "syrk_walk_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@functools.lru_cache(maxsize=None)
def classes(route):
    """{(label, index): {"walk", "multi", "tail", "thin", "fused", "shape"}} of one route, from the planner itself."""
    lines = plan_lines(route)
    r = subprocess.run([host_program(), "classify"], input="".join(l[2] + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    out = {}
    for (label, i, _), text in zip(lines, got):
        out[(label, i)] = dict(kv.split("=") for kv in text.split())
    return out
