"""CPU: the trailing update's tile walks and launch plan (gp_amd/csrc/syrk_walk.h) swept by a host program, and the path classes
the shapes of tests/test_gpu_multiround.py reach.

tests/syrk_walk_host.cpp includes the header the library is built from and is compiled with the host compiler.  `sweep` runs
T = 1 .. 40 tile rows, every TN <= T, last-row heights and last-column widths {1, 64, 65, 128}, K in {128, 130, 1024},
slots in {8, 16, 24, 40, 512}, syrk_order {0, 2}, ksplit {0, 1}, ksplit_max {0, 8, 100}, fuse_diag {0, 2, 8, 15}, lanes on and
off, a diagonal block offered or not (37 million plans, under a second).  It asserts that both walks enumerate every tile of the
triangle / trapezoid exactly once, and of each plan what the kernel relies on: the grid size that goes with the split, a partial
round to divide by in the band walk, sub-tile blocks only for a tile (0, 0) wholly inside C that is not a quadrant tile as well,
and the fused-block flag only where tile (0, 0) is multiplied whole by block 0 or by the sub-tile blocks.

Not covered: k_gemm_nt<1> decodes its block index in the kernel itself (moving that decode into a shared function changed the
kernel's machine code), so the program cannot walk the blocks of a grid and count the quadrants each one multiplies; the
elementwise GPU tests of tests/test_gpu_multiround.py are the check of that part.
"""
import subprocess

import multiround_shapes as ms


def test_walks_and_plans_hold_their_invariants_over_the_sweep():
    r = subprocess.run([ms.host_program(), "sweep"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " 0 violations" in r.stdout


def _key(c):
    return (c["walk"], c["multi"], c["tail"], c["thin"], c["fused"], c["shape"])


def test_the_shape_table_reaches_every_path_class():
    """Every class of a multi-round launch under BOTH walks -- quadrant tail and none, thin last row and none, the fused diagonal
    block and none, triangle and trapezoid -- and the single-round launch with and without its sub-tiled diagonal block."""
    seen = set()
    for route in ms.ROUTES:
        for c in ms.classes(route).values():
            seen.add(_key(c))
    for k in sorted(seen):
        print("walk=%s multi=%s tail=%s thin=%s fused=%s shape=%s" % k)

    def reached(**want):
        names = ("walk", "multi", "tail", "thin", "fused", "shape")
        return any(all(k[names.index(n)] == v for n, v in want.items()) for k in seen)

    for walk in ("0", "2"):
        for want in ({"tail": "1"}, {"tail": "0"}, {"thin": "1"}, {"thin": "0"}, {"fused": "multi"}, {"fused": "none"},
                     {"shape": "tri"}, {"shape": "trap"}, {"tail": "1", "thin": "1"}, {"tail": "1", "shape": "trap"},
                     {"thin": "1", "shape": "trap", "fused": "multi"}):
            assert reached(walk=walk, multi="1", **want), (walk, want)
    # the sub-tiled diagonal block: single-round launches, and multi-round row-major ones when bit 1 is off
    assert reached(walk="0", multi="0", fused="single") and reached(walk="0", multi="0", fused="none")
    assert reached(walk="0", multi="1", fused="single")
    assert not reached(walk="2", multi="0")


def test_the_yardstick_route_is_single_round_and_the_others_are_not():
    """... and the count of multi-round updates the GPU tests expect of gpmi_kernel_timing_ex is the planner's."""
    assert all(c["multi"] == "0" and c["walk"] == "0" for c in ms.classes(ms.YARDSTICK).values())
    for route in ms.ROUTES:
        cl = ms.classes(route)
        for label in ms.calls():
            want = sum(c["multi"] == "1" for (lab, _), c in cl.items() if lab == label)
            assert ms.multi_round_updates(route, label) == want, (route, label)
            if not ms.options(route)["debug_ncu"]:
                assert want == 0, (route, label)
            elif ms.options(route) == dict(ms.DEFAULTS, debug_ncu=8, nb_outer=128, syrk_order=ms.options(route)["syrk_order"]):
                assert cl[(label, 0)]["multi"] == "1", (route, label)   # 16 slots, K = 128: every call starts multi-round
        if ms.options(route)["debug_ncu"]:   # the other routes: not every call (769 at nb_outer = 256 is 15 tiles on 16 slots)
            assert all(ms.multi_round_updates(route, "potrf-%d" % n) > 0 for n in (1228, 1345)), route


def test_no_two_routes_agree_on_every_update():
    sig = {}
    for route in ms.ROUTES:
        s = tuple(sorted((k, _key(c)) for k, c in ms.classes(route).items()))
        assert s not in sig, (route, sig[s])
        sig[s] = route


def test_the_same_sums_routes_multiply_whole_tiles_only():
    """The routes tests/test_gpu_multiround.py compares bit for bit: nothing fused, no quadrants, on every update of the
    factorisations compared (gpmi_potrf; the band walk still takes a thin last row as quadrants, so those orders are left out
    there)."""
    for route in ms.SAME_SUMS:
        cl = ms.classes(route)
        for n in ms.SAME_SUMS_N:
            walks = set()
            for (label, i), c in cl.items():
                if label == "potrf-%d" % n:
                    assert c["tail"] == "0" and c["thin"] == "0" and c["fused"] == "none", (route, label, i, c)
                    walks.add(c["walk"])
            o = ms.options(route)
            assert walks == ({"0", "2"} if o["syrk_order"] == 2 and o["debug_ncu"] else {"0"}), (route, n, walks)
