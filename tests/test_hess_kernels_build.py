"""CPU: gp_amd/csrc/hess_kernels.hip compiles for gfx950, its kernels are exactly the named set and none of them spills or uses
scratch (the compiler's own resource remarks)."""
import os

from kernel_resources import resource_usage

KERNELS = ("k_hess_operands", "k_hess_bsum", "k_hess_mv_part", "k_hess_mv_sum", "k_hess_dots", "k_hess_second_ard",
           "k_hess_second_iso", "k_hess_traces", "k_hess_sum", "k_hess_finish")


def test_hess_kernels_use_no_scratch():
    from gp_amd import _build
    assert "hess_kernels.hip" in _build.SOURCES
    kernels = resource_usage(os.path.join(_build.CSRC, "hess_kernels.hip"), "hess_kernels.o", device_only=True)
    for want in KERNELS:
        found = [k for k in kernels if want in k]
        assert len(found) == 1, (want, sorted(kernels))
        r = kernels[found[0]]
        print(found[0], r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (found[0], r)
    assert len(kernels) == len(KERNELS), sorted(kernels)
