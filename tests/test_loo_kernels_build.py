"""CPU: gp_amd/csrc/loo_kernels.hip compiles for gfx950 and none of its kernels spills (the compiler's own resource remarks)."""
import os

from kernel_resources import resource_usage

KERNELS = ("k_loo_points", "k_loo_tiles", "k_loo_bsum", "k_loo_grad_finish")


def test_loo_kernels_use_no_scratch():
    from gp_amd import _build
    kernels = resource_usage(os.path.join(_build.CSRC, "loo_kernels.hip"), "loo_kernels.o", device_only=True)
    for want in KERNELS:
        found = [k for k in kernels if want in k]
        assert len(found) == 1, (want, sorted(kernels))
        r = kernels[found[0]]
        print(found[0], r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (found[0], r)
    assert len(kernels) == len(KERNELS), sorted(kernels)
