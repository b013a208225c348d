"""CPU: gp_amd/csrc/lowrank_kernels.hip compiles for gfx950, its kernels are exactly the named set (the Gram kernel once per
number of 16-column tiles) and none of them spills or uses scratch (the compiler's own resource remarks)."""
import os

from kernel_resources import resource_usage

KERNELS = ("k_lr_basis", "k_lr_finishILb0E", "k_lr_finishILb1E", "k_lr_latentE", "k_lr_latent_sum") + tuple("k_lr_gramILi%dE" % mt for mt in range(1, 9))


def test_lowrank_kernels_use_no_scratch():
    from gp_amd import _build
    assert "lowrank_kernels.hip" in _build.SOURCES
    kernels = resource_usage(os.path.join(_build.CSRC, "lowrank_kernels.hip"), "lowrank_kernels.o", device_only=True)
    for want in KERNELS:
        found = [k for k in kernels if want in k]
        assert len(found) == 1, (want, sorted(kernels))
        r = kernels[found[0]]
        print(found[0], r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (found[0], r)
    assert len(kernels) == len(KERNELS), sorted(kernels)
