"""CPU: what the compiler makes of the one-workgroup kernels (gp_amd/csrc/small_kernels.hip).  They live at the register cap:
the figures below are the invariants their comments state (256 registers, no AGPR traffic around factor16's DPP chain) and the
scratch they had before their shared steps were stated once -- a helper that changes what the compiler hoists moves them.  All
tests read ONE compilation of the source (device code only; minutes)."""
import os
import re

import pytest

from kernel_resources import resource_usage

# scratch bytes per lane of every one-workgroup kernel before the shared steps became helpers (same compiler, same flags)
SCRATCH_BOUND = {
    "k_logml_small": 80,
    "k_logml_small_batch": 88,
    "k_logml_small_batch_ard": 88,
    "k_logml_small_batch_dev": 88,
    "k_logml_grad_small": 4872,
    "k_logml_grad_small_batch": 4904,
    "k_sample_derivs_small_batch": 84,
    "k_gp_condition_small": 84,
    "k_gp_predict_small": 84,
    "k_exact_gp_small": 84,
    "k_exact_gp_vjp_small": 3844,
    "k_latent_gp_small": 3824,
    "k_centered_gp_small": 4036,
    "k_rbf_cov_chol_small": 164,
    "k_potrf_small": 100,
}

_KERNELS = None


def small_kernels():
    """{kernel name: figures} of small_kernels.hip, compiled once per session."""
    global _KERNELS
    if _KERNELS is None:
        from gp_amd import _build
        raw = resource_usage(os.path.join(_build.CSRC, "small_kernels.hip"), "small_kernels.o", device_only=True)
        _KERNELS = {}
        for sym, v in raw.items():
            mm = re.match(r"_ZN12_GLOBAL__N_1(\d+)", sym)   # anonymous namespace: <length><name>E<arguments>
            _KERNELS[sym[mm.end():mm.end() + int(mm.group(1))] if mm else sym] = v
    return _KERNELS


def test_one_workgroup_kernel_needs_no_more_scratch_than_the_plain_vjp():
    """k_latent_gp_small shares the body of k_exact_gp_vjp_small and inherits its spills; the head must not add to them.  Both
    numbers come from one compilation of small_kernels.hip (device code only; several minutes)."""
    kernels = small_kernels()
    new = [v for k, v in kernels.items() if "k_latent_gp_small" in k]
    old = [v for k, v in kernels.items() if "k_exact_gp_vjp_small" in k]
    assert len(new) == 1 and len(old) == 1, list(kernels)
    print("scratch bytes/lane: k_latent_gp_small %d, k_exact_gp_vjp_small %d; VGPRs spilled %d, %d" % (
        new[0]["ScratchSize [bytes/lane]"], old[0]["ScratchSize [bytes/lane]"], new[0]["VGPRs Spill"], old[0]["VGPRs Spill"]))
    assert new[0]["ScratchSize [bytes/lane]"] <= old[0]["ScratchSize [bytes/lane]"], (new, old)


def test_every_one_workgroup_kernel_is_measured():
    small = sorted(k for k in small_kernels() if "_small" in k)
    assert small == sorted(SCRATCH_BOUND), small


@pytest.mark.parametrize("name", sorted(SCRATCH_BOUND))
def test_one_workgroup_kernels_stay_inside_256_registers_without_agprs(name):
    """The dynamic-LDS comment's invariant: allocated like k_gemm_nt<0> -- at most 256 VGPRs and no AGPR copies, which would
    break the hazard spacing of factor16's hand-scheduled DPP chain."""
    v = small_kernels()[name]
    print(name, v)
    assert v["AGPRs"] == 0, v
    assert v["VGPRs"] <= 256, v


@pytest.mark.parametrize("name", sorted(SCRATCH_BOUND))
def test_one_workgroup_kernels_need_no_more_scratch_than_before(name):
    """Measured after the split (bytes per lane, before -> after): k_gp_condition_small 84 -> 80, k_gp_predict_small 84 -> 80,
    k_latent_gp_small 3824 -> 3820, k_logml_grad_small 4872 -> 4848, every other kernel unchanged.  The move into a translation
    unit of its own is not neutral by itself: the blocked kernels' calls of potrf_diag4_body / gemm_tile are no longer in the same
    file, interprocedural constant propagation sees another set of call sites, and every kernel that inlines those bodies is
    scheduled and allocated anew (predict and latent came out at 88 and 3840 until each got one more thread-index barrier)."""
    v = small_kernels()[name]
    print(name, v)
    assert v["ScratchSize [bytes/lane]"] <= SCRATCH_BOUND[name], (v, SCRATCH_BOUND[name])
