"""CPU: gp_amd/csrc/chol_kernels.hip compiles for gfx950, holds the kernels it is expected to hold and none of them spills
(the compiler's own resource remarks).  The three k_gemm_nt instantiations are the update kernels: two workgroups of 256
lanes per CU (__launch_bounds__(256, 2)) leave them 256 registers a lane, and a spill there costs the trailing update its speed
without failing any test of its numbers."""
import os

from kernel_resources import resource_usage

GEMM = ("9k_gemm_ntILi0E", "9k_gemm_ntILi1E", "9k_gemm_ntILi2E")   # C -= A B^T, the SYRK walk, C = A B^T
OTHERS = ("13k_potrf_diag4E", "12k_trsm_panelE", "14k_pack_factorsE", "12k_eye_blocksE", "18k_transpose_blocksE", "11k_trsv_waveE",
          "17k_trmv_lower_partE", "16k_trmv_lower_sumE", "14k_trmv_lower_tE", "15k_logml_partialE", "16k_logml_finalizeE", "9k_get_rowE")


def test_chol_kernels_use_no_scratch():
    from gp_amd import _build
    kernels = resource_usage(os.path.join(_build.CSRC, "chol_kernels.hip"), "chol_kernels.o", device_only=True)
    for want in GEMM + OTHERS:
        found = [k for k in kernels if want in k]
        assert len(found) == 1, (want, sorted(kernels))
        r = kernels[found[0]]
        print(found[0], r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (found[0], r)
        if want in GEMM:
            assert r["VGPRs"] + r["AGPRs"] <= 256, (found[0], r)   # two workgroups of four waves per CU
    assert len(kernels) == len(GEMM) + len(OTHERS), sorted(kernels)
