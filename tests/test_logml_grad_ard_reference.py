"""CPU: what tests/test_gpu_logml_grad_dev.py rests on.  The long-double and float64 references at every ARD grid point the GPU
tests compare with a reference (tests/logml_grad_ard_grids.py): cond_2(S) <= COND_MAX and the float64 value within HALF of each
bound of logml_grad_reference.bounds, as tests/test_logml_grad_reference.py asks of the single-call inputs.  The compiler's
figures of k_logml_grad_batch_dev (its name keeps it out of the table of tests/test_small_kernels_build.py, the criteria are
that file's).  And the four entry points in the library, the binding and the header."""
import os
import re
import subprocess

import numpy as np
import pytest

import logml_grad_ard_grids as ag
import logml_grad_reference as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gpmi_logml_grad_dev", "gpmi_logml_grad_grid_dev", "gpmi_logml_grad_grid_ard", "gpmi_logml_grad_grid_ard_dev")


@pytest.mark.parametrize("name,k,jitter", ag.checked_points(), ids=lambda v: str(v))
def test_float64_against_long_double_at_the_grid_points(name, k, jitter):
    n = ag.GRIDS[name][0][0]
    ref, cond = ag.point_reference(name, k, jitter)
    r64, _ = ag.point_reference(name, k, jitter, False)
    assert cond <= lg.COND_MAX, cond
    es, eq, eg = lg.errors(r64["out3"], r64["grad"], ref)
    bs, bq, bg = lg.bounds(ref, cond, n)
    rg = eg / np.where(bg > 0, bg, 1.0)
    print("%s point %d jitter %g: cond %.1e; float64 error / the device's bound: sum_log %.3f, z'z %.3f, grad %.3f (theta %d of %d)"
          % (name, k, jitter, cond, es / bs, eq / bq, rg.max(), int(np.argmax(rg)), rg.size))
    assert ref["grad"].shape == (ag.GRIDS[name][0][1] + 2,)
    assert es <= 0.5 * bs, es / bs
    assert eq <= 0.5 * bq, eq / bq
    assert np.all(eg <= 0.5 * bg), rg
    assert np.all(np.isfinite(ref["grad"].astype(float)))


@pytest.mark.parametrize("case", [c for c in ag.ONE_WG_SINGLE + ag.CHAIN_SINGLE if c not in lg.PARITY_CASES], ids=lg.case_id)
def test_float64_against_long_double_at_the_single_cases(case):
    """The single evaluations that tests/test_logml_grad_reference.py does not already cover."""
    _, ref, cond = lg.parity_reference(case)
    _, r64, _ = lg.parity_reference(case, False)
    assert cond <= lg.COND_MAX, cond
    es, eq, eg = lg.errors(r64["out3"], r64["grad"], ref)
    bs, bq, bg = lg.bounds(ref, cond, case[0])
    assert es <= 0.5 * bs and eq <= 0.5 * bq and np.all(eg <= 0.5 * bg), (es / bs, eq / bq, eg / bg)
    assert {c[3] for c in ag.ONE_WG_SINGLE + ag.CHAIN_SINGLE} >= {0.0, 1e-3}


def test_grids_are_as_specified():
    for name, (case, G, bad, jitters, pts) in ag.GRIDS.items():
        a, E, s = ag.grid_points(name)
        assert a.shape == (G,) and E.shape == (G, case[1]) and s.shape == (G,)
        keep = np.ones(G, bool)
        if bad is not None:
            assert bad not in pts and 0 < bad < G - 1 and 0.0 in jitters
            assert np.all(E[bad] == ag.BAD_ELL) and s[bad] == ag.BAD_SIGMA
            keep[bad] = False
        assert np.all((a[keep] >= 0.8) & (a[keep] <= 1.2)) and np.all((E[keep] >= 0.6) & (E[keep] <= 1.0))
        assert np.all((s[keep] >= 0.05) & (s[keep] <= 0.25))
        assert all(np.array_equal(u, v) for u, v in zip(ag.grid_points(name), (a, E, s)))
    G = ag.GRIDS["n21-D8-dup"][1]
    assert G == ag.PTS_PER_LAUNCH + 1 and {ag.PTS_PER_LAUNCH - 1, ag.PTS_PER_LAUNCH} <= set(ag.GRIDS["n21-D8-dup"][4])
    src = open(os.path.join(ROOT, "gp_amd", "csrc", "gpmi_internal.h")).read()
    assert re.search(r"#define GPMI_SMALL_GRAD_DEV_PTS (\d+)", src).group(1) == str(ag.PTS_PER_LAUNCH)


def test_ard_gradient_kernel_stays_inside_the_one_workgroup_budget():
    """One kernel of the name; allocated like its siblings (256 registers, no AGPR copies around factor16's DPP chain); and the
    body inlined once more needs no more scratch than in k_logml_grad_small_batch, in the same compilation."""
    from test_small_kernels_build import small_kernels
    kernels = small_kernels()
    new = [v for k, v in kernels.items() if k == "k_logml_grad_batch_dev"]
    old = [v for k, v in kernels.items() if k == "k_logml_grad_small_batch"]
    assert len(new) == 1 and len(old) == 1, sorted(kernels)
    print("k_logml_grad_batch_dev", new[0], "k_logml_grad_small_batch", old[0])
    assert new[0]["AGPRs"] == 0, new[0]
    assert new[0]["VGPRs"] <= 256, new[0]
    assert new[0]["ScratchSize [bytes/lane]"] <= old[0]["ScratchSize [bytes/lane]"], (new[0], old[0])


def test_the_four_entry_points_are_exported_and_bound():
    import gp_amd
    from gp_amd import _build, _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _build.build()]).decode()
    exported = set(re.findall(r" T (gpmi_[A-Za-z0-9_]+)", out))
    assert set(NEW_SYMBOLS) <= exported, set(NEW_SYMBOLS) - exported
    assert set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
    for name in NEW_SYMBOLS:
        assert callable(getattr(gp_amd.Context, name[len("gpmi_"):])), name
