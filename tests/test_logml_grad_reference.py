"""CPU: the reference of gpmi_logml_grad (tests/logml_grad_reference.py): float64 against long double on every parity input
(with the cap on cond_2 and the floor of the sum-log bound that tests/test_gpu_logml_grad_parity.py rests on), central
differences of the long-double value in every theta, the identity with the centred reference, the exact zero of d/dsigma at
sigma = 0, and the conditions on the parity inputs: the rotation covers what it has to, and the D > 8 matrices are not nearly
diagonal."""
import numpy as np
import pytest

import centered_gp_reference as cg
import logml_grad_reference as lg

LD = np.longdouble


@pytest.mark.parametrize("case", lg.PARITY_CASES, ids=lg.case_id)
def test_float64_against_long_double(case):
    """cond <= COND_MAX, and the float64 restatement within HALF of every bound the device gets (for sum_log that is what
    SUM_LOG_FLOOR_C is chosen by): a reference that used its bound up would leave the device none."""
    n = case[0]
    _, ref, cond = lg.parity_reference(case)
    _, r64, _ = lg.parity_reference(case, False)
    assert cond <= lg.COND_MAX, cond
    es, eq, eg = lg.errors(r64["out3"], r64["grad"], ref)
    bs, bq, bg = lg.bounds(ref, cond, n)
    rg = eg / np.where(bg > 0, bg, 1.0)
    print("%s: cond %.1e; float64 error / the device's bound: sum_log %.3f, z'z %.3f, grad %.3f (theta %d of %d)"
          % (lg.case_id(case), cond, es / bs, eq / bq, rg.max(), int(np.argmax(rg)), rg.size))
    assert es <= 0.5 * bs, es / bs
    assert eq <= 0.5 * bq, eq / bq
    assert np.all(eg <= 0.5 * bg), rg
    assert np.all(np.isfinite(ref["grad"].astype(float)))


def test_floor_constant_is_the_smallest_power_of_two():
    """With half of SUM_LOG_FLOOR_C the float64 value leaves half of the bound on some parity input (the one whose logs cancel)."""
    worst = 0.0
    for case in lg.PARITY_CASES:
        n = case[0]
        _, ref, cond = lg.parity_reference(case)
        _, r64, _ = lg.parity_reference(case, False)
        es = lg.errors(r64["out3"], r64["grad"], ref)[0]
        half = 10.0 * cond * lg.EPS * abs(float(ref["out3"][1])) + 0.5 * lg.SUM_LOG_FLOOR_C * n * lg.EPS
        worst = max(worst, es / (0.5 * half))
    print("with c / 2: the worst float64 sum_log error is %.2f of half the bound" % worst)
    assert worst > 1.0
    c = lg.SUM_LOG_FLOOR_C
    assert c > 0 and 2.0 ** round(np.log2(c)) == c


@pytest.mark.parametrize("n,D", [(21, 3), (40, 17)])
def test_gradient_equals_central_differences_of_the_long_double_value(n, D):
    """The formulas, not the arithmetic: every theta (alpha, each ell_d, sigma), ARD, both coordinate layouts."""
    X, y, a, ell, s, jit = lg.case_inputs(n, D, True, 0.15)
    th = np.concatenate([[a], ell, [s]]).astype(LD)

    def f(p):
        return lg.logml_grad_reference(X, y, p[0], p[1:-1], p[-1], jit, LD)["out3"][0]

    g = lg.logml_grad_reference(X, y, a, ell, s, jit, LD)["grad"]
    h = LD(1e-6)   # truncation h^2 f''' / 6 ~ 1e-12 relative; rounding 1e-19 |f| / h ~ 1e-11 absolute
    fd = np.array([(f(th + h * e) - f(th - h * e)) / (2 * h) for e in np.eye(th.size, dtype=LD)])
    err = float(np.max(np.abs(g - fd)) / np.max(np.abs(g)))
    print("n %d D %d: max|g - fd| / max|g| = %.2e" % (n, D, err))
    assert err <= 1e-9, (g, fd)


@pytest.mark.parametrize("case", [(21, 1, False, 0.15, ""), (40, 3, True, 1e-3, ""), (33, 17, True, 0.0, "")], ids=lg.case_id)
@pytest.mark.parametrize("dtype", [float, LD], ids=["float64", "longdouble"])
def test_equals_the_centred_reference_without_a_head(case, dtype):
    X, y, a, ell, s, jit = lg.case_inputs(*case)
    ref = lg.logml_grad_reference(X, y, a, ell, s, jit, dtype)
    cen = cg.centered_reference(X, a, ell, y[:, None], "none", jitter=dtype(s) * dtype(s) + dtype(jit), dtype=dtype)
    tol = 64 * float(np.finfo(dtype).eps)
    assert abs(float((ref["out3"][1] - cen["sum_log_diag"]) / cen["sum_log_diag"])) <= tol
    assert abs(float((ref["out3"][2] - cen["quad"]) / cen["quad"])) <= tol
    prior = ref["out3"][0] + len(y) * np.log(2 * dtype(np.pi)) / 2   # the `~` constant that the centred prior drops
    assert abs(float(prior - cen["prior"])) <= (tol if dtype is float else 1e-15) * abs(float(cen["prior"]))
    # the same contraction term by term: only the order of the sums differs
    assert np.all(np.abs(ref["grad"][:-1] - cen["grad"]).astype(float) <= tol * ref["gabs"][:-1])
    np.testing.assert_allclose(ref["gabs"][:-1], cen["gabs"], rtol=1e-12)
    A = cen["A"][:, 0]
    Sinv = np.linalg.inv(np.asarray(lg.vr.se_cov(X, a, ell, s * s + jit)[0], float))
    want = s * (float(A @ A) - np.trace(Sinv))
    assert abs(float(ref["grad"][-1]) - want) <= 1e-9 * max(abs(want), float(ref["gabs"][-1]))


@pytest.mark.parametrize("dtype", [float, LD], ids=["float64", "longdouble"])
def test_zero_noise_gives_an_exactly_zero_sigma_component(dtype):
    for case in lg.PARITY_CASES:
        if case[3] == 0.0 and case[0] <= 129:
            r = lg.logml_grad_reference(*lg.case_inputs(*case), dtype=dtype)
            assert r["grad"][-1] == 0.0 and r["gabs"][-1] == 0.0, case
            assert np.all(np.isfinite(r["grad"].astype(float)))


def test_case_inputs_are_deterministic_and_as_specified():
    a = lg.case_inputs(65, 17, True, 1e-3)
    b = lg.case_inputs(65, 17, True, 1e-3)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    X, y, alpha, ell, sigma, jit = a
    assert X.shape == (65, 17) and y.shape == (65,) and ell.shape == (17,) and (alpha, sigma, jit) == (1.3, 1e-3, 1e-6)
    assert np.all((ell >= 0.6) & (ell <= 1.0))
    assert np.array_equal(lg.case_inputs(65, 3, False, 0.0)[3], [0.8])
    X, *_ = lg.case_inputs(65, 3, True, 0.15, "dup")
    assert np.array_equal(X[-lg.DUP:], X[:lg.DUP])
    assert np.sum(lg.scaled_sq_dist(X, lg.case_inputs(65, 3, True, 0.15, "dup")[3]) == 0.0) == lg.DUP
    _, ref, cond = lg.parity_reference(lg.CANCEL_CASE)
    assert abs(float(ref["out3"][1])) <= 4 * lg.EPS and 5 <= cond <= 20   # the logs cancel: what the floor is for


def test_rotation_covers_every_layout_on_every_route():
    small = {(D, ard) for D in (1, 2, 3, 5, 8) for ard in (False, True)}
    big = {(D, ard) for D in (9, 16, 17, 33, 64) for ard in (False, True)}
    one = [c for c in lg.ONE_WG_CASES if not c[4]]
    chain = [c for c in lg.CHAIN_CASES if not c[4]]
    assert {c[0] for c in one} == set(lg.ONE_WG_SIZES) and {(c[1], c[2]) for c in one} == small
    assert {c[0] for c in chain} == set(lg.CHAIN_SIZES) and {(c[1], c[2]) for c in chain} == small | big
    assert (256, 8) in {(c[0], c[1]) for c in one}   # the LDS coordinate buffers at their largest
    for D in (9, 16, 17, 33, 64):
        assert any(c[1] == D and c[0] % 64 for c in chain), D
    for cases in (one, chain):
        assert {c[3] for c in cases} == set(lg.SIGMAS)
    for cases in (lg.ONE_WG_CASES, lg.CHAIN_CASES):
        assert [c for c in cases if c[4] == "dup" and c[0] == 65 and c[3] == 0.15]
    assert any(c[4] == "dup" and c[1] > 8 for c in lg.CHAIN_CASES)
    assert len(lg.PARITY_CASES) <= 60   # rotated, not the cross product


def test_big_D_inputs_are_not_nearly_diagonal():
    """D > 8: the median scaled squared distance lies in [1, 6] (the D <= 8 layout at D = 64 gives cond 1.5)."""
    seen = 0
    for case in lg.PARITY_CASES:
        n, D = case[0], case[1]
        if D > 8 and n > 1:
            X, _, _, ell, _, _ = lg.case_inputs(*case)
            med = float(np.median(lg.scaled_sq_dist(X, ell)))
            assert 1.0 <= med <= 6.0, (case, med)
            seen += 1
    assert seen >= 10
