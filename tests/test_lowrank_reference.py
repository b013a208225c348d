"""CPU: tests/lowrank_reference.py against itself -- the float64 recurrence (the device's algebra) against the 50-digit closed
form, the M x M identity against the n x n long-double factorisation, the gradients against long-double central differences of
the value, Phi Phi^T against the squared-exponential kernel where the expansion has converged, and the ratios that size the
bounds the GPU test uses."""
import numpy as np
import pytest

import lowrank_reference as lr

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


@pytest.mark.parametrize("case", lr.CASES + lr.BIG_CASES, ids=lambda c: "n%d_M%d_l%g" % c)
def test_float64_transcription_stays_within_half_of_every_bound(case):
    r = lr.all_ratios(case)
    print(case, " ".join("%s %.3f" % kv for kv in r.items()))
    assert max(r.values()) <= 0.5, r


@pytest.mark.parametrize("case", [(21, 10, 1.0), (65, 17, 0.3), (64, 1, 1.0), (1, 2, 0.3)], ids=lambda c: "n%d_M%d_l%g" % c)
def test_long_double_recurrence_reproduces_the_closed_form(case):
    n, M, l = case
    x = lr.case_inputs(*case)[0]
    Phi, dPhi = lr.basis_ld(x, M, lr.SCALE, lr.AMP, l)
    P, D = lr.basis_f64(x, M, lr.SCALE, lr.AMP, l, dtype=LD)
    bP, bD = lr.basis_bounds(Phi, dPhi, l)
    # the same bound with the long-double epsilon in place of 2^-52
    assert lr.worst_ratio(P, Phi, bP * EPS_LD / lr.EPS) <= 1.0
    assert lr.worst_ratio(D, dPhi, bD * EPS_LD / lr.EPS) <= 1.0


@pytest.mark.parametrize("case", [(21, 10, 1.0), (65, 17, 0.3), (3, 3, 0.3), (1, 1, 1.0)], ids=lambda c: "n%d_M%d_l%g" % c)
def test_identity_in_long_double_agrees_with_the_dense_factorisation(case):
    n, M, l = case
    (x, y, _, _), ref, rec = lr.marginal_reference(case)
    got = lr.marginal_identity(x, y, M, lr.SCALE, lr.AMP, l, lr.SIGMA, dtype=LD, basis=lr.basis_ld(x, M, lr.SCALE, lr.AMP, l))
    b = lr.bounds(rec)
    for k in ("out3", "grad"):
        assert lr.worst_ratio(got[k], ref[k], b[k] * EPS_LD / lr.EPS) <= 1.0, k


@pytest.mark.parametrize("case", lr.BIG_CASES, ids=lambda c: "n%d_M%d_l%g" % c)
def test_golden_record_is_the_identity_in_long_double(case):
    """The n x n long-double factorisation is the WORSE conditioned statement at these n (cond(Sigma) ~ n amp^2 / sigma^2 against
    cond(A) of a few): its own rounding shows against the M x M identity in long double.  It must stay under a quarter of the
    float64 bound, so that the record can serve as the reference for that bound."""
    n, M, l = case
    (x, y, _, _), ref, rec = lr.marginal_reference(case)
    got = lr.marginal_identity(x, y, M, lr.SCALE, lr.AMP, l, lr.SIGMA, dtype=LD, basis=lr.basis_ld(x, M, lr.SCALE, lr.AMP, l))
    b = lr.bounds(rec)
    for k in ("out3", "grad"):
        r = lr.worst_ratio(got[k], ref[k], b[k])
        print(case, k, r)
        assert r <= 0.25, k


def test_dense_gradient_is_the_central_difference_of_the_dense_value():
    n, M, l = 21, 10, 1.0
    x, y, _, _ = lr.case_inputs(n, M, l)
    ref = lr.marginal_dense(x, y, M, lr.SCALE, lr.AMP, l, lr.SIGMA)
    h = LD(2.0) ** -20   # step error h^2 ~ 1e-12 relative; rounding eps_ld / h ~ 1e-13
    th = [lr.AMP, l, lr.SIGMA]
    for q in range(3):
        vals = []
        for s in (1, -1):
            t = [float(v) for v in th]
            t[q] = float(LD(th[q]) + s * h)
            vals.append(lr.marginal_dense(x, y, M, lr.SCALE, t[0], t[1], t[2])["out3"][0])
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(float(fd - ref["grad"][q])) <= 1e-9 * max(1.0, abs(float(ref["grad"][q]))), (q, fd, ref["grad"][q])


@pytest.mark.parametrize("l,M", lr.CONVERGED)
def test_basis_converges_to_the_squared_exponential_kernel(l, M):
    x = np.linspace(-0.5, 0.5, 41)
    Phi, _ = lr.basis_ld(x, M, lr.SCALE, lr.AMP, l)
    err = float(np.max(np.abs(Phi @ Phi.T - lr.se_kernel_ld(x, lr.AMP, l))))
    bound = lr.truncation_bound(M, lr.SCALE, lr.AMP, l, 0.5) + 64 * EPS_LD * lr.AMP ** 2
    print(l, M, err, bound)
    assert err <= bound


def test_truncation_is_at_rounding_level_where_the_gpu_test_compares_with_the_exact_model():
    for l, M in ((0.3, 40), (1.0, 20)):
        assert lr.truncation_bound(M, lr.SCALE, lr.AMP, l, 0.5) < 1e-13
