"""GPU: the pair-row layout of the update tiles (k_gemm_nt<0> / <1>: two adjacent rows per lane, 16-byte fragment reads and
C accesses) at the smallest orders that reach each of its paths -- interior tiles and the whole-k-step form, in-block
products at K = 128 and 256, SYRK diagonal tiles with the fused diagonal block, edge tiles, the augmented row, a last
k-step that is not whole, and C tiles that are not 16-byte aligned.  The one-workgroup partial factorisation is switched
off (small_m = 0) so that the blocked path runs at these orders."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def blocked(ctx):
    ctx.set_option("small_m", 0)
    try:
        yield ctx
    finally:
        ctx.set_option("small_m", 160)
        ctx.set_option("nb_outer", 0)


@functools.lru_cache(maxsize=None)
def _case(n):
    """(X, y, K, numpy's factor, cond(K)) -- computed once per order, never written to."""
    from oracle import oracle as orc
    X, y = orc.synth(n, 3)
    K = orc.cov_exp_quad(X, 1.0, 0.3) + 0.01 * np.eye(n)
    L = np.linalg.cholesky(K)
    for a in (X, y, K, L):
        a.setflags(write=False)
    return X, y, K, L, float(np.linalg.cond(K))


@pytest.mark.parametrize("nb_outer", [128, 256])
@pytest.mark.parametrize("n", [256, 384, 640])
def test_potrf_vs_numpy(blocked, orc, n, nb_outer):
    """gpmi_potrf against numpy.linalg.cholesky, cond(K) * eps relative (forward error bound of a backward-stable
    Cholesky, the bound of test_potrf_vs_the_factor_the_reference_computes), cond(K) computed on the CPU."""
    _, _, K, Lref, cond = _case(n)
    blocked.set_option("nb_outer", nb_outer)
    L = blocked.potrf(K)
    tol = cond * np.finfo(float).eps
    d, dref = np.diag(L), np.diag(Lref)
    e_diag = np.max(np.abs(d - dref) / dref)
    e_low = np.max(np.abs(np.tril(L) - Lref)) / np.max(np.abs(Lref))
    print("potrf n=%d nb_outer=%d cond %.1e: diag rel %.2e, lower triangle rel %.2e (tolerance %.1e)"
          % (n, nb_outer, cond, e_diag, e_low, tol))
    assert e_diag <= tol and e_low <= tol


@pytest.mark.parametrize("n", [257, 300, 511])
def test_logml_vs_lapack(blocked, orc, n):
    """Log marginal likelihood against LAPACK, 1e-10 relative as in test_adaptive_outer_blocks_at_their_thresholds_vs_lapack:
    the augmented row, edge tiles and a last block whose K is not a multiple of 16."""
    import scipy.linalg as sla
    X, y, K, _, _ = _case(n)
    L = sla.cholesky(K, lower=True, check_finite=False)
    z = sla.solve_triangular(L, y, lower=True, check_finite=False)
    want = -0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    got = blocked.logml(X, y, 1.0, [0.3], 0.1)[0]
    print("logml n=%d: rel err vs LAPACK %.2e" % (n, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-10 * abs(want)


@pytest.mark.parametrize("n", [384, 640])
def test_potrf_dev_is_the_same_function_at_every_alignment(blocked, orc, n):
    """The same matrix factored in place three ways -- 16-byte-aligned base with an even leading dimension, the base
    shifted by one double, an odd leading dimension: the three lower triangles are equal bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    _, _, K, _, _ = _case(n)
    info = torch.zeros(1, dtype=torch.int32, device=dev)

    def factor(shift, lda):
        host = np.zeros(shift + lda * n)
        host[shift:].reshape(n, lda)[:, :n] = K  # column j at shift + j lda (K is symmetric)
        buf = torch.from_numpy(host).to(dev)
        assert buf.data_ptr() % 16 == 0
        blocked.potrf_dev(buf.data_ptr() + 8 * shift, n, lda, info.data_ptr())
        blocked.sync()
        assert int(info.item()) == 0
        return np.tril(buf.cpu().numpy()[shift:].reshape(n, lda)[:, :n].T)

    aligned, shifted, odd_ld = factor(0, n), factor(1, n), factor(0, n + 1)
    assert np.array_equal(aligned, shifted) and np.array_equal(aligned, odd_ld)
