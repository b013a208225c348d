"""GPU: leading dimensions across the C ABI of the host-buffer entry points, on each path a call can take (one launch through
the pinned, device-mapped buffer / the chain through the staging buffers).

Every case calls the library through gp_amd._lib.load() with raw ctypes arguments (the Python wrappers always pass packed
matrices) twice with the same data: packed (ld = rows), then with every matrix argument at leading dimension rows + 3, the
padding rows of the inputs NaN and the output arrays pre-filled with a sentinel.  The padded results must equal the packed ones
bit for bit -- outputs, gradient and return code -- and every padding row of every output must still hold the sentinel.

The bit-for-bit comparison rests on each packed call repeating itself bit for bit at its shape: every reduction of the
library has a fixed order, and the parent of the commit that added this file was checked to repeat itself on every case below
(no exception was found, so no case falls back to a tolerance).  The cases added since (leave-one-out, the Hessian, the
low-rank model) were checked the same way at the parent of the commit that added them.

A path is forced the way the neighbouring tests do it: a fresh Context with the relevant small_* option at 0 takes the chain,
the default takes one workgroup; the three hard-coded switches (gpmi_exact_gp_f at n <= 256, gpmi_rbf_cov_chol at n <= 64, the
interpolated models at n <= 256 with k <= 8) get one size either side.  Shapes: n = 37, D = 2, m = 5 -- no multiple of 16 or
64, far below any workload size, accepted by every chain."""
import numpy as np
import pytest

from abi_cases import CASES, N, PAD, SENTINEL, ALPHA, JIT, Bufs, _d, _p, contexts, gp_condition, run_case, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_leading_dimensions(contexts, case):
    _, opts, fn = case
    c = contexts(opts)
    packed, ok0 = run_case(c._lib, c._h, fn, 0)
    padded, ok1 = run_case(c._lib, c._h, fn, PAD)
    assert packed["rc"] == 0, c._lib.gpmi_last_error()
    assert ok0 and ok1, "a padding row of an output was written"
    assert packed.keys() == padded.keys()
    for name in packed:
        assert np.all(packed[name] != SENTINEL), name + " was not written"
        assert same_bits(packed[name], padded[name]), name


def test_vjp_gradient_of_nine_keeps_its_own_slot(contexts):
    """gpmi_exact_gp_f_vjp with D = 8 length-scales returns 1 + 8 gradient entries: in the one-launch layout they need a slot
    of nine doubles (a slot of eight let the last one land on F[0, 0]).  F of the one-workgroup call against F of the chain:
    both factor the same matrix backward-stably, so they differ by c cond(K) eps with K = alpha^2 K0 + 1e-6 I, cond(K) <=
    n alpha^2 / 1e-6 < 5e7 at n = 37: 100 cond eps = 1e-6 of max|F| bounds the difference."""
    d8, k = 8, 2
    rng = np.random.default_rng(17)
    X = rng.uniform(-1.0, 1.0, (N, d8)); Z = rng.standard_normal((N, k)); Fb = rng.standard_normal((N, k))
    ell = np.linspace(0.7, 1.4, d8)

    def call(c):
        B = Bufs(0)
        pX, ldx = B.mat(X); pZ, ldz = B.mat(Z); pFb, ldfb = B.mat(Fb)
        F, pF, ldf = B.out(N, k); Zb, pZb, ldzb = B.out(N, k)
        g = np.full(1 + d8, SENTINEL)
        rc = c._lib.gpmi_exact_gp_f_vjp(c._h, pX, N, ldx, d8, _d(ALPHA), B.vec(ell), d8, _d(JIT), pZ, k, ldz, pFb, ldfb, pF, ldf, pZb,
                                        ldzb, _p(g))
        assert rc == 0
        return F, g
    F1, g1 = call(contexts({}))
    F2, g2 = call(contexts({"small_vjp": 0}))
    assert np.max(np.abs(F1 - F2)) <= 1e-6 * np.max(np.abs(F2))
    assert np.all(g1 != SENTINEL) and np.all(g2 != SENTINEL)


def test_pinned_buffer_regrown():
    """A one-launch call that fits the initial 64 KiB pinned buffer, one that makes it grow (gpmi_gp_condition with m = 96:
    m * m doubles exceed 64 KiB, n + m + 1 = 134 rows stay one workgroup), and the first call again, on a path that did not arm
    its completion flag before: the fresh allocation's flag word is whatever the allocator returned."""
    import gp_amd
    c = gp_amd.Context(0)
    try:
        first, _ = run_case(c._lib, c._h, gp_condition(), 0)
        big, _ = run_case(c._lib, c._h, gp_condition(96), 0)
        again, _ = run_case(c._lib, c._h, gp_condition(), 0)
        assert first["rc"] == 0 and big["rc"] == 0 and again["rc"] == 0
        assert np.all(big["Kn"] != SENTINEL) and np.all(big["mn"] != SENTINEL)
        for name in first:
            assert same_bits(first[name], again[name]), name
    finally:
        c.close()
