"""GPU: no result depends on what the context's workspace held before the call.

Every entry point works in buffers its context keeps from call to call (W, the staging buffers, the device scratch, the
packed-factor ring, the finalize sums, the pinned buffer, and the same set in every grid lane), none of which is ever cleared as
a whole: a buffer that is large enough is handed back with a new leading dimension laid over the old contents, and tile loads
over-read rows and columns the call never wrote.  The design rests on one invariant -- whatever is over-read never flows into
a stored result -- and these tests state it directly, with no tolerance: every assertion is bit equality between two runs of the
same code on the same data, or equality of an integer.

 (a), (b), (e)  the five-step protocol: reserve far more workspace than the call needs, run (r0), run again (r0', the control:
                a difference there is non-determinism, not history), gpmi_debug_fill(0xFF) -- every double of the context's
                scratch a NaN --, run (r1), gpmi_debug_fill(0x7F) -- every double 1.38e306: finite, huge, and not absorbed by a
                comparison as a NaN is --, run (r2); r0 == r0' == r1 == r2 in every output and the return code, and
                gpmi_debug_counters() == 0 after every run.  (a): the catalogue of tests/abi_cases.py at n = 37, one workgroup and
                chain; (b): its blocked cases at the smallest ragged orders that leave one panel; (e): three `_dev` forms.
 (c)            the user's own sequence, no hook: a call at n after a larger call with another leading dimension on the same
                context equals the call on a fresh context.
 (d)            recovery: after a factorisation that failed, a batch with one failing lane and a call with a NaN coordinate
                (NaN all over W through the public API alone) the counters are zero and good calls equal a fresh context's.

All contexts are this module's own (one per option set, made on first use), never the session's: no other test's leftovers or
options enter.  No case fell back to a tolerance: every one repeats itself bit for bit."""
import numpy as np
import pytest

import abi_cases as ac
from abi_cases import contexts, run_case, same_bits  # noqa: F401  (contexts: the module's own fixture instance)

pytestmark = pytest.mark.gpu


def _fresh(opts):
    import gp_amd
    c = gp_amd.Context(0)
    for name, value in sorted(opts.items()):
        c.set_option(name, value)
    return c


def _run(c, fn):
    """One call and the counters right after it."""
    res, _ = run_case(c._lib, c._h, fn, 0)
    return res, c.debug_counters()


def _assert_same(label, what, a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert same_bits(a[name], b[name]), "%s: %s of %s differs" % (label, name, what)


def _protocol(label, c, call, reserve):
    """The five steps on context c; call() -> {name: array or int} with "rc"."""
    c.reserve(reserve)

    def run(after):
        res, k = call()
        assert k == 0, "%s: %d non-zero device counters after %s" % (label, k, after)
        return res
    r0 = run("the first run")
    r0b = run("the second run")
    c.debug_fill(0xFF)
    r1 = run("the run after debug_fill(0xFF)")
    c.debug_fill(0x7F)
    r2 = run("the run after debug_fill(0x7F)")
    assert r0["rc"] == 0, (label, r0["rc"], c._lib.gpmi_last_error())
    for name, v in r0.items():
        assert np.all(np.asarray(v) != ac.SENTINEL), "%s: %s was not written" % (label, name)
    _assert_same(label, "the second run (the control: a difference here is non-determinism, not history)", r0, r0b)
    print("%s: control r0 == r0' ok (%d outputs)" % (label, len(r0)))
    _assert_same(label, "the run after debug_fill(0xFF)", r0, r1)
    print("%s: after debug_fill(0xFF) r1 == r0 ok" % label)
    _assert_same(label, "the run after debug_fill(0x7F)", r0, r2)
    print("%s: after debug_fill(0x7F) r2 == r0 ok; counters zero after each of the four runs" % label)


# ---- (a) the catalogue at n = 37 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=[c[0] for c in ac.CASES])
def test_catalogue_is_independent_of_the_fill(contexts, case):
    name, opts, fn = case
    c = contexts(opts)
    _protocol(name, c, lambda: _run(c, fn), 640)


# ---- (b) the blocked factorisation and the chains at the smallest orders that reach them ----------------------------------
@pytest.mark.parametrize("case", ac.BLOCKED_CASES, ids=[c[0] for c in ac.BLOCKED_CASES])
def test_blocked_paths_are_independent_of_the_fill(contexts, case):
    name, opts, fn = case
    c = contexts(opts)
    _protocol(name, c, lambda: _run(c, fn), 1100)


# ---- (c) shrinking after a larger call, no hook ------------------------------------------------------------------------------
ONE, BLOCKED = {}, ac._chain()
SHRINK = [
    # (id, options, the call at n, the larger call before it)
    ("logml-one-37-after-300", ONE, ac.logml_at(37), ac.logml_at(300)),
    ("logml-blocked-300-after-640", BLOCKED, ac.logml_at(300, ac.SYNTH), ac.logml_at(640, ac.SYNTH)),
    ("logml_grad-one-37-after-300", ONE, ac.logml_grad_at(37), ac.logml_grad_at(300)),
    ("logml_grad-blocked-300-after-640", BLOCKED, ac.logml_grad_at(300, ac.SYNTH), ac.logml_grad_at(640, ac.SYNTH)),
    ("gp_condition-one-37-after-300", ONE, ac.gp_condition_series(37, 5), ac.gp_condition_series(300, 259)),
    ("gp_condition-blocked-300-after-640", BLOCKED, ac.gp_condition_series(300, 259), ac.gp_condition_series(640, 300)),
    ("gp_predict_joint-one-37-after-300", ONE, ac.gp_predict_joint(37, 5), ac.gp_predict_joint(300, 259, 3, ac.SYNTH)),
    ("gp_predict_joint-blocked-300-after-640", BLOCKED, ac.gp_predict_joint(300, 259, 3, ac.SYNTH),
     ac.gp_predict_joint(640, 300, 3, ac.SYNTH)),
    ("potrf-one-37-after-300", ONE, ac.potrf(37), ac.potrf(300)),
    ("potrf-blocked-300-after-640", BLOCKED, ac.potrf(300), ac.potrf(640)),
    # a 9-point grid at n = 300 after one at n = 511: one workgroup per point (the default at this size) and the lanes
    ("logml_grid-G9-one-300-after-511", ONE, ac.logml_grid(False, 300, 9, ac.SYNTH, ac.synth_grid_pars),
     ac.logml_grid(False, 511, 9, ac.SYNTH, ac.synth_grid_pars)),
    ("logml_grid-G9-lanes-300-after-511", ac._chain(small_n=0, small_n2=0), ac.logml_grid(False, 300, 9, ac.SYNTH, ac.synth_grid_pars),
     ac.logml_grid(False, 511, 9, ac.SYNTH, ac.synth_grid_pars)),
]


@pytest.mark.parametrize("case", SHRINK, ids=[c[0] for c in SHRINK])
def test_smaller_call_after_a_larger_one_equals_a_fresh_context(case):
    name, opts, fn, larger = case
    first, used = _fresh(opts), _fresh(opts)
    try:
        want, k = _run(first, fn)
        assert want["rc"] == 0 and k == 0, (name, want["rc"], k)
        big, k = _run(used, larger)
        assert big["rc"] == 0 and k == 0, (name, big["rc"], k)
        got, k = _run(used, fn)
        assert k == 0, name
        _assert_same(name, "the call after the larger one", want, got)
        print("%s: equals the fresh context in %d outputs" % (name, len(want)))
    finally:
        first.close(); used.close()


# ---- (d) recovery after failed calls -----------------------------------------------------------------------------------------
def _indefinite(n, pivot):
    A = 2.0 * np.eye(n)
    A[pivot - 1, pivot - 1] = -1.0
    return A


def _bad_batch(n, m):
    """Five draws of the derivative process, the third with sy = 0 and a length-scale of 500: K is numerically singular."""
    def fn(lib, h, B):
        nb = 5
        rng, t, ts, y = ac._series(n, m)
        par = np.array([[0.9 + 0.02 * b, 1.3, 0.1 + 0.01 * b] for b in range(nb)])
        par[2] = (500.0, 1.3, 0.0)
        pY, ldy = B.mat(y[:, None] + 0.01 * np.arange(nb)[None, :])
        pZ, ldz = B.mat(rng.standard_normal((m, nb)))
        dr, pdr, ldd = B.out(m, nb)
        info = np.full(nb, -1, dtype=np.int32)
        rc = lib.gpmi_sample_derivs_batch(h, B.vec(t), n, B.vec(ts), m, pY, ldy, B.vec(par), nb, ac._d(0.0), pZ, ldz, pdr, ldd, None, m,
                                          ac._p(info))
        return {"rc": rc, "draws": dr, "info": info}
    return fn


def _nan_logml(n):
    def fn(lib, h, B):
        _, X, y = ac._synth_data(n)
        X = X.copy(); X[7, 0] = np.nan
        pX, ldx = B.mat(X)
        out = np.full(3, ac.SENTINEL)
        rc = lib.gpmi_logml(h, pX, n, ldx, ac.D, B.vec(y), ac._d(1.0), B.vec(ac.SYNTH.ell), ac.D, ac._d(0.1), ac._d(ac.JIT), ac._p(out))
        return {"rc": rc, "out": out}
    return fn


def _good_calls(n, m):
    src = ac.SYNTH if n > ac.N else ac.UNIFORM
    return [("logml", ac.logml_at(n, src)), ("logml_grad", ac.logml_grad_at(n, src)), ("gp_condition", ac.gp_condition_series(n, m)),
            ("potrf", ac.potrf(n))]


RECOVERY = [
    # (id, options, (order, failing pivot) of the potrf, (n, m) of the batch, the good calls)
    ("blocked", ac._chain(), (300, 129), (301, 200), _good_calls(300, 259)),
    ("one-workgroup", {}, (40, 17), (37, 5), _good_calls(300, 259) + _good_calls(37, 5)),
]


@pytest.mark.parametrize("case", RECOVERY, ids=[c[0] for c in RECOVERY])
def test_good_calls_after_failed_ones_equal_a_fresh_context(case):
    name, opts, (n_bad, pivot), (bn, bm), good = case
    c = _fresh(opts)
    try:
        # every failing call is followed by the counter check BEFORE anything else is launched on this context: a stale
        # counter is what the waiting kernels would poll, and the next launch is not to be the detector
        res, k = _run(c, ac.potrf(n_bad, _indefinite(n_bad, pivot)))
        assert k == 0, "%s: non-zero device counters after the failed potrf" % name
        assert res["rc"] == pivot, (name, res["rc"])
        res, k = _run(c, _bad_batch(bn, bm))
        assert k == 0, "%s: non-zero device counters after the batch with a failing draw" % name
        assert res["rc"] == 0 and res["info"][2] != 0, (name, res["rc"], res["info"])
        batch_info = res["info"].tolist()
        nan_orders = (300,) if opts else (300, 37)
        for n in nan_orders:
            res, k = _run(c, _nan_logml(n))
            assert k == 0, "%s: non-zero device counters after logml with a NaN coordinate at n = %d" % (name, n)
            assert res["rc"] > 0 or np.isnan(res["out"][0]), (name, n, res)
        print("%s: potrf failed at pivot %d, batch info %r, logml with a NaN coordinate at n = %r returned %d; counters zero after each"
              % (name, pivot, batch_info, nan_orders, res["rc"]))
        for i, (what, fn) in enumerate(good):
            f = _fresh(opts)
            try:
                want, kf = _run(f, fn)
            finally:
                f.close()
            got, k = _run(c, fn)
            assert want["rc"] == 0 and kf == 0 and k == 0, (name, what, want["rc"], kf, k)
            _assert_same("%s %s #%d" % (name, what, i), "the call after the failed ones", want, got)
            print("%s: %s #%d equals the fresh context in %d outputs" % (name, what, i, len(want)))
    finally:
        c.close()


# ---- (e) the device-resident forms ---------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch, torch.device("cuda:0")


def _dev(a, dtype=np.float64):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _dev_call(c, enqueue, outs):
    """Sentinel-filled caller tensors, the enqueued call, one synchronisation: ({name: array}, counters)."""
    torch, _ = _torch()
    for name, (t, fill) in outs.items():
        t.copy_(fill) if isinstance(fill, torch.Tensor) else t.fill_(fill)
    torch.cuda.synchronize()
    enqueue()
    c.sync()
    res = {name: t.cpu().numpy() for name, (t, _) in outs.items()}
    res["rc"] = 0 if int(res["info"].ravel()[0]) == 0 else int(res["info"].ravel()[0])
    return res, c.debug_counters()


def _logml_grad_dev(c):
    n = 300
    _, X, y = ac._synth_data(n)
    dX, dy = _dev(X.T), _dev(y)      # column-major: row d of the (D, n) tensor is column d
    outs = {"out": (_dev(np.zeros(3)), ac.SENTINEL), "grad": (_dev(np.zeros(2 + ac.D)), ac.SENTINEL),
            "info": (_dev(np.zeros(1), np.int32), -7)}
    return lambda: _dev_call(c, lambda: c.logml_grad_dev(dX.data_ptr(), n, n, ac.D, dy.data_ptr(), 1.0, ac.SYNTH.ell, 0.1, ac.JIT,
                                                         outs["out"][0].data_ptr(), outs["grad"][0].data_ptr(),
                                                         outs["info"][0].data_ptr()), outs)


def _potrf_dev(c):
    n = 300
    A = _dev(ac._spd(n))             # symmetric: its row-major tensor is the column-major matrix
    outs = {"L": (_dev(np.zeros((n, n))), A), "info": (_dev(np.zeros(1), np.int32), -7)}
    return lambda: _dev_call(c, lambda: c.potrf_dev(outs["L"][0].data_ptr(), n, n, outs["info"][0].data_ptr()), outs)


def _gp_predict_joint_dev(c):
    n, m, nb = 300, 259, 3
    rng, X, y = ac._synth_data(n)
    Xs = rng.uniform(X.min(), X.max(), (m, ac.D)); Z = rng.standard_normal((m, nb))
    dX, dy, dXs, dZ = _dev(X.T), _dev(y), _dev(Xs.T), _dev(Z.T)
    outs = {"mean": (_dev(np.zeros(m)), ac.SENTINEL), "cov": (_dev(np.zeros((m, m))), ac.SENTINEL),
            "draws": (_dev(np.zeros((nb, m))), ac.SENTINEL), "info": (_dev(np.zeros(1), np.int32), -7)}
    return lambda: _dev_call(c, lambda: c.gp_predict_joint_dev(dX.data_ptr(), n, n, ac.D, dy.data_ptr(), 1.0, ac.SYNTH.ell, 0.1, ac.JIT,
                                                               dXs.data_ptr(), m, m, 1e-6, outs["mean"][0].data_ptr(),
                                                               outs["cov"][0].data_ptr(), m, dZ.data_ptr(), nb, m,
                                                               outs["draws"][0].data_ptr(), m, outs["info"][0].data_ptr()), outs)


DEV_FORMS = [("logml_grad_dev-n300", _logml_grad_dev), ("potrf_dev-n300", _potrf_dev),
             ("gp_predict_joint_dev-n300-m259-B3", _gp_predict_joint_dev)]


@pytest.mark.parametrize("case", DEV_FORMS, ids=[c[0] for c in DEV_FORMS])
def test_dev_forms_are_independent_of_the_fill(contexts, case):
    """The caller's buffers are torch tensors, which the fill does not touch: only the context's scratch changes."""
    name, make = case
    c = contexts({})
    _protocol(name, c, make(c), 640)


# ---- the hook itself -----------------------------------------------------------------------------------------------------------
def test_debug_hook_arguments_and_a_fresh_context():
    """byte outside 0..255 is GPMI_EARG; a fresh context (only its fixed buffers allocated, no workspace, no pinned buffer, no
    lanes: every other buffer is skipped) takes the fill, its counters read zero, and its first call is good."""
    import gp_amd
    c = gp_amd.Context(0)
    try:
        assert c._lib.gpmi_debug_fill(c._h, 256) == -1 and c._lib.gpmi_debug_fill(c._h, -1) == -1
        c.debug_fill(0xFF)
        assert c.debug_counters() == 0
        got, k = _run(c, ac.logml)
        assert got["rc"] == 0 and k == 0 and np.all(np.isfinite(got["out"]))
    finally:
        c.close()
