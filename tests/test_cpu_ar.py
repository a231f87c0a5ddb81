"""CPU-only checks of the Burg estimator and the forward/backward
extrapolation: the tests' own reference (tests/ar_ref.py) against a second
formulation and known answers, the host wrappers' ValueErrors, and the argument
validation of the three launching entry points (before any HIP call, so it runs
without a GPU)."""
import ctypes
import inspect

import numpy as np
import pytest

import ar_ref as A
import janssen_ref as R


# ------------------------------------------------------- the reference itself
def test_burg_reference_against_long_double():
    """Plain float64 against np.longdouble accumulation, on the GPU tests' signal."""
    x = R.sinusoid_mix(576, noise=1e-3, seed=10)
    for p in (1, 16, 33):
        a, b = A.arburg(x, p), A.arburg(x, p, np.longdouble)
        d = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f"arburg p={p}: float64 against long double {d:.3e}")
        assert a.shape == (p + 1,) and a[0] == 1.0
        assert d <= 1e-10


def test_burg_first_reflection_is_the_forward_backward_least_squares_fit():
    """Order 1: k minimises sum (x[n] + k x[n-1])^2 + (x[n-1] + k x[n])^2."""
    x = R.sinusoid_mix(300, noise=1e-3, seed=3)
    k = A.arburg(x, 1)[1]
    M = np.concatenate((x[:-1], x[1:]))[:, None]        # regressors of both errors
    y = np.concatenate((x[1:], x[:-1]))
    k_ls = np.linalg.lstsq(M, -y, rcond=None)[0][0]
    assert abs(k - k_ls) <= 1e-12


def test_burg_recovers_a_noiseless_ar2_process():
    """x[n] = 2 cos(th) x[n-1] - x[n-2], the undamped AR(2) process, which both
    prediction directions share.  Burg fixes k1 before it sees order 2, so the
    answer [1, -2 cos(th), 1] is exact only where the order-1 sums are: over a
    whole number of periods of 2 th, (n - 1) 2 th = 2 pi m.  Then k1 = -cos(th)
    and the order-1 errors are ef = -eb, so k2 = 1."""
    n, m = 401, 37
    th = np.pi * m / (n - 1)
    a1, a2 = -2 * np.cos(th), 1.0
    x = np.zeros(n)
    x[0], x[1] = np.cos(0.4), np.cos(th + 0.4)
    for i in range(2, n):
        x[i] = -a1 * x[i - 1] - a2 * x[i - 2]
    a = A.arburg(x, 2)
    print("arburg AR(2):", a, "want", [1.0, a1, a2])
    assert np.max(np.abs(a - [1.0, a1, a2])) <= 1e-8


def test_crossfade_weight_for_a_single_sample_is_matlabs():
    """MATLAB's linspace(0, pi/2, 1) is pi/2: weight cos^2(pi/2), so the sample
    is the postdiction."""
    w1 = A.crossfade_weights(1)
    assert w1.shape == (1,) and w1[0] == np.cos(np.pi / 2) ** 2 and w1[0] < 1e-30
    w = A.crossfade_weights(5)
    assert w[0] == 1.0 and w[-1] < 1e-30 and np.all(np.diff(w) < 0)
    x = R.sinusoid_mix(257, noise=1e-3, seed=5)
    sol, status = A.extrapolate(x, 128, 1, 24, 4096, "lpc")
    bwd, _ = A.predict(x[129:][::-1], 1, 24, "lpc")
    assert status == 1 and sol[128] == pytest.approx(bwd[0], rel=0, abs=1e-30)


def test_extrapolation_reference_continues_a_sinusoid():
    x = R.sinusoid_mix(600)
    for method in ("lpc", "arburg"):
        sol, status = A.extrapolate(x, 280, 40, 32, 4096, method)
        sdr = R.gap_sdr(x, sol, 280, 40)
        print(f"extrapolation reference, {method}: gap SDR {sdr:.1f} dB")
        assert status == 1 and sdr > 20.0
        obs = np.r_[0:280, 320:600]
        assert np.array_equal(sol[obs], x[obs])


def test_constant_context_predicts_its_mean():
    x = R.sinusoid_mix(300, noise=1e-3, seed=2)
    x[:100] = 0.25
    sol, status = A.extrapolate(x, 100, 10, 16, 4096, "arburg")
    fwd, const = A.predict(x[:100], 10, 16, "arburg")
    assert status == 0 and const and np.all(fwd == 0.25)


# ------------------------------------------------------------ host wrappers
def _mask(n, *gaps):
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


def test_method_names():
    from ainp.janssen import method_id
    assert method_id("lpc") == 0 and method_id("LPC") == 0
    assert method_id("arburg") == 1 and method_id("ArBurg") == 1
    for bad in ("burg", "", None, 2):
        with pytest.raises(ValueError, match="method"):
            method_id(bad)


def test_janssen_inpaint_defaults_to_lpc():
    from ainp.janssen import ar_extrapolate, janssen_inpaint
    from ainp import ops
    assert inspect.signature(janssen_inpaint).parameters["method"].default == "lpc"
    assert inspect.signature(ar_extrapolate).parameters["method"].default == "lpc"
    assert inspect.signature(ops.janssen).parameters["method"].default == "lpc"
    # the parameters that were there keep their positions
    assert list(inspect.signature(janssen_inpaint).parameters)[:7] == [
        "signal", "mask", "p", "w", "maxit", "return_history", "device"]


def test_wrappers_refuse_before_touching_the_gpu():
    """Unknown method, a context not longer than p, a second gap in a context:
    ValueError from the host checks, no device needed."""
    from ainp.janssen import ar_extrapolate, janssen_inpaint
    x = R.sinusoid_mix(2000)
    with pytest.raises(ValueError, match="method"):
        janssen_inpaint(x, _mask(2000, (900, 940)), p=16, w=200, method="yule")
    with pytest.raises(ValueError, match="method"):
        ar_extrapolate(x, _mask(2000, (900, 940)), p=16, w=200, method="yule")
    # contexts of 16 (clipped by the signal) and of 30 (clipped by w) samples, p = 16 / 30
    with pytest.raises(ValueError, match="contexts"):
        ar_extrapolate(x, _mask(2000, (16, 50)), p=16, w=200)
    with pytest.raises(ValueError, match="contexts"):
        ar_extrapolate(x, _mask(2000, (900, 940)), p=30, w=30)
    with pytest.raises(ValueError, match="contexts"):
        ar_extrapolate(x, _mask(2000, (1950, 1990)), p=16, w=200)
    with pytest.raises(ValueError, match="second gap"):
        ar_extrapolate(x, _mask(2000, (300, 340), (539, 550)), p=16, w=200)
    with pytest.raises(ValueError):
        ar_extrapolate(x, _mask(2000, (900, 940)), p=0, w=200)
    with pytest.raises(ValueError):
        ar_extrapolate(x, _mask(2000, (900, 940)), p=16, w=0)


def test_model_eval_refuses_unknown_cells(tmp_path):
    from models import model_eval
    with pytest.raises(ValueError, match="algorithm"):
        model_eval.run_ar_evaluation(str(tmp_path), str(tmp_path / "o"), algorithm="spain")
    with pytest.raises(ValueError, match="method"):
        model_eval.run_ar_evaluation(str(tmp_path), str(tmp_path / "o"), method="yule")
    from models.AudioReg import ar_extrapolate, gap_sdr, janssen_inpaint  # noqa: F401


# ---------------------------------------------------------------- the C ABI
ONE = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced


def _check(f, name, order, good, einval, eunsupported):
    from ainp import _lib

    def call(**kw):
        a = dict(good, **kw)
        return f(*(a[k] for k in order))

    for kw in einval:
        assert call(**kw) == -1, kw                               # AINP_EINVAL
        assert name in _lib.lib.ainp_last_error(), kw
    for kw in eunsupported:
        assert call(**kw) == -3, kw                               # AINP_EUNSUPPORTED
        assert name in _lib.lib.ainp_last_error(), kw
    assert call(nseg=0) == 0             # an empty batch is a no-op, still no launch


def test_janssen_ex_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ("sol", "nseg", "stride", "n", "gs", "gl", "p", "maxit", "hist", "iters", "ws", "wsb",
             "method", "stream")
    for method in (0, 1):
        good = dict(sol=ONE, nseg=1, stride=600, n=ONE, gs=ONE, gl=ONE, p=32, maxit=10, hist=None,
                    iters=ONE, ws=None, wsb=0, method=method, stream=None)
        _check(_lib.lib.ainp_janssen_ex, b"ainp_janssen_ex", order, good,
               (dict(sol=None), dict(n=None), dict(gs=None), dict(gl=None), dict(iters=None),
                dict(nseg=-1), dict(stride=0), dict(p=0), dict(p=-5), dict(maxit=0),
                dict(stride=32), dict(stride=20), dict(ws=None, wsb=64), dict(method=2),
                dict(method=-1)),
               (dict(p=3073, stride=4000), dict(maxit=1001), dict(nseg=2 ** 31)))


def test_janssen_forwards_with_lpc():
    """ainp_janssen keeps its thirteen arguments and its validation."""
    from ainp import _lib
    order = ("sol", "nseg", "stride", "n", "gs", "gl", "p", "maxit", "hist", "iters", "ws", "wsb",
             "stream")
    good = dict(sol=ONE, nseg=1, stride=600, n=ONE, gs=ONE, gl=ONE, p=32, maxit=10, hist=None,
                iters=ONE, ws=None, wsb=0, stream=None)
    _check(_lib.lib.ainp_janssen, b"ainp_janssen", order, good,
           (dict(sol=None), dict(p=0), dict(stride=32)), (dict(p=3073, stride=4000),))


def test_ar_extrapolate_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ("sol", "nseg", "stride", "n", "gs", "gl", "p", "w", "method", "status", "ws", "wsb",
             "stream")
    q = _lib.lib.ainp_ar_extrapolate_workspace
    for method in (0, 1):
        need = q(1, 600, 32, 2048, method)
        good = dict(sol=ONE, nseg=1, stride=600, n=ONE, gs=ONE, gl=ONE, p=32, w=4096,
                    method=method, status=ONE, ws=ONE, wsb=need, stream=None)
        _check(_lib.lib.ainp_ar_extrapolate, b"ainp_ar_extrapolate", order, good,
               (dict(sol=None), dict(n=None), dict(gs=None), dict(gl=None), dict(status=None),
                dict(nseg=-1), dict(stride=0), dict(p=0), dict(p=-5), dict(w=0), dict(w=-3),
                dict(stride=32), dict(stride=20), dict(ws=None), dict(wsb=need - 1),
                dict(ws=None, wsb=0), dict(method=2), dict(method=-1)),
               (dict(p=3073, stride=4000, wsb=1 << 20), dict(nseg=2 ** 31)))


def test_workspace_queries_are_pure_host():
    from ainp import _lib
    qj = _lib.lib.ainp_janssen_ex_workspace
    qx = _lib.lib.ainp_ar_extrapolate_workspace
    for nseg, n_max, p, h in ((1, 576, 32, 64), (256, 9472, 512, 1280), (9, 16384, 3072, 2048)):
        for method in (0, 1):
            # Burg's error vectors stay in registers: Janssen needs no global scratch
            assert qj(nseg, n_max, p, h, method) == 0
            assert _lib.lib.ainp_janssen_workspace(nseg, n_max, p, h) == 0
            # the two sides of a segment meet in global memory: 2 x h doubles + 2 flags
            assert qx(nseg, n_max, p, h, method) == nseg * 2 * (min(h, n_max, 2048) * 8 + 4)
    assert qx(0, 600, 32, 64, 0) == 0
    assert qx(3, 100, 32, 2048, 1) == 3 * 2 * (100 * 8 + 4)      # a gap is inside its segment
