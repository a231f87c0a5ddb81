"""CPU-only checks of the Janssen autoregressive baseline: known answers for
the tests' own reference (tests/janssen_ref.py), gap_sdr, the host-side
segmentation of ainp/janssen.py, and ainp_janssen's argument validation
(before any HIP call, so it runs without a GPU)."""
import ctypes

import numpy as np
import pytest

import janssen_ref as R


# ------------------------------------------------------- the reference itself
@pytest.mark.parametrize("maxit,sdr", [(1, 38.7), (2, 56.8), (10, 56.8)])
def test_reference_known_answers(maxit, sdr):
    """Three sinusoids, 576 samples, gap [256, 320), p = 32: the gap SDR after
    1, 2 and 10 iterations, to 0.2 dB."""
    x = R.sinusoid_mix(576)
    sol, hist, done = R.janssen(x, 256, 64, 32, maxit)
    assert done == maxit and hist.shape == (maxit, 64)
    got = R.gap_sdr(x, sol, 256, 64)
    print(f"maxit {maxit}: gap SDR {got:.3f} dB")
    assert abs(got - sdr) <= 0.2
    obs = np.r_[0:256, 320:576]
    assert np.array_equal(sol[obs], x[obs])


def test_reference_lpc_matches_direct_autocorrelation():
    x = R.sinusoid_mix(300, noise=1e-3, seed=3)
    p = 12
    r = np.array([np.dot(x[:len(x) - k], x[k:]) for k in range(p + 1)])
    a = R.lpc(x, p)
    # the normal equations sum_j a_j r[|i-j|] = 0 for i = 1..p
    T = r[np.abs(np.arange(1, p + 1)[:, None] - np.arange(p + 1)[None, :])]
    assert np.max(np.abs(T @ a)) <= 1e-9 * r[0]


# ------------------------------------------------------------------ gap_sdr
def test_gap_sdr_hand_cases():
    from ainp.janssen import gap_sdr
    clean = np.array([5.0, 3.0, 4.0, 7.0])
    mask = np.array([1, 0, 0, 1])
    # num = 9 + 16 = 25; den = 0.3^2 + 0.4^2 = 0.25 -> 100 -> 20 dB
    assert gap_sdr(clean, np.array([9.0, 3.3, 3.6, -1.0]), mask) == pytest.approx(20.0, abs=1e-9)
    # restored = 0 on the gap -> 0 dB, whatever the observed samples hold
    assert gap_sdr(clean, np.array([5.0, 0.0, 0.0, 7.0]), mask) == pytest.approx(0.0, abs=1e-12)
    # den = 25 / 10 -> 10 dB
    r = clean.copy()
    r[1] += np.sqrt(2.5)
    assert gap_sdr(clean, r, mask.astype(bool)) == pytest.approx(10.0, abs=1e-9)
    assert gap_sdr(clean, clean, mask) == np.inf
    with pytest.raises(ValueError):
        gap_sdr(clean, clean[:3], mask)


# ------------------------------------------------------------- segmentation
def _mask(n, *gaps):
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


def test_find_gaps():
    from ainp.janssen import find_gaps
    assert find_gaps(_mask(10)) == []
    assert find_gaps(_mask(10, (0, 2), (4, 5), (8, 10))) == [(0, 2), (4, 5), (8, 10)]


def test_segments_clip_at_both_ends():
    from ainp.janssen import plan_segments
    seg = plan_segments([_mask(1000, (20, 50)), _mask(1000, (950, 990))], w=100, p=16)
    assert seg.signal.tolist() == [0, 1]
    assert seg.lo.tolist() == [0, 850]
    assert seg.n.tolist() == [150, 150]          # [0, 150) and [850, 1000)
    assert seg.gap_start.tolist() == [20, 100]
    assert seg.gap_len.tolist() == [30, 40]
    assert all(c.dtype == np.int32 for c in (seg.n, seg.gap_start, seg.gap_len))


def test_two_separated_gaps_give_two_segments():
    from ainp.janssen import plan_segments
    seg = plan_segments([_mask(2000, (300, 340), (1500, 1510))], w=200, p=16)
    assert len(seg) == 2
    assert seg.lo.tolist() == [100, 1300] and seg.n.tolist() == [440, 410]
    assert seg.gap_start.tolist() == [200, 200] and seg.gap_len.tolist() == [40, 10]
    # touching but not overlapping: gap 2 starts exactly where segment 1 ends
    seg = plan_segments([_mask(2000, (300, 340), (540, 550))], w=200, p=16)
    assert len(seg) == 2


def test_second_gap_inside_a_segment_is_refused():
    from ainp.janssen import plan_segments
    with pytest.raises(ValueError, match="second gap"):
        plan_segments([_mask(2000, (300, 340), (539, 550))], w=200, p=16)
    with pytest.raises(ValueError, match="second gap"):
        plan_segments([_mask(2000, (300, 340), (350, 360))], w=200, p=16)


def test_unsupported_shapes_are_refused():
    from ainp.janssen import plan_segments
    with pytest.raises(ValueError, match="longer than 2048"):
        plan_segments([_mask(9000, (3000, 5049))], w=100, p=16)
    plan_segments([_mask(9000, (3000, 5048))], w=100, p=16)
    with pytest.raises(ValueError, match="at most 16384"):
        plan_segments([_mask(40000, (20000, 20002))], w=8192, p=16)
    plan_segments([_mask(40000, (20000, 20002))], w=8191, p=16)
    with pytest.raises(ValueError, match="needs p <"):
        plan_segments([_mask(1000, (500, 510))], w=10, p=30)


def test_nan_marks_equal_mask_input():
    from ainp.janssen import _normalise
    x = R.sinusoid_mix(400)
    m = _mask(400, (100, 130), (300, 301))
    xn = x.copy()
    xn[~m] = np.nan
    s1, m1, k1 = _normalise(x, m)
    s2, m2, k2 = _normalise(xn, None)
    assert k1 == k2 == "single"
    assert np.array_equal(s1[0], s2[0]) and np.array_equal(m1[0], m2[0])
    assert np.all(s1[0][~m] == 0) and np.array_equal(s1[0][m], x[m])
    # 0/1 float masks, lists and batches
    s3, m3, k3 = _normalise([x, x[:300]], [m.astype(np.float32), m[:300].astype(int)])
    assert k3 == "list" and np.array_equal(s3[0], s1[0]) and np.array_equal(m3[1], m[:300])
    s4, m4, k4 = _normalise(np.stack([x, x]), np.stack([m, m]))
    assert k4 == "batch" and np.array_equal(s4[1], s1[0])


def test_non_finite_observed_samples_are_refused():
    from ainp.janssen import _normalise
    x = R.sinusoid_mix(100)
    x[7] = np.inf
    with pytest.raises(ValueError, match="finite"):
        _normalise(x, _mask(100, (50, 60)))
    x[7] = np.nan                       # NaN with a mask that calls it observed: a gap
    _, m, _ = _normalise(x, _mask(100, (50, 60)))
    assert not m[0][7]


def test_argument_ranges():
    from ainp.janssen import check_args
    check_args(1, 1)
    check_args(3072, 1000)
    for p, it in ((0, 1), (3073, 1), (16, 0), (16, 1001)):
        with pytest.raises(ValueError):
            check_args(p, it)


# ---------------------------------------------------------------- the C ABI
def test_bad_arguments_fail_without_launching():
    """Every out-of-range argument of ainp_janssen is refused on the host with
    null device pointers standing in -- nothing is dereferenced or launched."""
    from ainp import _lib
    f = _lib.lib.ainp_janssen
    one = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced
    good = dict(sol=one, nseg=1, stride=600, n=one, gs=one, gl=one, p=32, maxit=10, hist=None,
                iters=one, ws=None, wsb=0)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["sol"], a["nseg"], a["stride"], a["n"], a["gs"], a["gl"], a["p"], a["maxit"],
                 a["hist"], a["iters"], a["ws"], a["wsb"], None)

    for kw in (dict(sol=None), dict(n=None), dict(gs=None), dict(gl=None), dict(iters=None),
               dict(nseg=-1), dict(stride=0), dict(p=0), dict(p=-5), dict(maxit=0),
               dict(stride=32), dict(stride=20), dict(ws=None, wsb=64)):
        rc = call(**kw)
        assert rc == -1, kw                                   # AINP_EINVAL
        assert b"ainp_janssen" in _lib.lib.ainp_last_error(), kw
    for kw in (dict(p=3073, stride=4000), dict(maxit=1001), dict(nseg=2 ** 31)):
        rc = call(**kw)
        assert rc == -3, kw                                   # AINP_EUNSUPPORTED
        assert b"ainp_janssen" in _lib.lib.ainp_last_error(), kw
    assert call(nseg=0) == 0             # an empty batch is a no-op, still no launch


def test_workspace_query_is_pure_host():
    from ainp import _lib
    q = _lib.lib.ainp_janssen_workspace
    # every supported shape keeps its vectors in LDS: no global scratch
    for nseg, n_max, p, h in ((1, 576, 32, 64), (256, 9472, 512, 1280), (9, 16384, 3072, 2048)):
        assert q(nseg, n_max, p, h) == 0
