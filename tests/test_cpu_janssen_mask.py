"""CPU-only checks of Janssen inpainting for any mask: the tests' own dense
reference (tests/janssen_mask_ref.py), the cluster planner of ainp/janssen.py,
and ainp_janssen_mask's argument validation and workspace query (before any
HIP call, so they run without a GPU)."""
import ctypes

import numpy as np
import pytest

import janssen_mask_ref as R
import janssen_ref


# ------------------------------------------------------- the reference itself
def test_reference_equals_the_single_run_reference():
    """On one run the index-set reference is janssen_ref.janssen, to the bit."""
    x = R.sinusoid_mix(576)
    a, ha, da = R.janssen(x, np.arange(256, 320), 32, 10)
    b, hb, db = janssen_ref.janssen(x, 256, 64, 32, 10)
    d = np.max(np.abs(a - b))
    print(f"index-set reference vs single-run reference: {d}")
    assert d == 0.0 and da == db == 10 and np.array_equal(ha, hb)


@pytest.mark.parametrize("maxit,sdr", [(1, 39.4), (2, 60.9), (10, 60.9)])
def test_reference_known_answer_two_runs(maxit, sdr):
    """Three sinusoids, 576 samples, missing [200, 232) and [250, 282) (18
    samples apart, p = 32: coupled): the SDR over the missing samples after 1,
    2 and 10 iterations, to 0.2 dB."""
    x = R.sinusoid_mix(576)
    miss = R.runs((200, 232), (250, 282))
    sol, hist, done = R.janssen(x, miss, 32, maxit)
    assert done == maxit and hist.shape == (maxit, 64)
    got = R.set_sdr(x, sol, miss)
    print(f"maxit {maxit}: SDR {got:.3f} dB")
    assert abs(got - sdr) <= 0.2
    obs = np.setdiff1d(np.arange(576), miss)
    assert np.array_equal(sol[obs], x[obs])


# ------------------------------------------------------------- the planner
def _mask(n, *gaps):
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


@pytest.mark.parametrize("second", [(539, 550), (350, 360)])
def test_what_plan_segments_refuses_is_one_cluster(second):
    from ainp.janssen import plan_mask_segments, plan_segments
    masks = [_mask(2000, (300, 340), second)]
    with pytest.raises(ValueError, match="second gap"):
        plan_segments(masks, w=200, p=16)
    seg = plan_mask_segments(masks, w=200, p=16)
    assert len(seg) == 1 and seg.signal.tolist() == [0] and seg.runs.tolist() == [2]
    assert seg.lo.tolist() == [100] and seg.n.tolist() == [second[1] + 200 - 100]
    want = np.r_[200:240, second[0] - 100:second[1] - 100]
    assert np.array_equal(seg.missing[0], want) and seg.missing[0].dtype == np.int32
    assert all(c.dtype == np.int32 for c in (seg.signal, seg.lo, seg.n, seg.runs))


def test_runs_w_apart_stay_two_clusters_as_plan_segments_has_them():
    from ainp.janssen import plan_mask_segments, plan_segments
    masks = [_mask(2000, (300, 340), (540, 550)), _mask(1000, (20, 50))]
    seg, old = plan_mask_segments(masks, w=200, p=16), plan_segments(masks, w=200, p=16)
    assert len(seg) == len(old) == 3 and seg.runs.tolist() == [1, 1, 1]
    for name in ("signal", "lo", "n"):
        assert getattr(seg, name).tolist() == getattr(old, name).tolist(), name
    for r in range(3):
        assert seg.missing[r].tolist() == list(range(old.gap_start[r],
                                                     old.gap_start[r] + old.gap_len[r]))


def test_clusters_clip_at_both_ends():
    from ainp.janssen import plan_mask_segments
    seg = plan_mask_segments([_mask(1000, (20, 50), (70, 75)), _mask(1000, (930, 950), (985, 1000))],
                             w=100, p=16)
    assert seg.signal.tolist() == [0, 1] and seg.runs.tolist() == [2, 2]
    assert seg.lo.tolist() == [0, 830] and seg.n.tolist() == [175, 170]
    assert seg.missing[0].tolist() == list(range(20, 50)) + list(range(70, 75))
    assert seg.missing[1].tolist() == list(range(100, 120)) + list(range(155, 170))


def test_a_chain_of_runs_is_one_cluster():
    """Each run within w of the next, the first and the last farther than w apart."""
    from ainp.janssen import plan_mask_segments
    seg = plan_mask_segments([_mask(3000, (500, 520), (700, 710), (900, 930), (1400, 1410))],
                             w=200, p=16)
    assert seg.runs.tolist() == [3, 1]
    assert seg.lo.tolist() == [300, 1200] and seg.n.tolist() == [830, 410]
    assert len(seg.missing[0]) == 60 and seg.missing[0][[0, -1]].tolist() == [200, 629]
    assert plan_mask_segments([np.ones(50, bool)], w=10, p=4).missing == []


def test_limits_sit_exactly_at_their_values():
    from ainp.janssen import plan_mask_segments
    # 2048 / 2049 missing samples in a cluster of two runs
    plan_mask_segments([_mask(9000, (3000, 4024), (4030, 5054))], w=100, p=16)
    with pytest.raises(ValueError, match=r"signal 0: .*\[3000, 5055\).*2049 missing.*2048"):
        plan_mask_segments([_mask(9000, (3000, 4024), (4030, 5055))], w=100, p=16)
    # 16384 / 16385 samples: two runs whose hull is 2 / 3 samples, w either side
    seg = plan_mask_segments([_mask(40000, (20000, 20001), (20002, 20003))], w=8190, p=16)
    assert seg.n.tolist() == [16383]
    seg = plan_mask_segments([_mask(40000, (20000, 20001), (20003, 20004))], w=8190, p=16)
    assert seg.n.tolist() == [16384]
    with pytest.raises(ValueError, match=r"signal 0: .*\[11810, 28195\).*16385.*16384"):
        plan_mask_segments([_mask(40000, (20000, 20001), (20004, 20005))], w=8190, p=16)
    # n = p + 1 / n = p
    seg = plan_mask_segments([_mask(1000, (500, 502), (505, 511))], w=10, p=30)
    assert seg.n.tolist() == [31]
    with pytest.raises(ValueError, match=r"signal 0: .*\[490, 521\).*needs p < 31"):
        plan_mask_segments([_mask(1000, (500, 502), (505, 511))], w=10, p=31)
    with pytest.raises(ValueError):
        plan_mask_segments([_mask(100, (5, 6))], w=0, p=4)


def test_re_exports():
    import models.AudioReg as A
    from ainp import janssen
    assert A.janssen_inpaint_mask is janssen.janssen_inpaint_mask
    assert A.plan_mask_segments is janssen.plan_mask_segments
    assert {"janssen_inpaint_mask", "plan_mask_segments"} <= set(A.__all__)


# ---------------------------------------------------------------- the C ABI
def test_bad_arguments_fail_without_launching():
    """Every out-of-range argument of ainp_janssen_mask is refused on the host
    with null device pointers standing in -- nothing is dereferenced or
    launched, so this runs with no GPU present."""
    from ainp import _lib
    f = _lib.lib.ainp_janssen_mask
    q = _lib.lib.ainp_janssen_mask_workspace
    one = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced
    need = q(1, 600, 32, 64, 0)
    good = dict(sol=one, nseg=1, stride=600, n=one, off=one, idx=one, h_max=64, p=32, maxit=10,
                method=0, hist=None, hist_row=0, iters=one, ws=one, wsb=need)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["sol"], a["nseg"], a["stride"], a["n"], a["off"], a["idx"], a["h_max"], a["p"],
                 a["maxit"], a["method"], a["hist"], a["hist_row"], a["iters"], a["ws"], a["wsb"],
                 None)

    for kw in (dict(sol=None), dict(n=None), dict(off=None), dict(idx=None), dict(iters=None),
               dict(nseg=-1), dict(stride=0), dict(p=0), dict(p=-5), dict(maxit=0), dict(h_max=0),
               dict(stride=32), dict(method=2), dict(method=-1),
               dict(hist=one, hist_row=63), dict(wsb=need - 1), dict(ws=None), dict(wsb=0)):
        rc = call(**kw)
        assert rc == -1, kw                                   # AINP_EINVAL
        assert b"ainp_janssen_mask" in _lib.lib.ainp_last_error(), kw
    for kw in (dict(p=3073, stride=4000), dict(maxit=1001), dict(h_max=2049),
               dict(nseg=2 ** 31)):
        rc = call(**kw)
        assert rc == -3, kw                                   # AINP_EUNSUPPORTED
        assert b"ainp_janssen_mask" in _lib.lib.ainp_last_error(), kw
    assert call(nseg=0) == 0             # an empty batch is a no-op, still no launch


def test_workspace_query_is_pure_host_and_monotone():
    from ainp import _lib
    q = _lib.lib.ainp_janssen_mask_workspace
    # per segment: the row (n_max rounded up to even) and h_max (rounded up to
    # even) columns of min(h_max - 1, p) + 1 entries, in doubles
    assert q(1, 600, 32, 64, 0) == 8 * (600 + 64 * 33)
    assert q(3, 601, 32, 5, 1) == 3 * 8 * (602 + 6 * 5)
    assert q(1, 9952, 512, 1280, 0) == 8 * (9952 + 1280 * 513)
    assert q(1, 16384, 3072, 2048, 0) == 8 * (16384 + 2048 * 2048)
    for n_max, p in ((600, 32), (16384, 3072)):
        sizes = [q(2, n_max, p, h, 0) for h in range(1, 2049)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        assert [q(2, n_max, p, h, 1) for h in (1, 100, 2048)] == [sizes[0], sizes[99], sizes[2047]]
