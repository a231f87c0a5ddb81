"""STOI / ESTOI without a GPU: the float64 oracle (tests/stoi_ref.py) has the
properties DESIGN §17 claims for the measure, the band table and the frame
count are the formula's, the Python plan equals the C query, every refusal is
raised before a launch, and the parity fixtures stay clear of the silent-frame
threshold -- with their measured sensitivity printed (the GPU test's bound is
100 times it)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_ref as S  # noqa: E402

FIX = [f.name for f in S.FIXTURES]


def test_band_table_is_the_formula():
    from ainp import stoi as st
    lo, hi = S.band_edges()
    assert lo == S.LO == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert hi == S.HI == S.LO[1:] + [219]
    assert list(st.BAND) == S.LO + [219]
    assert (st.FS, st.NF, st.HOP, st.NFFT, st.J, st.N) == (S.FS, S.NF, S.HOP, S.NFFT, S.J, S.N)
    assert (st.BETA, st.DYN, st.EPS, st.SENTINEL) == (S.BETA, S.DYN, S.EPS, S.SENTINEL)


def test_frame_counts():
    from ainp import stoi as st
    for length, want in S.FRAME_COUNTS.items():
        assert S.frames(length) == st.frames(length) == want, length
    for f in S.FIXTURES:
        if f.length in S.FRAME_COUNTS:
            assert len(S.frame_energies(f.clean)) == S.FRAME_COUNTS[f.length]
            assert S.reference(f.name, False)[1] == S.FRAME_COUNTS[f.length]   # nothing dropped


@pytest.mark.parametrize("extended", [False, True])
def test_identical_signals_score_one(extended):
    for name in ("len3968", "len8000", "silence"):
        x = S.BY_NAME[name].clean
        s, T = S.score(x, x, extended)
        assert T >= S.N and abs(s - 1.0) <= 1e-12, (name, s)


@pytest.mark.parametrize("extended", [False, True])
def test_sentinel_below_thirty_frames(extended):
    for name, T in (("len255", 0), ("len3840", 29)):
        assert S.reference(name, extended) == (1e-5, T)
    assert S.reference("len3968", extended)[1] == 30
    assert S.reference("len3968", extended)[0] != 1e-5


@pytest.mark.parametrize("extended", [False, True])
def test_zeros_score_exactly_zero(extended):
    s, T = S.reference("zeros", extended)
    assert s == 0.0 and not np.isnan(s) and T == S.frames(5000) == 38


def test_silence_drops_some_frames_and_clip_clips():
    f = S.BY_NAME["silence"]
    keep = S.kept_frames(f.clean)
    K = S.frames(f.length)
    assert 0 < len(keep) < K
    assert keep[0] > 0 and keep[-1] < K - 1               # dropped at both ends
    assert np.any(np.diff(keep) > 1)                      # and in the middle
    detail = {}
    S.score(S.BY_NAME["clip"].clean, S.BY_NAME["clip"].restored, False, detail)
    assert detail["clipped"] >= 1


@pytest.mark.parametrize("name", ["len4224", "len8000", "silence", "clip"])
def test_scale_invariance(name):
    f = S.BY_NAME[name]
    bound = 100.0 * S.sensitivity(name)
    for extended in (False, True):
        a, _ = S.reference(name, extended)
        b, _ = S.score(f.clean, 3.0 * f.restored, extended)
        assert abs(a - b) <= bound, (extended, a, b, bound)


@pytest.mark.parametrize("name", FIX)
def test_fixture_is_clear_of_the_threshold(name):
    """The keep decision is a threshold: every frame of every fixture is at
    least 1e-6 dB away from it.  Prints the fixture's sensitivity."""
    f = S.BY_NAME[name]
    e = S.frame_energies(f.clean)
    assert S.threshold_margin(f.clean) >= 1e-6
    E = S.sensitivity(name)
    print(f"{name}: frames {e.size}, kept {S.reference(name, False)[1]}, "
          f"STOI {S.reference(name, False)[0]:.6f}, ESTOI {S.reference(name, True)[0]:.6f}, "
          f"sensitivity {E:.3e}")
    assert 0.0 <= E <= 1e-10


def test_plan_equals_c_query():
    from ainp import _lib
    from ainp import stoi as st
    lengths = sorted({f.length for f in S.FIXTURES} | {0, 256, 50000, st.MAX_LEN})
    for L in lengths:
        for C, R in ((1, 1), (3, 7), (9, 900), (2, 0), (0, 0)):
            py = st.plan(C, R, L)
            assert py == st.query_plan(C, R, L), (C, R, L)
            assert py.frames == S.frames(L) and py.max_len == st.MAX_LEN
            assert _lib.lib.ainp_stoi_workspace(C, R, L) == py.bytes
    assert st.MAX_LEN >= 60 * st.FS
    # the same through the torch operator
    import torch
    from ainp import ops  # noqa: F401
    assert tuple(torch.ops.ainp.stoi_plan(3, 7, 9000)) == tuple(st.plan(3, 7, 9000))
    # the figures DESIGN §17 quotes
    p = st.plan(9, 900, 50000)
    assert (p.frames, p.t_stride, p.chunks, p.bytes) == (389, 390, 6, 42598448)


def test_plan_refusals():
    from ainp import _lib
    from ainp import stoi as st
    for C, R, L in ((-1, 0, 100), (0, -1, 100), (1, 1, -1), (1, 1, st.MAX_LEN + 1)):
        with pytest.raises(ValueError):
            st.plan(C, R, L)
        with pytest.raises(_lib.AinpError, match="ainp_stoi_plan"):
            st.query_plan(C, R, L)
        assert _lib.lib.ainp_stoi_workspace(C, R, L) == 0


def _tables(n, row):
    n = np.asarray(n, np.int32)
    row = np.asarray(row, np.int32)
    return n, row, n.ctypes.data_as(ctypes.c_void_p), row.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("n,row,stride,extended", [
    ([9000, 255, 4096], [2, 0, 3], 9000, 0),            # clean_row past the last clean row
    ([9000, 255, 4096], [2, -1, 0], 9000, 0),           # negative clean_row
    ([9000, 255, 4096], [2, 0, 0], 8999, 0),            # a row longer than the stride
    ([(1 << 20) + 1], [0], 1 << 21, 0),                 # a row over the limit
    ([-5], [0], 9000, 0),
    ([9000], [0], 9000, 2),                             # extended is 0 or 1
    ([9000], [0], -1, 0),
])
def test_bad_arguments_fail_without_a_launch(n, row, stride, extended):
    from ainp import _lib
    n, row, pn, pr = _tables(n, row)
    one = ctypes.c_void_p(16)     # never dereferenced: refused before any HIP call
    rc = _lib.lib.ainp_stoi(one, one, stride, pn, len(n), pr, len(row), one, extended, one, one,
                            one, 1 << 30, None)
    assert rc == -1 and b"ainp_stoi" in _lib.lib.ainp_last_error()


def test_negative_sizes_and_missing_pointers():
    from ainp import _lib
    n, row, pn, pr = _tables([9000], [0])
    one = ctypes.c_void_p(16)
    f = _lib.lib.ainp_stoi
    assert f(one, one, 9000, pn, -1, pr, 1, one, 0, one, one, one, 1 << 30, None) == -1
    assert f(one, one, 9000, pn, 1, pr, -1, one, 0, one, one, one, 1 << 30, None) == -1
    assert f(one, one, 9000, None, 1, pr, 1, one, 0, one, one, one, 1 << 30, None) == -1
    assert f(None, one, 9000, pn, 1, pr, 1, one, 0, one, one, one, 1 << 30, None) == -1
    need = _lib.lib.ainp_stoi_workspace(1, 1, 9000)
    assert f(one, one, 9000, pn, 1, pr, 1, one, 0, one, one, one, need - 1, None) == -1
    assert f(None, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None) == 0   # empty


def test_python_refuses_before_any_launch():
    from ainp import stoi as st
    x = np.zeros(4000)
    with pytest.raises(ValueError, match="restored"):
        st.stoi(x, np.zeros(3999), fs=10000)
    with pytest.raises(ValueError, match="restored"):
        st.stoi([x, x], [x], fs=10000)
    with pytest.raises(ValueError, match="restored"):
        st.stoi(np.zeros((2, 4000)), np.zeros((3, 4000)), fs=10000)
    with pytest.raises(ValueError, match="history_info"):
        st.stoi_curve(x, np.ones(4000, bool), [])
    with pytest.raises(ValueError, match="history"):
        st.stoi_curve(x, np.ones(4000, bool), [{"signal": 0, "start": 5, "end": 9,
                                                "history": None}])
    info = [{"signal": 0, "start": 5, "end": 9, "history": np.zeros((3, 4))}]
    with pytest.raises(ValueError, match="mask"):      # the gap is observed in the mask
        st.stoi_curve(x, np.ones(4000, bool), info)


def test_plan_header_under_asan_ubsan():
    """csrc/stoi_plan.h as a stand-alone host program under ASan + UBSan
    (tests/sanitize/stoi_plan_check.cpp): the band table, the frame count, the
    workspace blocks and the ragged-table check."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "ml-audio-inpainting_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/stoi_plan_check"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(csrc, "build", "stoi_plan_check")], capture_output=True,
                       text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "stoi_plan_check OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
