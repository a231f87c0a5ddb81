"""Gap-constrained Griffin-Lim without a GPU: the float64 reference
(tests/gap_phase_ref.py) has the properties DESIGN §16 claims for the
algorithm, the Python plan equals the C query, every refusal is raised before
a launch, and the parity fixtures are well-conditioned -- with their measured
sensitivity E printed (the GPU test's bound is 100 E)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gap_phase_ref as G  # noqa: E402

FIX = [f.name for f in G.FIXTURES]


@pytest.mark.parametrize("name", FIX)
def test_reference_resid_non_increasing_without_momentum(name):
    f = G.BY_NAME[name]
    _, resid = G.gap_phase(f.observed, f.mask, f.mag, f.n_fft, f.hop, f.win, 32, 0.0)
    assert resid.shape == (len(G.runs(f.mask, f.n_fft, f.hop, f.win)), 32)
    for r in resid:
        assert np.all(np.diff(r) <= 1e-12 * r[0]), r


def _as_pairs(runs):
    return [(r.first_frame, r.n_frames) for r in runs]


@pytest.mark.parametrize("name", FIX)
def test_plan_equals_c_query(name):
    from ainp import gap_phase as gp
    f = G.BY_NAME[name]
    py = gp.plan_gap_phase_runs(f.mask, f.n_fft, f.hop, f.win)
    assert py == gp.query_runs(f.mask, f.n_fft, f.hop, f.win)
    assert _as_pairs(py) == G.runs(f.mask, f.n_fft, f.hop, f.win)
    for r in py:
        assert r.span_start == r.first_frame * f.hop - f.n_fft // 2
        assert r.span == (r.n_frames - 1) * f.hop + f.n_fft
    want = {"n2048-h512": gp.GP_WORKSPACE}.get(name, gp.GP_LDS)
    assert all(r.residency == want for r in py)


def test_plan_without_gap_and_all_missing():
    from ainp import gap_phase as gp
    ones = np.ones(1024, bool)
    assert gp.plan_gap_phase_runs(ones, 64, 16, 48) == gp.query_runs(ones, 64, 16, 48) == []
    none = np.zeros(1024, bool)
    py = gp.plan_gap_phase_runs(none, 64, 16, 48)
    assert py == gp.query_runs(none, 64, 16, 48)
    assert _as_pairs(py) == [(0, 65)] == G.runs(none, 64, 16, 48)
    # the same rule through the torch operator over a host mask
    import torch
    from ainp import ops  # noqa: F401
    t = torch.ops.ainp.gap_phase_plan(torch.from_numpy(G.BY_NAME["far-w48"].mask.astype(np.uint8)),
                                      64, 16, 48)
    assert [tuple(r) for r in t.tolist()] == \
        [tuple(r) for r in gp.plan_gap_phase_runs(G.BY_NAME["far-w48"].mask, 64, 16, 48)]


def test_plan_byte_counts():
    """The LDS figures DESIGN §16 quotes are the plan's."""
    from ainp import gap_phase as gp
    from ainp import _lib
    p = gp.run_plan(512, 128, 15)
    assert (p.waves, p.residency, p.lds_bytes, p.state_bytes) == (8, gp.GP_LDS, 155088, 76864)
    p = gp.run_plan(2048, 512, 8)
    assert (p.waves, p.residency, p.lds_bytes, p.state_bytes) == (2, gp.GP_WORKSPACE, 150096,
                                                                  163872)
    assert _lib.lib.ainp_gap_phase_workspace(3, 8, 2048, 512) == 3 * 163872
    assert _lib.lib.ainp_gap_phase_workspace(3, 15, 512, 128) == 0
    for n_fft, hop in ((64, 16), (512, 128), (512, 192), (2048, 512)):
        for R in range(1, 80):
            p = gp.run_plan(n_fft, hop, R)
            assert p is None or p.lds_bytes <= gp.LDS_MAX
    assert gp.run_plan(512, 128, 67) is not None and gp.run_plan(512, 128, 68) is None


REFUSED_SHAPES = [
    (48, 16, 48),      # n_fft not a power of two
    (8, 2, 8),         # below 16
    (4096, 512, 4096),  # above 2048
    (64, 16, 65),      # win_length > n_fft
    (64, 64, 64),      # hop >= win_length: the window sum-square has a zero
    (64, 48, 48),
    (64, 0, 64),
]


@pytest.mark.parametrize("n_fft,hop,win", REFUSED_SHAPES)
def test_refused_shapes(n_fft, hop, win):
    from ainp import _lib
    from ainp import gap_phase as gp
    mask = np.ones(1024, np.uint8)
    mask[100:120] = 0
    with pytest.raises(ValueError):
        gp.plan_gap_phase_runs(mask, n_fft, hop, win)
    ptr = mask.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.ainp_gap_phase_plan(ptr, mask.size, n_fft, hop, win, None, 0) == -1
    assert b"ainp_gap_phase_plan" in _lib.lib.ainp_last_error()
    one = ctypes.c_void_p(16)     # never dereferenced: refused before any launch
    rc = _lib.lib.ainp_gap_phase(one, ctypes.c_void_p(32), 1, 1, 1024, one, one,
                                 1 + 1024 // max(hop, 1), one, one, one, 1, 1, one, n_fft, hop,
                                 win, 8, 0.5, None, None, 0, None)
    assert rc == -1 and b"ainp_gap_phase" in _lib.lib.ainp_last_error()


def test_refused_run_over_the_cap():
    from ainp import _lib
    from ainp import gap_phase as gp
    mask = np.ones(16000, np.uint8)
    mask[1000:1000 + 68 * 128] = 0        # more than 67 frames of n_fft 512, hop 128
    with pytest.raises(ValueError, match="cap"):
        gp.plan_gap_phase_runs(mask, 512, 128, 512)
    ptr = mask.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.ainp_gap_phase_plan(ptr, mask.size, 512, 128, 512, None, 0) == -3
    assert b"cap" in _lib.lib.ainp_last_error()
    one = ctypes.c_void_p(16)
    rc = _lib.lib.ainp_gap_phase(one, ctypes.c_void_p(32), 1, 1, 16000, one, one, 126, one, one,
                                 one, 1, 68, one, 512, 128, 512, 8, 0.5, None, None, 0, None)
    assert rc == -3 and b"cap" in _lib.lib.ainp_last_error()


@pytest.mark.parametrize("n_iter,alpha", [(0, 0.5), (1001, 0.5), (8, -0.01), (8, 1.01),
                                           (8, float("nan"))])
def test_refused_iterations_and_momentum(n_iter, alpha):
    from ainp import _lib
    one = ctypes.c_void_p(16)
    rc = _lib.lib.ainp_gap_phase(one, ctypes.c_void_p(32), 1, 1, 1024, one, one, 65, one, one,
                                 one, 1, 4, one, 64, 16, 48, n_iter, alpha, None, None, 0, None)
    assert rc == -1 and b"n_iter" in _lib.lib.ainp_last_error()


class _NotCuda:
    """Stands in for the audio: gap_phase_fill must refuse before it looks at it."""


@pytest.mark.parametrize("kw", [dict(n_fft=48), dict(win_length=65), dict(hop_length=64),
                                dict(n_iter=0), dict(n_iter=1001), dict(momentum=-0.1),
                                dict(momentum=1.5)])
def test_fill_refuses_before_any_launch(kw):
    from ainp.gap_phase import gap_phase_fill
    args = dict(n_fft=64, hop_length=16, win_length=48, n_iter=8, momentum=0.5)
    args.update(kw)
    with pytest.raises(ValueError):
        gap_phase_fill(_NotCuda(), _NotCuda(), _NotCuda(), **args)


@pytest.mark.parametrize("name", FIX)
def test_fixture_is_well_conditioned(name):
    """At every iteration the parity test compares, each |a| of the reference
    is exactly 0 or at least 1e-8 max|a|; the sensitivity E to a 1e-13
    perturbation of the reliable samples stays below 1e-10 max|x|."""
    f = G.BY_NAME[name]
    for alpha in G.PARITY_ALPHAS:
        cond = []
        G.gap_phase(f.observed, f.mask, f.mag, f.n_fft, f.hop, f.win, max(G.PARITY_ITERS), alpha,
                    cond=cond)
        for lo, hi in cond:
            assert lo >= 1e-8 * hi, (alpha, lo, hi)
    E = G.sensitivity(name)
    print(f"{name}: E = {E:.3e}")
    assert 0 < E <= 1e-10 * np.max(np.abs(f.clean)), E


def test_plan_header_under_asan_ubsan():
    """csrc/gap_phase_plan.h as a stand-alone host program under ASan + UBSan
    (tests/sanitize/gap_phase_plan_check.cpp): the LDS blocks of every plan up
    to the cap are aligned, disjoint and inside 160 KB, and the run finder
    equals the definition taken sample by sample."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "ml-audio-inpainting_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/gap_phase_plan_check"], check=True,
                   capture_output=True)
    r = subprocess.run([os.path.join(csrc, "build", "gap_phase_plan_check")], capture_output=True,
                       text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "gap_phase_plan_check OK" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
