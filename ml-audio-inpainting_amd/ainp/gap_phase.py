"""Gap-constrained Griffin-Lim: blind phase for the frames of a gap.

Given observed audio, a sample mask and target STFT magnitudes, find a phase
for the frames whose window touches a missing sample and new values for the
missing samples only (csrc/gap_phase.hip, include/ainp.h: ainp_gap_phase; the
algorithm is stated there and in DESIGN §16).  Reliable samples and reliable
frames are never touched, nothing is random, the arithmetic is float64.

plan_gap_phase_runs restates csrc/gap_phase_plan.h in Python (the tests hold it
equal to the C query); gap_phase_fill is the entry point the evaluation uses.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _lib

GP_LDS, GP_WORKSPACE = 0, 1    # include/ainp.h AINP_GP_*
WAVES_MAX = 8
LDS_MAX = 160 * 1024
ITER_MAX = 1000

Run = collections.namedtuple("Run", "first_frame n_frames span_start span residency waves")
RunPlan = collections.namedtuple("RunPlan", "waves residency slots span lds_bytes state_bytes")


def _up(n, m):
    return (n + m - 1) // m * m


def check_shape(n_fft, hop, win_length):
    """The shapes csrc/gap_phase_plan.h takes (gp_shape_ok); ValueError otherwise."""
    n_fft, hop, win_length = int(n_fft), int(hop), int(win_length)
    if n_fft < 16 or n_fft > 2048 or n_fft & (n_fft - 1):
        raise ValueError(f"n_fft must be a power of two in [16, 2048], got {n_fft}")
    if win_length < 1 or win_length > n_fft:
        raise ValueError(f"win_length must lie in [1, n_fft], got {win_length}")
    if hop < 1 or hop >= win_length:
        raise ValueError(f"hop_length {hop} >= win_length {win_length} (or < 1): the window "
                         "sum-square over the frames has a zero")


def run_plan(n_fft, hop, n_frames):
    """gp_plan: waves, residency and byte counts of a workgroup whose longest
    run has n_frames frames; None for a run over the cap."""
    R = int(n_frames)
    if R < 1 or (R - 1) * hop + n_fft > LDS_MAX:
        return None
    N = n_fft // 2
    L = (R - 1) * hop + n_fft
    P = _up(N + (N >> 5), 2)
    slots = 64 * max(1, n_fft // 256)

    def fixed(waves):
        return (8 * _up(n_fft // 4 + 1, 2) + 8 * n_fft + 2 * 8 * _up(L, 2) + 8 * _up(R, 2)
                + 8 * 2 * P * waves + _up(L, 16))

    waves = WAVES_MAX
    while fixed(waves) > LDS_MAX:
        if waves == 1:
            return None
        waves >>= 1
    while waves > 1 and waves // 2 >= R:
        waves >>= 1
    state = R * 2 * slots * 16 + R * slots * 8 + _up(R * 4, 16)
    lds = fixed(waves) + state <= LDS_MAX
    return RunPlan(waves, GP_LDS if lds else GP_WORKSPACE, slots, L,
                   fixed(waves) + (state if lds else 0), state)


def unreliable_frames(mask, n_fft, hop, win_length):
    """bool [T]: frame t (center, T = 1 + S // hop) has a missing sample under
    the win_length samples of its window; padding counts as reliable."""
    m = np.asarray(mask).astype(bool).reshape(-1)
    S = m.size
    miss = np.concatenate(([0], np.cumsum(~m)))
    t = np.arange(1 + S // hop, dtype=np.int64)
    a = t * hop + (n_fft - win_length) // 2 - n_fft // 2
    lo, hi = np.clip(a, 0, S), np.clip(a + win_length, 0, S)
    return miss[hi] > miss[lo]


def plan_gap_phase_runs(mask, n_fft, hop, win=None):
    """The runs of consecutive unreliable frames of one signal's mask (1 =
    reliable), ascending, as Run tuples -- what ainp_gap_phase_plan returns."""
    win = n_fft if win is None else win
    check_shape(n_fft, hop, win)
    bad = unreliable_frames(mask, n_fft, hop, win)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], bad.view(np.int8), [0]))))
    runs = []
    for first, end in zip(edges[::2], edges[1::2]):
        p = run_plan(n_fft, hop, end - first)
        if p is None:
            raise ValueError(f"a run of {end - first} unreliable frames is longer than the cap "
                             f"at n_fft={n_fft}, hop={hop}")
        runs.append(Run(int(first), int(end - first), int(first * hop - n_fft // 2), p.span,
                        p.residency, p.waves))
    return runs


def query_runs(mask, n_fft, hop, win=None):
    """The same through the C query (ainp_gap_phase_plan); AinpError for a refusal."""
    import ctypes
    win = n_fft if win is None else win
    m = np.ascontiguousarray(np.asarray(mask).astype(bool).reshape(-1).astype(np.uint8))
    ptr = m.ctypes.data_as(ctypes.c_void_p)
    n = _lib.lib.ainp_gap_phase_plan(ptr, m.size, int(n_fft), int(hop), int(win), None, 0)
    if n < 0:
        _lib.check(int(n), "ainp_gap_phase_plan")
    arr = (_lib.GapPhaseRun * max(1, n))()
    _lib.lib.ainp_gap_phase_plan(ptr, m.size, int(n_fft), int(hop), int(win), arr, n)
    return [Run(r.first_frame, r.n_frames, r.span_start, r.span, r.residency, r.waves)
            for r in arr[:n]]


def gap_phase_fill(audio, mask, mag, n_fft, hop_length, win_length=None, n_iter=64,
                   momentum=0.99, return_resid=False):
    """Fill the missing samples of `audio` so that the STFT of the frames around
    them has the magnitudes `mag`.

    audio [S] or [B, S] float32 / float64 cuda; mask the same shape, nonzero =
    reliable (one mask per row); mag [F, T] or [B, F, T] linear magnitudes,
    F = n_fft/2 + 1, T = 1 + S // hop_length.  The values audio holds on the
    missing samples are the start (NaN: 0), so a Janssen fill can be refined.
    Returns audio's shape and dtype, reliable samples bit-identical, a row
    without gaps unchanged; with return_resid also resid [runs, n_iter]
    float64, the runs in row order.  ValueError for a refused shape (see
    check_shape), a run over the cap, n_iter outside [1, 1000] or momentum
    outside [0, 1]: nothing is launched then."""
    import torch
    from . import ops
    win_length = n_fft if win_length is None else win_length
    check_shape(n_fft, hop_length, win_length)
    if not 1 <= int(n_iter) <= ITER_MAX:
        raise ValueError(f"n_iter must lie in [1, {ITER_MAX}], got {n_iter}")
    if not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"momentum must lie in [0, 1], got {momentum}")
    ops._req(audio, "audio", dtype=None)
    if audio.dtype not in (torch.float32, torch.float64):
        raise TypeError("audio must be float32 or float64")
    if audio.dim() not in (1, 2):
        raise ValueError("audio must be [S] or [B, S]")
    if tuple(mask.shape) != tuple(audio.shape):
        raise ValueError(f"mask is {tuple(mask.shape)}, audio {tuple(audio.shape)}")
    x = audio.reshape(1, -1) if audio.dim() == 1 else audio
    rows, S = x.shape
    F, T = n_fft // 2 + 1, 1 + S // hop_length
    if tuple(mag.shape) != tuple(audio.shape[:-1]) + (F, T):
        raise ValueError(f"mag is {tuple(mag.shape)}, expected "
                         f"{tuple(audio.shape[:-1]) + (F, T)}")
    m8 = (torch.as_tensor(mask).reshape(rows, S) != 0).to(torch.uint8)
    m_host = m8.cpu().numpy()
    run_row, run_first, run_frames = [], [], []
    for r in range(rows):
        for run in plan_gap_phase_runs(m_host[r], n_fft, hop_length, win_length):
            run_row.append(r)
            run_first.append(run.first_frame)
            run_frames.append(run.n_frames)
    out = x.contiguous().clone()
    resid = torch.empty(len(run_row), int(n_iter), device=x.device, dtype=torch.float64)
    if run_row:
        ops.gap_phase(x.contiguous(), m8.to(x.device),
                      mag.reshape(rows, F, T).to(torch.float32).contiguous(), run_row, run_first,
                      run_frames, n_fft, hop_length, win_length, n_iter, momentum, out=out,
                      resid=resid if return_resid else None)
    out = out.reshape(audio.shape)
    return (out, resid) if return_resid else out
