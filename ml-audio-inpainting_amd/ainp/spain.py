"""Host side of the sparsity-based row of the reference's model comparison
(models/AudioReg/references/spain: spain_segmentation.m driving aspain.m or
sspain.m with f_update = 'H'), restated without LTFAT: DESIGN §14.

spain_segmentation pads the whole signal to a circular length L, cuts a window
of w samples every a samples and runs SPAIN on every window with missing
samples.  Here every such window, of every gap and signal, is one row of one
ainp_spain launch (csrc/spain.hip, float64) between the gather and the
overlap-add of csrc/janssen_windows.hip, which take this layout as it is.
"""
from __future__ import annotations

import numpy as np

from .janssen import (GAP_MAX, WindowPlan, _cdiv, _normalise, find_gaps, window_pair,
                      window_rescale)

ALGORITHMS = {"aspain": 0, "sspain": 1}      # AINP_SPAIN_A, AINP_SPAIN_S
W_MIN, W_MAX, M_MAX = 8, 4096, 8192          # csrc/spain.hip SP_WMIN, SP_WMAX, SP_MMAX
REDS = (1, 2, 4)


def algorithm_id(algorithm):
    """param.algorithm ("aspain" | "sspain", any case) -> the ABI's id."""
    key = algorithm.lower() if isinstance(algorithm, str) else algorithm
    if key not in ALGORITHMS:
        raise ValueError(f"algorithm must be one of {sorted(ALGORITHMS)}, got {algorithm!r}")
    return ALGORITHMS[key]


def default_maxit(w, red=2, s=1, r=1):
    """ceil(floor(w red / 2 + 1) r / s), clipped to what the loop can use: with
    k >= M/2 + 1 the threshold keeps everything."""
    return min(_cdiv((w * red // 2 + 1) * r, s), w * red // 2 + 1)


def check_window(w, a):
    w, a = int(w), int(a)
    if not (W_MIN <= w <= W_MAX and w & (w - 1) == 0):
        raise ValueError(f"w must be a power of two in [{W_MIN}, {W_MAX}], got w = {w}")
    if a < 1 or w % a:
        raise ValueError(f"the shift a = {a} must divide the window length w = {w}")
    if w // a < 2:
        raise ValueError(f"w / a must be at least 2, got w = {w}, a = {a}")
    return w, a


def check_args(w, red=2, s=1, r=1, epsilon=0.1, maxit=None):
    """The solver's range (ainp_spain's) -> maxit with the default filled in."""
    w, red = int(w), int(red)
    if not (W_MIN <= w <= W_MAX and w & (w - 1) == 0):
        raise ValueError(f"w must be a power of two in [{W_MIN}, {W_MAX}], got w = {w}")
    if red not in REDS or red * w > M_MAX:
        raise ValueError(f"red must be one of {REDS} with red * w <= {M_MAX}, got red = {red}")
    if int(s) < 1 or int(r) < 1:
        raise ValueError("s and r must be at least 1")
    if not float(epsilon) >= 0.0:
        raise ValueError("epsilon must not be negative")
    if maxit is None:
        maxit = default_maxit(w, red, int(s), int(r))
    if not 1 <= int(maxit) <= red * w // 2 + 1:
        raise ValueError(f"maxit must be in [1, red * w / 2 + 1 = {red * w // 2 + 1}]")
    return int(maxit)


def plan_spain_windows(masks, w=4096, a=1024):
    """The batch layout of spain_segmentation.m for a list of boolean observed
    masks: a signal of Ls samples is its own support (origin 0), padded with
    observed zeros to L = ceil(Ls / a) a + (ceil(w / a) - 1) a; window n holds
    the circular indices (n a - floor(w / 2) + i) mod L.  One row per window
    with some, not all, samples missing; a window with all of them missing adds
    zeros and gets none.  Hann windows only.  ValueError for what is not
    covered: w no power of two in [8, 4096], a not dividing w, w / a < 2, a
    window that holds a second gap or two runs, a run of more than 2048."""
    w, a = check_window(w, a)
    gana, gsyn = window_pair("hann", w, a)
    resc = window_rescale(gana, gsyn, a)
    if not (np.all(np.isfinite(gsyn)) and np.all(np.isfinite(resc)) and np.all(resc > 0)):
        raise ValueError(f"w = {w}, a = {a}: the overlap-add weight is not positive everywhere")
    lens = [len(m) for m in masks]
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    sig_off, row_tab, gap_start, gap_len = [], [], [], []
    gap_off, gap_tab, gap_signal, gap_range = [], [], [], []
    pos = np.arange(w)
    for i, obs in enumerate(masks):
        obs = np.asarray(obs, bool)
        Ls, base = len(obs), int(starts[i])
        L = _cdiv(Ls, a) * a + (_cdiv(w, a) - 1) * a
        miss_any = np.zeros(L, bool)
        miss_any[:Ls] = ~obs
        for (g0, g1) in find_gaps(obs):
            if g1 - g0 > GAP_MAX:
                raise ValueError(f"signal {i}: gap [{g0}, {g1}) is longer than {GAP_MAX} samples")
            miss = np.zeros(L, bool)
            miss[g0:g1] = True
            row0 = len(sig_off)
            # the windows that can reach the gap: |n a - c| <= w / 2 for a sample c of it
            n_lo, n_hi = (g0 - w // 2) // a, _cdiv(g1 + w // 2, a)
            for n in sorted({n % (L // a) for n in range(n_lo, n_hi + 1)}):
                idx = (n * a - w // 2 + pos) % L
                m = miss[idx]
                if not m.any():
                    continue
                if np.count_nonzero(miss_any[idx]) != np.count_nonzero(m):
                    raise ValueError(f"signal {i}: a window around the gap [{g0}, {g1}) holds a "
                                     "second gap; one run of missing samples per window only")
                if m.all():
                    continue                      # zeros in the overlap-add
                runs = find_gaps(~m)
                if len(runs) != 1:
                    raise ValueError(f"signal {i}: the gap [{g0}, {g1}) falls into two runs of "
                                     "one window")
                sig_off.append(base)
                row_tab.append((Ls, 0, Ls, L, n, 0))
                gap_start.append(runs[0][0])
                gap_len.append(runs[0][1] - runs[0][0])
            gap_off.append(base + g0)
            gap_tab.append((g1 - g0, g0, L, row0, len(sig_off) - row0, 0))
            gap_signal.append(i)
            gap_range.append((g0, g1))
    i32 = lambda v, cols=None: np.array(v, dtype=np.int32).reshape((-1,) if cols is None
                                                                  else (-1, cols))
    return WindowPlan(("hann",), w, a, int(starts[-1]), gana[None], gsyn[None],
                      np.array(sig_off, dtype=np.int64), i32(row_tab, 6), i32(gap_start),
                      i32(gap_len), np.array(gap_off, dtype=np.int64), i32(gap_tab, 6),
                      i32(gap_signal), i32(gap_range, 2))


def spain_inpaint(signal, mask=None, algorithm="aspain", w=4096, a=1024, wtype="hann", red=2,
                  s=1, r=1, epsilon=0.1, maxit=None, return_history=False, device="cuda"):
    """Fill every gap of `signal` by A-SPAIN or S-SPAIN on the GPU (the
    reference's spain_segmentation.m): windows of w samples every a samples
    over the signal, each with missing samples solved by the ADMM loop with the
    DFT frame of redundancy red, multiplied by the dual window and
    overlap-added.

    Input layouts, mask / NaN conventions and the return layout are
    janssen_inpaint's; only missing samples are written.  algorithm: "aspain"
    or "sspain" (any case).  wtype: "hann" only.  s, r: k starts at s and grows
    by s every r passes; epsilon: the objective that ends a window's loop;
    maxit None: ceil(floor(w red / 2 + 1) r / s).  return_history: also one
    dict per gap (signal, start, end, iters: passes per window with a row,
    objective [n_windows, maxit]: the objective of every pass, NaN after the
    last).
    """
    import torch
    from . import ops
    algorithm_id(algorithm)
    if not (isinstance(wtype, str) and wtype.lower() == "hann"):
        raise ValueError(f"wtype must be 'hann' (the only window SPAIN is set up for), "
                         f"got {wtype!r}")
    w, a = check_window(w, a)
    maxit = check_args(w, red, s, r, epsilon, maxit)
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_spain_windows(masks, w, a)
    info = []
    buf = np.concatenate(sigs) if sigs else np.zeros(0)
    iters = np.zeros(0, np.int32)
    obj = np.zeros((0, maxit)) if return_history else None
    if len(plan):
        dbuf = torch.from_numpy(buf).to(device)
        sol = ops.janssen_windows(dbuf, plan.sig_off, plan.row_tab, plan.gap_start,
                                  plan.gap_len, plan.w, plan.a, plan.gana)
        iters, obj = ops.spain(sol, plan.gap_start, plan.gap_len, algorithm=algorithm, red=red,
                               s=s, r=r, epsilon=epsilon, maxit=maxit,
                               return_history=return_history)
        ops.janssen_ola(sol, None, plan.row_tab, plan.gap_start, plan.gap_len, plan.gap_off,
                        plan.gap_tab, plan.a, plan.gana, plan.gsyn, dbuf)
        buf, iters = dbuf.cpu().numpy(), iters.cpu().numpy()
        obj = obj.cpu().numpy() if obj is not None else None
    for g in range(len(plan.gap_off)):
        h, _, _, row0, nrows, _ = (int(v) for v in plan.gap_tab[g])
        g0, g1 = (int(v) for v in plan.gap_range[g])
        # a sample that only all-missing windows cover stays zero, as the reference gives
        info.append({"signal": int(plan.gap_signal[g]), "start": g0, "end": g1,
                     "iters": [int(v) for v in iters[row0:row0 + nrows]],
                     "objective": obj[row0:row0 + nrows].copy() if obj is not None else None})
    res, at = [], 0
    for sg in sigs:
        res.append(buf[at:at + len(sg)].copy())
        at += len(sg)
    out = res[0] if kind == "single" else res if kind == "list" else np.stack(res)
    return (out, info) if return_history else out
