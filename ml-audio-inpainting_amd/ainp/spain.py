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

from .gaps import (_cdiv, _normalise, check_shift, find_gaps, restack, solve_windows, window_pairs,
                   window_plan, window_rows)
from .janssen import GAP_MAX

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


def _check_w(w):
    if not (W_MIN <= w <= W_MAX and w & (w - 1) == 0):
        raise ValueError(f"w must be a power of two in [{W_MIN}, {W_MAX}], got w = {w}")


def check_window(w, a):
    w, a = int(w), int(a)
    _check_w(w)
    check_shift(w, a)
    return w, a


def check_args(w, red=2, s=1, r=1, epsilon=0.1, maxit=None):
    """The solver's range (ainp_spain's) -> maxit with the default filled in."""
    w, red = int(w), int(red)
    _check_w(w)
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
    pairs = window_pairs(("hann",), w, a, name_shape=False)
    gaps = []
    for i, obs in enumerate(masks):
        obs = np.asarray(obs, bool)
        Ls = len(obs)
        L = _cdiv(Ls, a) * a + (_cdiv(w, a) - 1) * a
        miss_any = np.zeros(L, bool)
        miss_any[:Ls] = ~obs
        for (g0, g1) in find_gaps(obs):
            if g1 - g0 > GAP_MAX:
                raise ValueError(f"signal {i}: gap [{g0}, {g1}) is longer than {GAP_MAX} samples")
            # the windows that can reach the gap: |n a - c| <= w / 2 for a sample c of it
            n_lo, n_hi = (g0 - w // 2) // a, _cdiv(g1 + w // 2, a)
            windows = sorted({n % (L // a) for n in range(n_lo, n_hi + 1)})
            gaps.append((0, i, g0, g1, 0, Ls, L,
                         list(window_rows(miss_any, g0, w, a, windows, i, g0, g1))))
    return window_plan(("hann",), w, a, pairs, masks, gaps)


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
    from . import ops
    algorithm_id(algorithm)
    if not (isinstance(wtype, str) and wtype.lower() == "hann"):
        raise ValueError(f"wtype must be 'hann' (the only window SPAIN is set up for), "
                         f"got {wtype!r}")
    w, a = check_window(w, a)
    maxit = check_args(w, red, s, r, epsilon, maxit)
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_spain_windows(masks, w, a)
    (res,), iters, obj = solve_windows(
        sigs, plan, device, per_gap=False,
        solve=lambda sol: ops.spain(sol, plan.gap_start, plan.gap_len, algorithm=algorithm,
                                    red=red, s=s, r=r, epsilon=epsilon, maxit=maxit,
                                    return_history=return_history))
    if obj is None and return_history:
        obj = np.zeros((0, maxit))           # an empty plan
    info = []
    for g in range(len(plan.gap_off)):
        h, _, _, row0, nrows, _ = (int(v) for v in plan.gap_tab[g])
        g0, g1 = (int(v) for v in plan.gap_range[g])
        # a sample that only all-missing windows cover stays zero, as the reference gives
        info.append({"signal": int(plan.gap_signal[g]), "start": g0, "end": g1,
                     "iters": [int(v) for v in iters[row0:row0 + nrows]],
                     "objective": obj[row0:row0 + nrows].copy() if obj is not None else None})
    out = restack(res, kind)
    return (out, info) if return_history else out
