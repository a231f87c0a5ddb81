"""Host side of the autoregressive baselines (models/AudioReg of the
reference: utils/janssen_inp.m and utils/arinpaint.m driven by train.m, with
method "lpc" or "arburg").

train.m cuts one segment of w samples either side of every gap and hands each
to janssen_inp; here every gap of every signal becomes one row of a batch and
the whole batch is one launch of ainp_janssen_ex (csrc/janssen.hip, float64)
or of ainp_ar_extrapolate (csrc/ar_extrapolate.hip).  janssen_inpaint_mask lifts
the one-gap-per-segment limit: gaps closer than w share a segment, solved by
ainp_janssen_mask (csrc/janssen_mask.hip), as janssen_inp.m takes any mask.
Segments are clipped to the signal (train.m:134-135 indexes past the ends for
a gap within w of them).  gap_sdr is train.m:196 / model_eval.m:60.

The window-wise rows (utils/segmentation_inp.m on the support train.m:146-172
cuts with offset.m and min_sig_supp_2.m; Hann, rectangular and Tukey windows)
are plan_windows / janssen_windowed at the end of the file: every window with
missing samples, of every gap, signal and window shape, is one row of the same
ainp_janssen_ex launch, between the gather and the overlap-add of
csrc/janssen_windows.hip.  plan_windows_mask / janssen_windowed_mask after them
are segmentation_inp.m on a whole signal with any mask: one window grid per
signal, windows with one run of missing samples to ainp_janssen_ex, the others
to ainp_janssen_mask, between the same gather and overlap-add.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .gaps import (WTYPES, MaskWindowPlan, WindowPlan, _cdiv, _normalise,  # noqa: F401
                   _to_numpy, check_shift, find_gaps, gap_sdr, mask_window_plan, restack,
                   solve_windows, window_pair, window_pairs, window_plan, window_rescale,
                   window_rows, wtype_key)

P_MAX = 3072          # csrc/ar_limits.h JN_PMAX
N_MAX = 16384         # JN_NMAX
GAP_MAX = 2048        # JN_HMAX
MAXIT_MAX = 1000      # JN_ITMAX
METHODS = {"lpc": 0, "arburg": 1}     # AINP_AR_LPC, AINP_AR_BURG


def method_id(method):
    """train.m's `method` ("lpc" | "arburg", any case as strcmpi) -> the ABI's id."""
    key = method.lower() if isinstance(method, str) else method
    if key not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
    return METHODS[key]


@dataclass
class Segments:
    """One row per gap: signal index, segment [lo, lo + n) within it, and the
    gap [gap_start, gap_start + gap_len) relative to lo."""
    signal: np.ndarray
    lo: np.ndarray
    n: np.ndarray
    gap_start: np.ndarray
    gap_len: np.ndarray

    def __len__(self):
        return len(self.signal)


def plan_segments(masks, w=4096, p=512):
    """The batch layout for a list of boolean observed masks: every gap gets
    [start - w, end + w) clipped to its signal.  ValueError for what the kernel
    does not cover: a second gap inside a segment, a gap longer than 2048, a
    segment longer than 16384 or not longer than p."""
    if w < 1:
        raise ValueError("w must be positive")
    rows = []
    for i, obs in enumerate(masks):
        gaps = find_gaps(obs)
        for g, (a, b) in enumerate(gaps):
            if b - a > GAP_MAX:
                raise ValueError(f"signal {i}: gap [{a}, {b}) is longer than {GAP_MAX} samples")
            lo, hi = max(0, a - w), min(len(obs), b + w)
            if (g > 0 and gaps[g - 1][1] > lo) or (g + 1 < len(gaps) and gaps[g + 1][0] < hi):
                raise ValueError(f"signal {i}: the segment [{lo}, {hi}) around the gap [{a}, {b}) "
                                 "contains a second gap; one gap per segment only")
            if hi - lo > N_MAX:
                raise ValueError(f"signal {i}: segment of {hi - lo} samples, at most {N_MAX}")
            if hi - lo <= p:
                raise ValueError(f"signal {i}: segment of {hi - lo} samples needs p < {hi - lo}")
            rows.append((i, lo, hi - lo, a - lo, b - a))
    cols = np.array(rows, dtype=np.int64).reshape(-1, 5).T
    return Segments(*(c.astype(np.int32) for c in cols))


@dataclass
class MaskSegments:
    """One row per cluster of runs: signal index, segment [lo, lo + n) within
    it, the missing samples relative to lo (ascending), and how many runs they
    form."""
    signal: np.ndarray
    lo: np.ndarray
    n: np.ndarray
    missing: list
    runs: np.ndarray

    def __len__(self):
        return len(self.signal)


def plan_mask_segments(masks, w=4096, p=512):
    """The batch layout for any mask: consecutive runs of missing samples
    [a_k, b_k), [a_k+1, b_k+1) share a cluster exactly when a_k+1 - b_k < w (where
    plan_segments refuses), and a cluster's segment is [a_first - w, b_last + w)
    clipped to its signal.  Where nothing merges the rows are plan_segments'.
    ValueError for what the kernel does not cover: more than 2048 missing
    samples in a cluster, a segment longer than 16384 or not longer than p."""
    if w < 1:
        raise ValueError("w must be positive")
    sig, los, ns, miss, runs = [], [], [], [], []
    for i, obs in enumerate(masks):
        clusters = []
        for a, b in find_gaps(obs):
            if clusters and a - clusters[-1][-1][1] < w:
                clusters[-1].append((a, b))
            else:
                clusters.append([(a, b)])
        for cl in clusters:
            a, b = cl[0][0], cl[-1][1]
            count = sum(e - s for s, e in cl)
            if count > GAP_MAX:
                raise ValueError(f"signal {i}: the gaps in [{a}, {b}) hold {count} missing "
                                 f"samples, at most {GAP_MAX} per segment")
            lo, hi = max(0, a - w), min(len(obs), b + w)
            if hi - lo > N_MAX:
                raise ValueError(f"signal {i}: segment [{lo}, {hi}) of {hi - lo} samples, at "
                                 f"most {N_MAX}")
            if hi - lo <= p:
                raise ValueError(f"signal {i}: segment [{lo}, {hi}) of {hi - lo} samples needs "
                                 f"p < {hi - lo}")
            sig.append(i)
            los.append(lo)
            ns.append(hi - lo)
            miss.append(np.concatenate([np.arange(s - lo, e - lo, dtype=np.int32)
                                        for s, e in cl]))
            runs.append(len(cl))
    return MaskSegments(np.array(sig, np.int32), np.array(los, np.int32), np.array(ns, np.int32),
                        miss, np.array(runs, np.int32))


def check_args(p, maxit):
    if not 1 <= int(p) <= P_MAX:
        raise ValueError(f"p must be in [1, {P_MAX}]")
    if not 1 <= int(maxit) <= MAXIT_MAX:
        raise ValueError(f"maxit must be in [1, {MAXIT_MAX}]")


def _solve_segments(sigs, seg, device, key, launch):
    """The gap-wise batch: one zero-padded float64 row per segment goes to the
    device, launch(sol) -> (int32 per row, history or None) solves the rows in
    place, and every row's gap is written into its signal.  -> (one dict per gap:
    signal, start, end, `key`: the row's integer; the history as numpy)."""
    import torch
    if not len(seg):
        return [], None
    batch = np.zeros((len(seg), int(seg.n.max())), np.float64)
    for r in range(len(seg)):
        s = sigs[seg.signal[r]]
        batch[r, :seg.n[r]] = s[seg.lo[r]:seg.lo[r] + seg.n[r]]
    sol = torch.from_numpy(batch).to(device)
    count, hist = launch(sol)
    sol, count = sol.cpu().numpy(), count.cpu().numpy()
    hist = hist.cpu().numpy() if hist is not None else None
    info = []
    for r in range(len(seg)):
        a, h = int(seg.gap_start[r]), int(seg.gap_len[r])
        lo = int(seg.lo[r])
        sigs[seg.signal[r]][lo + a:lo + a + h] = sol[r, a:a + h]
        info.append({"signal": int(seg.signal[r]), "start": lo + a, "end": lo + a + h,
                     key: int(count[r])})
    return info, hist


def janssen_inpaint(signal, mask=None, p=512, w=4096, maxit=20, return_history=False,
                    device="cuda", method="lpc"):
    """Fill every gap of `signal` by the gap-wise Janssen algorithm on the GPU.

    signal: 1-D, a list of 1-D signals, or a 2-D batch (numpy or torch).  mask:
    True / 1 where observed (same layout), or None with NaN marking the missing
    samples as in the reference.  Returns float64 numpy in the layout of the
    input; observed samples come back unchanged.  return_history: also a list
    with one dict per gap (signal, start, end, iters, history [maxit, gap_len]:
    the gap after every iteration, NaN for iterations not completed).
    method: the AR estimator, "lpc" or "arburg" (train.m's `method`).
    """
    from . import ops
    check_args(p, maxit)
    method_id(method)
    sigs, masks, kind = _normalise(signal, mask)
    seg = plan_segments(masks, w, p)
    info, hist = _solve_segments(
        sigs, seg, device, "iters",
        lambda sol: ops.janssen(sol, seg.n, seg.gap_start, seg.gap_len, p, maxit,
                                return_history=return_history, method=method))
    for r, d in enumerate(info):
        d["history"] = hist[r, :, :int(seg.gap_len[r])].copy() if hist is not None else None
    out = restack(sigs, kind)
    return (out, info) if return_history else out


def janssen_inpaint_mask(signal, mask=None, p=512, w=4096, maxit=20, return_history=False,
                         device="cuda", method="lpc"):
    """janssen_inpaint for any mask: gaps closer than w to one another share a
    segment and are solved together, as the reference's janssen_inp.m does with
    any NaN pattern.  Input layouts, mask / NaN conventions and the return
    layout are janssen_inpaint's, and wherever that accepts the input the
    result is the same bits: a cluster of one run goes to the same launch
    (ops.janssen, the Toeplitz solver), all others to one launch of
    ops.janssen_mask (banded Cholesky).  return_history: also a list with one
    dict per cluster (signal, start, end: the hull of its missing samples,
    missing: their indices in the signal, iters, history [maxit, h]: the
    missing samples after every iteration, NaN for iterations not completed).
    """
    import torch
    from . import ops
    check_args(p, maxit)
    method_id(method)
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_mask_segments(masks, w, p)
    one = np.flatnonzero(plan.runs == 1)
    many = np.flatnonzero(plan.runs > 1)
    info = [None] * len(plan)
    # every row is cut before anything is written back (no segment holds a
    # missing sample of another cluster, so the order would not matter)
    seg = Segments(plan.signal[one], plan.lo[one], plan.n[one],
                   np.array([plan.missing[r][0] for r in one], np.int32),
                   np.array([len(plan.missing[r]) for r in one], np.int32))
    batch = None
    if len(many):
        batch = np.zeros((len(many), int(plan.n[many].max())), np.float64)
        for k, r in enumerate(many):
            lo, n = int(plan.lo[r]), int(plan.n[r])
            batch[k, :n] = sigs[plan.signal[r]][lo:lo + n]
    got, hist = _solve_segments(
        sigs, seg, device, "iters",
        lambda sol: ops.janssen(sol, seg.n, seg.gap_start, seg.gap_len, p, maxit,
                                return_history=return_history, method=method))
    for k, (r, d) in enumerate(zip(one, got)):
        d["missing"] = np.arange(d["start"], d["end"])
        d["history"] = hist[k, :, :int(seg.gap_len[k])].copy() if hist is not None else None
        info[r] = d
    if batch is not None:
        sol = torch.from_numpy(batch).to(device)
        lists = [plan.missing[r] for r in many]
        count, hist = ops.janssen_mask(sol, plan.n[many], lists, p, maxit,
                                       return_history=return_history, method=method)
        sol, count = sol.cpu().numpy(), count.cpu().numpy()
        hist = hist.cpu().numpy() if hist is not None else None
        for k, r in enumerate(many):
            idx = plan.missing[r].astype(np.int64)
            where = int(plan.lo[r]) + idx
            sigs[plan.signal[r]][where] = sol[k, idx]
            info[r] = {"signal": int(plan.signal[r]), "start": int(where[0]),
                       "end": int(where[-1]) + 1, "iters": int(count[k]), "missing": where,
                       "history": hist[k, :, :len(idx)].copy() if hist is not None else None}
    out = restack(sigs, kind)
    return (out, info) if return_history else out


def ar_extrapolate(signal, mask=None, p=512, w=4096, method="lpc", return_status=False,
                   device="cuda"):
    """Fill every gap of `signal` by forward/backward AR extrapolation on the
    GPU (the reference's arinpaint.m): the at most w samples before the gap are
    predicted forwards, those after it backwards, and the two are cross-faded
    with cos^2 weights.  Input layouts, mask / NaN conventions and the return
    layout are janssen_inpaint's.  Both contexts (clipped to the signal and to
    w) must be longer than p and free of other gaps.  return_status: also a
    list with one dict per gap (signal, start, end, status: 1, or 0 when a side
    had a constant context and predicted its mean).
    """
    from . import ops
    check_args(p, 1)
    method_id(method)
    sigs, masks, kind = _normalise(signal, mask)
    seg = plan_segments(masks, w, p)
    for r in range(len(seg)):
        pre, post = int(seg.gap_start[r]), int(seg.n[r] - seg.gap_start[r] - seg.gap_len[r])
        if min(pre, post) <= p:
            a = int(seg.lo[r] + seg.gap_start[r])
            raise ValueError(f"signal {seg.signal[r]}: the gap [{a}, {a + int(seg.gap_len[r])}) "
                             f"has contexts of {pre} and {post} samples, both need more than "
                             f"p = {p}")
    info, _ = _solve_segments(
        sigs, seg, device, "status",
        lambda sol: (ops.ar_extrapolate(sol, seg.n, seg.gap_start, seg.gap_len, p, w,
                                        method=method), None))
    out = restack(sigs, kind)
    return (out, info) if return_status else out


# ------------------------------------------------------------ window-wise
# utils/segmentation_inp.m as train.m:146-172 drives it (the janssen_hann,
# janssen_rect and janssen_tukey rows), restated without LTFAT: DESIGN §14.
W_MAX = N_MAX


def gap_support(start, end, w, a):
    """[lo, hi) (0-based, may leave the signal) that train.m:147-150 hands to
    segmentation_inp for the gap [start, end): offset(s, f, a, 'half') and
    min_sig_supp_2(w, a, 0, s, f, N, 1, off) with s = start + 1, f = end."""
    s, f = start + 1, end
    c = _cdiv(s + f, 2)
    off = c - (1 + ((c - 1) // a) * a + _cdiv(a, 2))
    first = _cdiv(s - _cdiv(w, 2), a) + 1
    mid = 1 + (first - 1) * a + off % a          # centre of the first window on the gap
    if mid - a + _cdiv(w, 2) - 1 >= s:
        mid -= a
    q = mid - _cdiv(w // 2, a) * a
    last = mid + ((f + w // 2 - mid) // a) * a
    Q = last + _cdiv(_cdiv(w, 2), a) * a
    return q - 1, Q - 1


def plan_windows(masks, p=512, w=4096, a=1024, wtypes=("hann",)):
    """The batch layout of the window-wise algorithm for a list of boolean
    observed masks and a sequence of window shapes.  ValueError for what is not
    covered: a not dividing w, w / a < 2, w not in (p, 16384], an overlap-add
    weight that is not positive, a window that holds a second gap, a run of
    more than 2048 missing samples."""
    w, a, p = int(w), int(a), int(p)
    check_shift(w, a)
    if not p < w <= W_MAX:
        raise ValueError(f"w must be in (p, {W_MAX}], got w = {w}, p = {p}")
    keys = tuple(wtype_key(t) for t in wtypes)
    if not keys or len(set(keys)) != len(keys):
        raise ValueError("wtype needs at least one shape, each once")
    pairs = window_pairs(keys, w, a)
    gaps = []
    for k in range(len(keys)):
        for i, obs in enumerate(masks):
            obs = np.asarray(obs, bool)
            for (g0, g1) in find_gaps(obs):
                lo, hi = gap_support(g0, g1, w, a)
                L = _cdiv(hi - lo, a) * a + (_cdiv(w, a) - 1) * a
                miss_any = np.zeros(L, bool)
                s0, s1 = max(lo, 0), min(hi, len(obs))
                miss_any[s0 - lo:s1 - lo] = ~obs[s0:s1]
                rows = []
                for row in window_rows(miss_any, g0 - lo, w, a, range(L // a), i, g0, g1):
                    if row[2] > GAP_MAX:
                        raise ValueError(f"signal {i}: a window holds {row[2]} missing samples, "
                                         f"at most {GAP_MAX}")
                    rows.append(row)
                gaps.append((k, i, g0, g1, lo, hi - lo, L, rows))
    return window_plan(keys, w, a, pairs, masks, gaps)


def janssen_windowed(signal, mask=None, p=512, w=4096, a=1024, wtype="hann", maxit=20,
                     method="lpc", return_history=False, device="cuda"):
    """Fill every gap of `signal` by the window-wise Janssen algorithm on the
    GPU (the reference's segmentation_inp.m on the support train.m:146-172
    gives it): windows of w samples every a samples around the gap, each with
    missing samples inpainted by Janssen, overlap-added and rescaled.

    Input layouts, mask / NaN conventions and the return layout are
    janssen_inpaint's; only missing samples are written.  wtype: "hann", "rect"
    or "tukey" (any case), or a sequence of them -- then the windows of all
    shapes share one Janssen launch and a dict {wtype: result} comes back (with
    return_history: {wtype: (result, history)}).  The history is one dict per
    gap (signal, start, end, iters: iterations completed per window with a row,
    history [maxit, gap_len]: the gap after every iteration, NaN from the
    iteration on that one of its windows did not complete).
    """
    from . import ops
    check_args(p, maxit)
    method_id(method)
    single = isinstance(wtype, str)
    shapes = (wtype,) if single else tuple(wtype)
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_windows(masks, p, w, a, shapes)
    keys = plan.wtypes
    res, iters, hist = solve_windows(
        sigs, plan, device,
        [(0, len(plan), lambda sol: ops.janssen(sol, np.full(len(plan), plan.w), plan.gap_start,
                                                plan.gap_len, p, maxit,
                                                return_history=return_history, method=method))])
    info = {k: [] for k in keys}
    for g in range(len(plan.gap_off)):
        h, _, _, row0, nrows, k = (int(v) for v in plan.gap_tab[g])
        info[keys[k]].append({"signal": int(plan.gap_signal[g]),
                              "start": int(plan.gap_range[g, 0]),
                              "end": int(plan.gap_range[g, 1]),
                              "iters": [int(v) for v in iters[row0:row0 + nrows]],
                              "history": hist[g, :, :h].copy() if hist is not None else None})
    out = {}
    for k, r in zip(keys, res):
        r = restack(r, kind)
        out[k] = (r, info[k]) if return_history else r
    return out[keys[0]] if single else out


# -------------------------------------------------- window-wise, any mask
# utils/segmentation_inp.m as it is written: called on a whole signal with any
# NaN pattern, one fixed grid of windows, no per-gap support.
def plan_windows_mask(masks, p=512, w=4096, a=1024, wtypes=("hann",)):
    """The batch layout of the window-wise algorithm on whole signals for a
    list of boolean observed masks of any pattern and a sequence of window
    shapes.  Signal i of n samples is padded to L = ceil(n / a) a + (w / a - 1) a
    and window s < L / a holds the circular indices (s a - floor(w / 2) + j) mod
    L; every window with some, not all, samples missing is a row, whatever the
    number of runs they form (a set split by the wrap counts as two runs).
    ValueError for what is not covered: what plan_windows refuses for w, a and
    p (a not dividing w, w / a < 2, w not in (p, 16384]), an overlap-add weight
    that is not positive, a window that holds more than 2048 missing samples.
    A run may be longer than w or than 2048: the windows inside it have no row."""
    w, a, p = int(w), int(a), int(p)
    check_shift(w, a)
    if not p < w <= W_MAX:
        raise ValueError(f"w must be in (p, {W_MAX}], got w = {w}, p = {p}")
    keys = tuple(wtype_key(t) for t in wtypes)
    if not keys or len(set(keys)) != len(keys):
        raise ValueError("wtype needs at least one shape, each once")
    pairs = window_pairs(keys, w, a)
    pos = np.arange(w)
    rows = []
    for i, obs in enumerate(masks):
        n = len(obs)
        L = _cdiv(n, a) * a + (_cdiv(w, a) - 1) * a
        miss = np.zeros(L, bool)
        miss[:n] = ~np.asarray(obs, bool)
        # missing samples per window from one prefix sum over the circle
        csum = np.concatenate(([0], np.cumsum(np.concatenate((miss, miss[:w])))))
        first = (np.arange(L // a) * a - w // 2) % L
        count = csum[first + w] - csum[first]
        if count.max(initial=0) > GAP_MAX:
            s = int(np.argmax(count))
            raise ValueError(f"signal {i}: window {s} holds {int(count[s])} missing samples, at "
                             f"most {GAP_MAX}")
        rows.append([(int(s), np.flatnonzero(miss[(first[s] + pos) % L]).astype(np.int32))
                     for s in np.flatnonzero((count > 0) & (count < w))])
    return mask_window_plan(keys, w, a, pairs, masks, rows)


def janssen_windowed_mask(signal, mask=None, p=512, w=4096, a=1024, wtype="hann", maxit=20,
                          method="lpc", return_history=False, device="cuda"):
    """Fill the missing samples of `signal`, in any pattern, by the window-wise
    Janssen algorithm on the GPU as the reference's segmentation_inp.m does on
    a whole signal: one grid of windows of w samples every a samples, anchored
    at the first sample and the same whatever the mask, every window with
    missing samples inpainted by Janssen (any number of gaps in it),
    overlap-added and rescaled.  It takes what janssen_windowed refuses --
    several gaps in one window, scattered samples -- and does not use train.m's
    per-gap supports, so its result is not janssen_windowed's.

    Input layouts, mask / NaN conventions, wtype (a string, or a sequence of
    shapes: a dict comes back), method and the return layout are
    janssen_windowed's; only missing samples are written.  Windows whose
    missing samples are one run go to ops.janssen (the Toeplitz solver), all
    others to ops.janssen_mask, one launch each.  The history is one dict per
    run of missing samples of the signal (signal, start, end, iters:
    iterations completed by each window with a row that covers the run, in
    ascending window order, history [maxit, end - start]: the run after every
    iteration, NaN from the iteration on that one of its windows did not
    complete).  ValueError: see plan_windows_mask.
    """
    from . import ops
    check_args(p, maxit)
    method_id(method)
    single = isinstance(wtype, str)
    shapes = (wtype,) if single else tuple(wtype)
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_windows_mask(masks, p, w, a, shapes)
    keys = plan.wtypes
    full = lambda rows: np.full(rows, plan.w)
    res, iters, hist = solve_windows(
        sigs, plan, device,
        [(0, plan.n_one,
          lambda sol: ops.janssen(sol, full(plan.n_one), plan.gap_start[:plan.n_one],
                                  plan.gap_len[:plan.n_one], p, maxit,
                                  return_history=return_history, method=method)),
         (plan.n_one, len(plan),
          lambda sol: ops.janssen_mask(sol, full(len(plan) - plan.n_one), plan.lists(), p, maxit,
                                       return_history=return_history, method=method))])
    info = {k: [] for k in keys}
    for g in range(len(plan.run_off)):
        h, c0, L, tab0, k = (int(v) for v in plan.run_tab[g])
        # the windows that hold a sample of the run, ascending
        S = L // plan.a
        lo, hi = _cdiv(c0 + plan.w // 2 - plan.w + 1, plan.a), (c0 + h - 1 + plan.w // 2) // plan.a
        cover = sorted({s % S for s in range(lo, hi + 1)})
        rows = [int(r) for r in plan.win_row[tab0:tab0 + S][cover] if r >= 0]
        history = None
        if return_history:
            history = hist[g, :, :h].copy() if hist is not None else np.zeros((int(maxit), h))
        info[keys[k]].append({"signal": int(plan.run_signal[g]), "start": c0, "end": c0 + h,
                              "iters": [int(iters[r]) for r in rows], "history": history})
    out = {}
    for k, r in zip(keys, res):
        r = restack(r, kind)
        out[k] = (r, info[k]) if return_history else r
    return out[keys[0]] if single else out
