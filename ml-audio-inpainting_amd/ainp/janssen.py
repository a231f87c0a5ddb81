"""Host side of the autoregressive baselines (models/AudioReg of the
reference: utils/janssen_inp.m and utils/arinpaint.m driven by train.m, with
method "lpc" or "arburg").

train.m cuts one segment of w samples either side of every gap and hands each
to janssen_inp; here every gap of every signal becomes one row of a batch and
the whole batch is one launch of ainp_janssen_ex (csrc/janssen.hip, float64)
or of ainp_ar_extrapolate (csrc/ar_extrapolate.hip).
Segments are clipped to the signal (train.m:134-135 indexes past the ends for
a gap within w of them).  gap_sdr is train.m:196 / model_eval.m:60.

The window-wise rows (utils/segmentation_inp.m on the support train.m:146-172
cuts with offset.m and min_sig_supp_2.m; Hann, rectangular and Tukey windows)
are plan_windows / janssen_windowed at the end of the file: every window with
missing samples, of every gap, signal and window shape, is one row of the same
ainp_janssen_ex launch, between the gather and the overlap-add of
csrc/janssen_windows.hip.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

P_MAX = 3072          # csrc/janssen.hip JN_PMAX
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


def _to_numpy(a):
    if hasattr(a, "detach"):            # torch.Tensor
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _normalise(signal, mask):
    """-> (list of float64 1-D signals with zeros on the gaps, list of boolean
    observed masks, kind) with kind in 'single' | 'list' | 'batch'."""
    if isinstance(signal, (list, tuple)):
        sigs, kind = [_to_numpy(s) for s in signal], "list"
    else:
        a = _to_numpy(signal)
        if a.ndim == 1:
            sigs, kind = [a], "single"
        elif a.ndim == 2:
            sigs, kind = list(a), "batch"
        else:
            raise ValueError("signal must be 1-D, a list of 1-D signals or a 2-D batch")
    if mask is None:
        masks = [None] * len(sigs)
    elif kind == "list":
        if not isinstance(mask, (list, tuple)) or len(mask) != len(sigs):
            raise ValueError("mask must be a list with one mask per signal")
        masks = [_to_numpy(m) for m in mask]
    else:
        m = _to_numpy(mask)
        masks = [m] if kind == "single" else list(np.broadcast_to(m, (len(sigs),) + m.shape[-1:]))
    out_s, out_m = [], []
    for s, m in zip(sigs, masks):
        if s.ndim != 1:
            raise ValueError("every signal must be 1-D")
        s = s.astype(np.float64)
        obs = ~np.isnan(s)               # NaN marks missing, as janssen_inp.m:61
        if m is not None:
            if m.shape != s.shape:
                raise ValueError("mask and signal differ in length")
            obs &= m.astype(bool)
        if not np.all(np.isfinite(s[obs])):
            raise ValueError("observed samples must be finite")
        s[~obs] = 0.0
        out_s.append(s)
        out_m.append(obs)
    return out_s, out_m, kind


def find_gaps(observed):
    """[(start, end)) of every run of missing samples."""
    miss = np.concatenate(([False], ~np.asarray(observed, bool), [False]))
    edges = np.flatnonzero(miss[1:] != miss[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


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


def check_args(p, maxit):
    if not 1 <= int(p) <= P_MAX:
        raise ValueError(f"p must be in [1, {P_MAX}]")
    if not 1 <= int(maxit) <= MAXIT_MAX:
        raise ValueError(f"maxit must be in [1, {MAXIT_MAX}]")


def _batch(sigs, seg):
    """One zero-padded float64 row per segment."""
    batch = np.zeros((len(seg), int(seg.n.max())), np.float64)
    for r in range(len(seg)):
        s = sigs[seg.signal[r]]
        batch[r, :seg.n[r]] = s[seg.lo[r]:seg.lo[r] + seg.n[r]]
    return batch


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
    import torch
    from . import ops
    check_args(p, maxit)
    method_id(method)
    sigs, masks, kind = _normalise(signal, mask)
    seg = plan_segments(masks, w, p)
    info = []
    if len(seg):
        sol = torch.from_numpy(_batch(sigs, seg)).to(device)
        iters, hist = ops.janssen(sol, seg.n, seg.gap_start, seg.gap_len, p, maxit,
                                  return_history=return_history, method=method)
        sol, iters = sol.cpu().numpy(), iters.cpu().numpy()
        hist = hist.cpu().numpy() if hist is not None else None
        for r in range(len(seg)):
            a, h = int(seg.gap_start[r]), int(seg.gap_len[r])
            lo = int(seg.lo[r])
            sigs[seg.signal[r]][lo + a:lo + a + h] = sol[r, a:a + h]
            info.append({"signal": int(seg.signal[r]), "start": lo + a, "end": lo + a + h,
                         "iters": int(iters[r]),
                         "history": hist[r, :, :h].copy() if hist is not None else None})
    out = sigs[0] if kind == "single" else sigs if kind == "list" else np.stack(sigs)
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
    import torch
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
    info = []
    if len(seg):
        sol = torch.from_numpy(_batch(sigs, seg)).to(device)
        status = ops.ar_extrapolate(sol, seg.n, seg.gap_start, seg.gap_len, p, w, method=method)
        sol, status = sol.cpu().numpy(), status.cpu().numpy()
        for r in range(len(seg)):
            a, h = int(seg.gap_start[r]), int(seg.gap_len[r])
            lo = int(seg.lo[r])
            sigs[seg.signal[r]][lo + a:lo + a + h] = sol[r, a:a + h]
            info.append({"signal": int(seg.signal[r]), "start": lo + a, "end": lo + a + h,
                         "status": int(status[r])})
    out = sigs[0] if kind == "single" else sigs if kind == "list" else np.stack(sigs)
    return (out, info) if return_status else out


def gap_sdr(clean, restored, mask):
    """10 log10(sum_M clean^2 / sum_M (clean - restored)^2) over the missing
    samples M (mask True / 1 where observed), in dB; host float64."""
    clean = _to_numpy(clean).astype(np.float64)
    restored = _to_numpy(restored).astype(np.float64)
    miss = ~_to_numpy(mask).astype(bool)
    if clean.shape != restored.shape or clean.shape != miss.shape:
        raise ValueError("clean, restored and mask must have one shape")
    num = np.sum(clean[miss] ** 2)
    den = np.sum((clean[miss] - restored[miss]) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(num / den))


# ------------------------------------------------------------ window-wise
# utils/segmentation_inp.m as train.m:146-172 drives it (the janssen_hann,
# janssen_rect and janssen_tukey rows), restated without LTFAT: DESIGN §14.
WTYPES = ("hann", "rect", "tukey")
W_MAX = N_MAX


def wtype_key(wtype):
    """segmentation_inp's `wtype` ("hann" | "rect" | "tukey", any case as
    strcmpi) -> its lower-case name."""
    key = wtype.lower() if isinstance(wtype, str) else wtype
    if key not in WTYPES:
        raise ValueError(f"wtype must be one of {sorted(WTYPES)}, got {wtype!r}")
    return key


def _cdiv(x, y):
    return -((-x) // y)


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


def window_pair(wtype, w, a):
    """(gana, gsyn) of segmentation_inp.m:74-87, float64 [w].  hann: the
    periodic Hann and its painless dual for the shift a; rect: ones and that
    Hann; tukey: MATLAB tukeywin(w) (r = 0.5) for both."""
    key = wtype_key(wtype)
    i = np.arange(w, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / w)
    if key == "rect":
        return np.ones(w), hann
    if key == "tukey":
        t = np.linspace(0.0, 1.0, w)
        g = np.ones(w)
        lo, hi = t < 0.25, t >= 0.75
        g[lo] = 0.5 * (1.0 + np.cos(4.0 * np.pi * (t[lo] - 0.25)))
        g[hi] = 0.5 * (1.0 + np.cos(4.0 * np.pi * (t[hi] - 0.75)))
        return g, g.copy()
    idx = np.arange(w)
    den = np.zeros(w)
    for k in range(w // a):
        den += hann[(idx - k * a) % w] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return hann, hann / den


def window_rescale(gana, gsyn, a):
    """The overlap-add weight sum_k (gana gsyn)[m + k a] per residue m of the
    window index modulo a (segmentation_inp.m's `rescale`, which repeats with
    period a on the circular support)."""
    return (gana * gsyn).reshape(-1, a).sum(axis=0)


@dataclass
class WindowPlan:
    """The tables of one window-wise call.  Signals lie end to end in one
    buffer, once per window shape (shape-major).  One row per window that
    holds some, not all, missing samples; one gap entry per (shape, signal,
    gap); a gap's rows are consecutive, in ascending window order."""
    wtypes: tuple
    w: int
    a: int
    total: int
    gana: np.ndarray          # [n_shapes, w]
    gsyn: np.ndarray
    sig_off: np.ndarray       # int64 [n_rows]
    row_tab: np.ndarray       # int32 [n_rows, 6]: sig_len, origin, sup_len, L, window, shape
    gap_start: np.ndarray     # int32 [n_rows], relative to the window
    gap_len: np.ndarray
    gap_off: np.ndarray       # int64 [n_gaps]
    gap_tab: np.ndarray       # int32 [n_gaps, 6]: h, c0, L, row0, n_rows, shape
    gap_signal: np.ndarray    # int32 [n_gaps]
    gap_range: np.ndarray     # int32 [n_gaps, 2]: [start, end) in the signal

    def __len__(self):
        return len(self.sig_off)


def plan_windows(masks, p=512, w=4096, a=1024, wtypes=("hann",)):
    """The batch layout of the window-wise algorithm for a list of boolean
    observed masks and a sequence of window shapes.  ValueError for what is not
    covered: a not dividing w, w / a < 2, w not in (p, 16384], an overlap-add
    weight that is not positive, a window that holds a second gap, a run of
    more than 2048 missing samples."""
    w, a, p = int(w), int(a), int(p)
    if a < 1 or w < 1 or w % a:
        raise ValueError(f"the shift a = {a} must divide the window length w = {w}")
    if w // a < 2:
        raise ValueError(f"w / a must be at least 2, got w = {w}, a = {a}")
    if not p < w <= W_MAX:
        raise ValueError(f"w must be in (p, {W_MAX}], got w = {w}, p = {p}")
    keys = tuple(wtype_key(t) for t in wtypes)
    if not keys or len(set(keys)) != len(keys):
        raise ValueError("wtype needs at least one shape, each once")
    pairs = [window_pair(k, w, a) for k in keys]
    for k, (ga, gs) in zip(keys, pairs):
        r = window_rescale(ga, gs, a)
        if not (np.all(np.isfinite(gs)) and np.all(np.isfinite(r)) and np.all(r > 0)):
            raise ValueError(f"wtype {k!r} with w = {w}, a = {a}: the overlap-add weight is not "
                             "positive everywhere")
    lens = [len(m) for m in masks]
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    per_shape = int(starts[-1])
    sig_off, row_tab, gap_start, gap_len = [], [], [], []
    gap_off, gap_tab, gap_signal, gap_range = [], [], [], []
    pos = np.arange(w)
    for k in range(len(keys)):
        for i, obs in enumerate(masks):
            obs = np.asarray(obs, bool)
            base = k * per_shape + int(starts[i])
            for (g0, g1) in find_gaps(obs):
                lo, hi = gap_support(g0, g1, w, a)
                n = hi - lo
                L = _cdiv(n, a) * a + (_cdiv(w, a) - 1) * a
                miss_any = np.zeros(L, bool)
                s0, s1 = max(lo, 0), min(hi, len(obs))
                miss_any[s0 - lo:s1 - lo] = ~obs[s0:s1]
                miss = np.zeros(L, bool)
                miss[g0 - lo:g1 - lo] = True
                row0 = len(sig_off)
                for s in range(L // a):
                    idx = (s * a - w // 2 + pos) % L
                    m = miss[idx]
                    if not m.any():
                        continue
                    if np.count_nonzero(miss_any[idx]) != np.count_nonzero(m):
                        raise ValueError(f"signal {i}: a window around the gap [{g0}, {g1}) holds "
                                         "a second gap; one run of missing samples per window "
                                         "only")
                    if m.all():
                        continue                  # zeros in the sum, counted by the rescale
                    runs = find_gaps(~m)
                    if len(runs) != 1:
                        raise ValueError(f"signal {i}: the gap [{g0}, {g1}) falls into two runs "
                                         "of one window")
                    if runs[0][1] - runs[0][0] > GAP_MAX:
                        raise ValueError(f"signal {i}: a window holds {runs[0][1] - runs[0][0]} "
                                         f"missing samples, at most {GAP_MAX}")
                    sig_off.append(base)
                    row_tab.append((len(obs), lo, n, L, s, k))
                    gap_start.append(runs[0][0])
                    gap_len.append(runs[0][1] - runs[0][0])
                gap_off.append(base + g0)
                gap_tab.append((g1 - g0, g0 - lo, L, row0, len(sig_off) - row0, k))
                gap_signal.append(i)
                gap_range.append((g0, g1))
    i32 = lambda v, cols=None: np.array(v, dtype=np.int32).reshape((-1,) if cols is None
                                                                  else (-1, cols))
    return WindowPlan(keys, w, a, per_shape * len(keys),
                      np.stack([g for g, _ in pairs]), np.stack([g for _, g in pairs]),
                      np.array(sig_off, dtype=np.int64), i32(row_tab, 6), i32(gap_start),
                      i32(gap_len), np.array(gap_off, dtype=np.int64), i32(gap_tab, 6),
                      i32(gap_signal), i32(gap_range, 2))


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
    import torch
    from . import ops
    check_args(p, maxit)
    method_id(method)
    single = isinstance(wtype, str)
    shapes = (wtype,) if single else tuple(wtype)
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_windows(masks, p, w, a, shapes)
    keys, ns = plan.wtypes, len(sigs)
    buf = np.concatenate([s for _ in keys for s in sigs]) if ns else np.zeros(0)
    info = {k: [] for k in keys}
    if len(plan):
        dbuf = torch.from_numpy(buf).to(device)
        sol = ops.janssen_windows(dbuf, plan.sig_off, plan.row_tab, plan.gap_start,
                                  plan.gap_len, plan.w, plan.a, plan.gana)
        iters, rhist = ops.janssen(sol, np.full(len(plan), plan.w), plan.gap_start, plan.gap_len,
                                   p, maxit, return_history=return_history, method=method)
        hist = ops.janssen_ola(sol, rhist, plan.row_tab, plan.gap_start, plan.gap_len,
                               plan.gap_off, plan.gap_tab, plan.a, plan.gana, plan.gsyn, dbuf)
        buf, iters = dbuf.cpu().numpy(), iters.cpu().numpy()
        hist = hist.cpu().numpy() if hist is not None else None
        for g in range(len(plan.gap_off)):
            h, _, _, row0, nrows, k = (int(v) for v in plan.gap_tab[g])
            info[keys[k]].append({"signal": int(plan.gap_signal[g]),
                                  "start": int(plan.gap_range[g, 0]),
                                  "end": int(plan.gap_range[g, 1]),
                                  "iters": [int(v) for v in iters[row0:row0 + nrows]],
                                  "history": hist[g, :, :h].copy() if hist is not None else None})
    out, at = {}, 0
    for k in keys:
        res = []
        for s in sigs:
            res.append(buf[at:at + len(s)].copy())
            at += len(s)
        res = res[0] if kind == "single" else res if kind == "list" else np.stack(res)
        out[k] = (res, info[k]) if return_history else res
    return out[keys[0]] if single else out
