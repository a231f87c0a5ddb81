"""Host side of the autoregressive baselines (models/AudioReg of the
reference: utils/janssen_inp.m and utils/arinpaint.m driven by train.m, with
method "lpc" or "arburg").

train.m cuts one segment of w samples either side of every gap and hands each
to janssen_inp; here every gap of every signal becomes one row of a batch and
the whole batch is one launch of ainp_janssen_ex (csrc/janssen.hip, float64)
or of ainp_ar_extrapolate (csrc/ar_extrapolate.hip).
Segments are clipped to the signal (train.m:134-135 indexes past the ends for
a gap within w of them).  gap_sdr is train.m:196 / model_eval.m:60.
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
