"""What the host sides of the audio-regression algorithms share (ainp/janssen.py,
ainp/spain.py): the input layouts and the gap SDR, the windows of
utils/segmentation_inp.m, and the window-wise batch -- the rows a gap makes on
a circular support (window_rows), the plan of a call with one support per gap
(WindowPlan, window_plan) and of one on whole signals with any mask
(MaskWindowPlan, mask_window_plan), the device tables of
csrc/janssen_windows.hip that either gives (WindowTables, tables()) and the
launches around the solvers (solve_windows).
"""
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

WTYPES = ("hann", "rect", "tukey")


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


def restack(sigs, kind):
    """The per-signal results in the layout _normalise found the input in."""
    return sigs[0] if kind == "single" else sigs if kind == "list" else np.stack(sigs)


def find_gaps(observed):
    """[(start, end)) of every run of missing samples."""
    miss = np.concatenate(([False], ~np.asarray(observed, bool), [False]))
    edges = np.flatnonzero(miss[1:] != miss[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def _cdiv(x, y):
    return -((-x) // y)


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


# ---------------------------------------------------------------- windows
def wtype_key(wtype):
    """segmentation_inp's `wtype` ("hann" | "rect" | "tukey", any case as
    strcmpi) -> its lower-case name."""
    key = wtype.lower() if isinstance(wtype, str) else wtype
    if key not in WTYPES:
        raise ValueError(f"wtype must be one of {sorted(WTYPES)}, got {wtype!r}")
    return key


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


def check_shift(w, a):
    """The shift the window-wise layout takes: a divides w, w / a >= 2."""
    if a < 1 or w < 1 or w % a:
        raise ValueError(f"the shift a = {a} must divide the window length w = {w}")
    if w // a < 2:
        raise ValueError(f"w / a must be at least 2, got w = {w}, a = {a}")


def window_pairs(keys, w, a, name_shape=True):
    """The window pairs of `keys`; ValueError unless every overlap-add weight is positive."""
    pairs = [window_pair(k, w, a) for k in keys]
    for k, (ga, gs) in zip(keys, pairs):
        r = window_rescale(ga, gs, a)
        if not (np.all(np.isfinite(gs)) and np.all(np.isfinite(r)) and np.all(r > 0)):
            raise ValueError((f"wtype {k!r} with " if name_shape else "") + f"w = {w}, a = {a}: "
                             "the overlap-add weight is not positive everywhere")
    return pairs


class WindowTables(NamedTuple):
    """The device tables of the gather and the overlap-add (include/ainp.h), as
    host arrays: what ops.janssen_windows and ops.janssen_ola take."""
    missing: np.ndarray       # uint8 [total], 1 on a missing sample
    sig_off: np.ndarray       # int64 [n_rows]
    row_tab: np.ndarray       # int32 [n_rows, 6]: sig_len, origin, sup_len, L, window, shape
    gap_start: np.ndarray     # int32 [n_rows], relative to the window
    gap_len: np.ndarray       # int32 [n_rows]: >= 1 a row of one run, 0 a row with a list
    miss_off: np.ndarray      # int32 [n_rows + 1]
    miss_idx: np.ndarray      # int32, window positions, ascending per row
    win_row: np.ndarray       # int32: per support and shape the row of each window, -1: none
    unit_off: np.ndarray      # int64 [n_units]
    unit_tab: np.ndarray      # int32 [n_units, 5]: h, c0, L, tab0, shape


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

    def tables(self):
        """Every gap is a unit with a support of its own: its window-to-row
        table is one segment of L / a entries, its rows have one run each."""
        h, c0, L, row0, n_rows, shape = self.gap_tab.T.astype(np.int64)
        tab0 = np.concatenate(([0], np.cumsum(L // self.a)))
        missing = np.zeros(self.total, np.uint8)
        win_row = np.full(int(tab0[-1]), -1, np.int32)
        for g in range(len(h)):
            missing[self.gap_off[g]:self.gap_off[g] + h[g]] = 1
            rows = np.arange(row0[g], row0[g] + n_rows[g])
            win_row[tab0[g] + self.row_tab[rows, 4]] = rows
        unit_tab = np.stack((h, c0, L, tab0[:-1], shape), axis=1).astype(np.int32)
        return WindowTables(missing, self.sig_off, self.row_tab, self.gap_start, self.gap_len,
                            np.zeros(len(self) + 1, np.int32), np.zeros(0, np.int32), win_row,
                            self.gap_off, unit_tab)


def window_rows(miss_any, c0, w, a, windows, i, g0, g1):
    """(window, run_start, run_len) for every window of `windows` (ascending)
    that holds some, not all, samples of the gap [g0, g1) of signal i.
    miss_any: the missing samples of the circular support, boolean [L]; the gap
    starts at c0 in it; window n holds the indices (n a - floor(w / 2) + j) mod
    L.  ValueError for a window that holds a second gap or the gap in two runs."""
    L = len(miss_any)
    miss = np.zeros(L, bool)
    miss[c0:c0 + g1 - g0] = True
    pos = np.arange(w)
    for n in windows:
        idx = (n * a - w // 2 + pos) % L
        m = miss[idx]
        if not m.any():
            continue
        if np.count_nonzero(miss_any[idx]) != np.count_nonzero(m):
            raise ValueError(f"signal {i}: a window around the gap [{g0}, {g1}) holds a second "
                             "gap; one run of missing samples per window only")
        if m.all():
            continue                      # zeros in the sum, counted by the rescale
        runs = find_gaps(~m)
        if len(runs) != 1:
            raise ValueError(f"signal {i}: the gap [{g0}, {g1}) falls into two runs of one "
                             "window")
        yield n, runs[0][0], runs[0][1] - runs[0][0]


def window_plan(keys, w, a, pairs, masks, gaps):
    """The WindowPlan of `gaps`: one (shape, signal, g0, g1, origin, sup_len, L,
    rows) per gap in table order -- the support [origin, origin + sup_len) of
    its signal, padded to L, and the rows window_rows gave."""
    starts = np.concatenate(([0], np.cumsum([len(m) for m in masks]))).astype(np.int64)
    per_shape = int(starts[-1])
    sig_off, row_tab, gap_start, gap_len = [], [], [], []
    gap_off, gap_tab, gap_signal, gap_range = [], [], [], []
    for k, i, g0, g1, origin, sup_len, L, rows in gaps:
        base = k * per_shape + int(starts[i])
        gap_off.append(base + g0)
        gap_tab.append((g1 - g0, g0 - origin, L, len(sig_off), len(rows), k))
        gap_signal.append(i)
        gap_range.append((g0, g1))
        for n, start, length in rows:
            sig_off.append(base)
            row_tab.append((len(masks[i]), origin, sup_len, L, n, k))
            gap_start.append(start)
            gap_len.append(length)
    i32 = lambda v, cols=None: np.array(v, dtype=np.int32).reshape((-1,) if cols is None
                                                                  else (-1, cols))
    return WindowPlan(tuple(keys), w, a, per_shape * len(keys),
                      np.stack([g for g, _ in pairs]), np.stack([g for _, g in pairs]),
                      np.array(sig_off, dtype=np.int64), i32(row_tab, 6), i32(gap_start),
                      i32(gap_len), np.array(gap_off, dtype=np.int64), i32(gap_tab, 6),
                      i32(gap_signal), i32(gap_range, 2))


def solve_windows(sigs, plan, device, parts, per_gap=True):
    """The launches of a window-wise call: the signals, end to end once per
    shape, and their byte mask go to the device; ops.janssen_windows gathers
    the rows; every (first, end, solve) of `parts` with rows in it runs
    solve(sol[first:end]) -> (iters, history or None) in place, once;
    ops.janssen_ola adds the rows back (per_gap: and turns their history into
    the units', else the rows' own history comes back untouched).  -> (per shape
    the per-signal results, iters per row, history) as numpy.  A plan without
    rows launches nothing: its missing samples, if any, belong to windows that
    are all missing and stay zero; iters is empty, the history None."""
    import torch
    from . import ops
    buf = np.concatenate([s for _ in plan.wtypes for s in sigs]) if sigs else np.zeros(0)
    iters, hist = np.zeros(0, np.int32), None
    if len(plan):
        tables = plan.tables()
        dbuf = torch.from_numpy(buf).to(device)
        sol = ops.janssen_windows(dbuf, torch.from_numpy(tables.missing).to(device), tables,
                                  plan.w, plan.a, plan.gana)
        done = [solve(sol[first:end]) for first, end, solve in parts if end > first]
        iters, hist = torch.cat([it for it, _ in done]), done[0][1]
        if len(done) > 1 and hist is not None:
            # the solvers' histories side by side, NaN beyond a row's list
            hist = torch.full((len(plan), hist.shape[1], max(h.shape[2] for _, h in done)),
                              float("nan"), device=sol.device, dtype=torch.float64)
            at = 0
            for _, h in done:
                hist[at:at + h.shape[0], :, :h.shape[2]] = h
                at += h.shape[0]
        units = ops.janssen_ola(sol, hist if per_gap else None, tables, plan.a, plan.gana,
                                plan.gsyn, dbuf)
        hist = units if per_gap else hist
        buf, iters = dbuf.cpu().numpy(), iters.cpu().numpy()
        hist = hist.cpu().numpy() if hist is not None else None
    out, at = [], 0
    for _ in plan.wtypes:
        out.append([])
        for s in sigs:
            out[-1].append(buf[at:at + len(s)].copy())
            at += len(s)
    return out, iters, hist


# ---------------------------------------------------------------- any mask
@dataclass
class MaskWindowPlan:
    """The tables of one window-wise call on whole signals with any mask.
    Signals lie end to end in one buffer, once per window shape (shape-major);
    signal i is its own support (origin 0, sup_len its length), padded to the
    circular length L_i, and has S_i = L_i / a windows whatever its mask.
    One row per window that holds some, not all, missing samples: first the
    rows whose missing samples are one run in window order (rows [0, n_one),
    gap_start / gap_len), then the rows with a list (gap_len 0, miss_off /
    miss_idx); within each part by shape, signal and window.  One run entry
    per (shape, signal, run of missing samples of the signal)."""
    wtypes: tuple
    w: int
    a: int
    total: int
    gana: np.ndarray          # [n_shapes, w]
    gsyn: np.ndarray
    missing: np.ndarray       # uint8 [total], 1 on a missing sample
    sig_off: np.ndarray       # int64 [n_rows]
    row_tab: np.ndarray       # int32 [n_rows, 6]: sig_len, origin 0, sup_len, L, window, shape
    n_one: int
    gap_start: np.ndarray     # int32 [n_rows], relative to the window
    gap_len: np.ndarray
    miss_off: np.ndarray      # int32 [n_rows + 1]
    miss_idx: np.ndarray      # int32, window positions, ascending per row
    win_row: np.ndarray       # int32: per (shape, signal) the row of each window, -1: none
    run_off: np.ndarray       # int64 [n_runs]
    run_tab: np.ndarray       # int32 [n_runs, 5]: h, c0, L, tab0, shape
    run_signal: np.ndarray    # int32 [n_runs]

    def __len__(self):
        return len(self.sig_off)

    def lists(self):
        """The missing lists of the rows [n_one, n_rows)."""
        return [self.miss_idx[self.miss_off[r]:self.miss_off[r + 1]]
                for r in range(self.n_one, len(self))]

    def tables(self):
        """Every run of missing samples of a signal is a unit."""
        return WindowTables(self.missing, self.sig_off, self.row_tab, self.gap_start,
                            self.gap_len, self.miss_off, self.miss_idx, self.win_row,
                            self.run_off, self.run_tab)


def mask_window_plan(keys, w, a, pairs, masks, rows):
    """The MaskWindowPlan of `rows`: per signal the (window, missing positions
    in the window, ascending) of every window with a row, in window order."""
    starts = np.concatenate(([0], np.cumsum([len(m) for m in masks]))).astype(np.int64)
    per_shape = int(starts[-1])
    Ls = [_cdiv(len(m), a) * a + (_cdiv(w, a) - 1) * a for m in masks]
    one, many = [], []
    for k in range(len(keys)):
        for i, sig_rows in enumerate(rows):
            for n, where in sig_rows:
                run = int(where[-1]) - int(where[0]) + 1 == len(where)
                (one if run else many).append((k, i, n, where))
    order = one + many
    # the window-to-row table of (shape k, signal i) starts at tab0[k * len(masks) + i]
    tab0 = np.concatenate(([0], np.cumsum([L // a for L in Ls] * len(keys)))).astype(np.int64)
    win_row = np.full(int(tab0[-1]), -1, np.int32)
    for r, (k, i, n, _) in enumerate(order):
        win_row[tab0[k * len(masks) + i] + n] = r
    run_off, run_tab, run_signal = [], [], []
    for k in range(len(keys)):
        for i, m in enumerate(masks):
            for g0, g1 in find_gaps(m):
                run_off.append(k * per_shape + int(starts[i]) + g0)
                run_tab.append((g1 - g0, g0, Ls[i], int(tab0[k * len(masks) + i]), k))
                run_signal.append(i)
    i32 = lambda v, cols=None: np.array(v, dtype=np.int32).reshape((-1,) if cols is None
                                                                  else (-1, cols))
    lists = [np.zeros(0, np.int32)] * len(one) + [np.asarray(wh, np.int32) for *_, wh in many]
    miss_off = np.zeros(len(order) + 1, np.int32)
    np.cumsum([len(v) for v in lists], out=miss_off[1:])
    missing = np.concatenate([~np.asarray(m, bool) for m in masks]) if masks else np.zeros(0, bool)
    return MaskWindowPlan(
        tuple(keys), w, a, per_shape * len(keys),
        np.stack([g for g, _ in pairs]), np.stack([g for _, g in pairs]),
        np.tile(missing.astype(np.uint8), len(keys)),
        np.array([k * per_shape + int(starts[i]) for k, i, _, _ in order], dtype=np.int64),
        i32([(len(masks[i]), 0, len(masks[i]), Ls[i], n, k) for k, i, n, _ in order], 6),
        len(one),
        i32([wh[0] for *_, wh in one] + [0] * len(many)),
        i32([len(wh) for *_, wh in one] + [0] * len(many)),
        miss_off, np.concatenate(lists) if lists else np.zeros(0, np.int32), win_row,
        np.array(run_off, dtype=np.int64), i32(run_tab, 5), i32(run_signal))
