"""Short-time objective intelligibility on the GPU: STOI (Taal, Hendriks,
Heusdens, Jensen, IEEE TASL 19(7), 2011) and ESTOI (Jensen, Taal, IEEE/ACM
TASLP 24(11), 2016), the intelligibility column beside the gap SDR of the
reference's comparison table (models/AudioReg/train.m:35-41, 183-213).

The measure is defined at 10 kHz (csrc/stoi.hip, include/ainp.h: ainp_stoi;
DESIGN §17 states it in full); signals at another rate go through
ops.resample_poly in float64 first.  The unit is a batch: many restored
signals per clean signal in one call, the clean side (the silent-frame
decision and the clean band envelopes) done once.  stoi scores signals,
stoi_curve every iteration of a Janssen history.  plan restates
csrc/stoi_plan.h in Python (the tests hold it equal to the C query).
"""
from __future__ import annotations

import collections
import math

import numpy as np

from . import _lib
from .gaps import _normalise, _to_numpy, restack

FS = 10000
NF, HOP, NFFT = 256, 128, 512
J, N = 15, 30
BETA, DYN = -15.0, 40.0
EPS = 2.0 ** -52
SENTINEL = 1e-5
BAND = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)   # csrc/stoi_plan.h
MAX_LEN = 1 << 20     # STOI_MAX_LEN: samples of a row at 10 kHz
SEG = 64              # STOI_SEG

Plan = collections.namedtuple(
    "Plan", "max_len frames t_stride chunks keep_off env_off part_off bytes keep_lds")


def _up(n, m):
    return (n + m - 1) // m * m


def frames(length):
    """Frames of a row of `length` samples at 10 kHz."""
    return 0 if length < NF else (length - NF) // HOP + 1


def plan(n_clean, n_restored, max_len):
    """stoi_plan of csrc/stoi_plan.h: the workspace of a launch over n_clean
    clean and n_restored restored rows, the longest max_len samples; ValueError
    for negative counts or a row over MAX_LEN."""
    C, R, L = int(n_clean), int(n_restored), int(max_len)
    if C < 0 or R < 0 or not 0 <= L <= MAX_LEN:
        raise ValueError(f"counts must be >= 0 and max_len in [0, {MAX_LEN}], got {C}, {R}, {L}")
    K = frames(L)
    t_stride = _up(max(K, 1), 2)
    segs = K - N + 1
    chunks = -(-segs // SEG) if segs > 0 else 1
    keep_off = 0
    env_off = _up(4 * C * t_stride, 16)
    part_off = env_off + 8 * (C + R) * J * t_stride
    return Plan(MAX_LEN, K, t_stride, chunks, keep_off, env_off, part_off,
                part_off + _up(8 * R * chunks, 16), 8 * t_stride)


def query_plan(n_clean, n_restored, max_len):
    """The same through the C query (ainp_stoi_plan); AinpError for a refusal."""
    p = _lib.StoiPlan()
    _lib.check(_lib.lib.ainp_stoi_plan(int(n_clean), int(n_restored), int(max_len), p),
               "ainp_stoi_plan")
    return Plan(*(getattr(p, f) for f in Plan._fields))


def _lengths_at_10k(n, fs):
    """The rows' lengths after the resampling to 10 kHz; ValueError for fs < 1 or
    a row over MAX_LEN there.  Host only: the entry points call it before they
    touch the device."""
    from . import resample as rs
    fs = int(fs)
    if fs < 1:
        raise ValueError(f"fs must be positive, got {fs}")
    g = math.gcd(fs, FS)
    out = [int(v) if fs == FS else rs.out_len(int(v), FS // g, fs // g) for v in n]
    if out and max(out) > MAX_LEN:
        raise ValueError(f"a signal of {max(out)} samples at 10 kHz is over the limit of "
                         f"{MAX_LEN}")
    return out


def _score(rows, n, clean_row, n_clean, fs, extended):
    """rows [C + R, stride] float64 cuda at `fs`, clean rows first -> (score [R],
    frames [C]) on the device."""
    from . import ops
    fs = int(fs)
    n10 = _lengths_at_10k(n, fs)
    if fs != FS:
        g = math.gcd(fs, FS)
        lengths = [int(v) for v in n] + [int(n[c]) for c in clean_row]
        rows = ops.resample_poly(rows, FS // g, fs // g, n=lengths)
    return ops.stoi(rows[:n_clean], rows[n_clean:], n10, clean_row, extended)


def _restored_rows(restored, clean_len, what):
    r = _to_numpy(restored).astype(np.float64)
    if r.ndim not in (1, 2) or r.shape[-1] != clean_len:
        raise ValueError(f"{what}: restored must be [S] or [k, S] with S = {clean_len}, got "
                         f"{r.shape}")
    if not np.all(np.isfinite(r)):
        raise ValueError(f"{what}: restored samples must be finite")
    return r


def stoi(clean, restored, fs=16000, extended=False, device="cuda"):
    """STOI (extended: ESTOI) of restored signals against their clean signals.

    clean: 1-D, a list of 1-D signals, or a 2-D batch (numpy or torch), sampled
    at fs.  restored: the same layout, or k restored signals per clean one ([k, S]
    for a 1-D clean, a list of [S] / [k, S], [B, k, S] for a batch): all k are
    scored against the one clean signal, whose silent-frame decision and band
    envelopes are computed once.  Returns a float per pair (a [k] array per
    clean signal where k were given) in the layout of the input.  Signals with
    fewer than 30 kept frames score 1e-5.  Everything runs in one call of
    ops.stoi, after one of ops.resample_poly when fs is not 10000."""
    import torch
    sigs, _, kind = _normalise(clean, None)
    if kind == "list":
        if not isinstance(restored, (list, tuple)) or len(restored) != len(sigs):
            raise ValueError("restored must be a list with one entry per clean signal")
        rest = [_restored_rows(r, len(s), f"signal {i}")
                for i, (r, s) in enumerate(zip(restored, sigs))]
    elif kind == "single":
        rest = [_restored_rows(restored, len(sigs[0]), "signal")]
    else:
        r = _to_numpy(restored)
        if r.ndim not in (2, 3) or r.shape[0] != len(sigs):
            raise ValueError(f"restored must be [B, S] or [B, k, S] with B = {len(sigs)}")
        rest = [_restored_rows(r[i], len(s), f"signal {i}") for i, s in enumerate(sigs)]
    _lengths_at_10k([len(s) for s in sigs], fs)
    C = len(sigs)
    clean_row = [c for c, r in enumerate(rest) for _ in range(1 if r.ndim == 1 else len(r))]
    stride = max(2, _up(max((len(s) for s in sigs), default=0), 2))
    host = np.zeros((C + len(clean_row), stride), np.float64)
    for c, s in enumerate(sigs):
        host[c, :len(s)] = s
    k = C
    for r in rest:
        r2 = r.reshape(-1, r.shape[-1])
        host[k:k + len(r2), :r2.shape[1]] = r2
        k += len(r2)
    score, _ = _score(torch.from_numpy(host).to(device), [len(s) for s in sigs], clean_row, C, fs,
                      extended)
    score = score.cpu().numpy()
    out, k = [], 0
    for r in rest:
        if r.ndim == 1:
            out.append(float(score[k]))
            k += 1
        else:
            out.append(score[k:k + len(r)].copy())
            k += len(r)
    return out[0] if kind == "single" else out if kind == "list" else np.asarray(out)


def stoi_curve(clean, mask, history_info, fs=16000, extended=False, device="cuda"):
    """The score after every iteration of a Janssen run, the loop of
    models/AudioReg/train.m:188-213 as one call.

    clean and mask in the layouts of janssen_inpaint (mask True / 1 where
    observed); history_info: the list janssen_inpaint*(..., return_history=True)
    returns (one dict per gap or cluster: signal, start, end, optionally
    missing, history [maxit, h]).  For every signal the maxit restored signals
    (the clean signal outside the gaps, iteration i's values inside) are built
    on the device and scored against the clean row in one call.  Returns one
    [maxit] float64 curve per signal in the layout of the input, NaN from the
    first iteration whose history is NaN (not completed)."""
    import torch
    sigs, _, kind = _normalise(clean, None)
    _, masks, _ = _normalise(clean, mask)
    if not history_info:
        raise ValueError("history_info is empty: nothing to score")
    maxit = {int(np.asarray(d["history"]).shape[0]) for d in history_info
             if d.get("history") is not None}
    if len(maxit) != 1 or any(d.get("history") is None for d in history_info):
        raise ValueError("every entry of history_info needs a history of one maxit "
                         "(return_history=True)")
    maxit = maxit.pop()
    C = len(sigs)
    rows_i, cols_i, vals = [], [], []
    valid = np.full(C, maxit, np.int64)      # iterations completed by every gap of the signal
    for d in history_info:
        c = int(d["signal"])
        if not 0 <= c < C:
            raise ValueError(f"history_info names signal {c}, there are {C}")
        idx = np.asarray(d["missing"], np.int64) if d.get("missing") is not None \
            else np.arange(int(d["start"]), int(d["end"]), dtype=np.int64)
        h = np.asarray(d["history"], np.float64)
        if h.shape != (maxit, idx.size) or idx.size == 0 or idx.min() < 0 \
                or idx.max() >= len(sigs[c]) or masks[c][idx].any():
            raise ValueError(f"signal {c}: a history entry does not match the mask")
        bad = np.isnan(h).any(axis=1)
        if bad.any():
            valid[c] = min(valid[c], int(np.argmax(bad)))
        rows_i.append(np.repeat(c * maxit + np.arange(maxit, dtype=np.int64), idx.size))
        cols_i.append(np.tile(idx, maxit))
        vals.append(np.nan_to_num(h, nan=0.0).reshape(-1))
    _lengths_at_10k([len(s) for s in sigs], fs)
    stride = max(2, _up(max(len(s) for s in sigs), 2))
    host = np.zeros((C, stride), np.float64)
    for c, s in enumerate(sigs):
        host[c, :len(s)] = s
    x = torch.from_numpy(host).to(device)
    y = x.repeat_interleave(maxit, dim=0)
    y.index_put_((torch.from_numpy(np.concatenate(rows_i)).to(device),
                  torch.from_numpy(np.concatenate(cols_i)).to(device)),
                 torch.from_numpy(np.concatenate(vals)).to(device))
    clean_row = [c for c in range(C) for _ in range(maxit)]
    score, _ = _score(torch.cat((x, y)), [len(s) for s in sigs], clean_row, C, fs, extended)
    curves = score.cpu().numpy().reshape(C, maxit)
    for c in range(C):
        curves[c, valid[c]:] = np.nan
    return restack(list(curves), kind)
