"""The mel filterbank of librosa.filters.mel, built on the host.

mel_filterbank follows librosa's defaults (htk=False, norm="slaney",
dtype=float32): the Slaney mel scale (linear below 1 kHz, logarithmic above),
n_mels + 2 points evenly spaced in mel between fmin and fmax, one triangle per
band from the float64 ramps stored into a float32 array, each row scaled by
2 / (f[m+2] - f[m]).  The reference calls it through
librosa.feature.melspectrogram (utils.py:268) and directly (utils.py:367-373).

Every row is non-zero on one run of bins, so the device gets the matrix
compressed to bands (mel_bands: first bin per row, offsets into the packed
weights) -- the layout ainp_mel_fwd reads (include/ainp.h).  mel_pinv is
np.linalg.pinv of the float32 matrix, as the reference computes it
(utils.py:376); 128 x 1025 on the host is not worth a kernel.  Host results
are cached per argument set, device copies per (arguments, device).
"""
from __future__ import annotations

import functools
import warnings
from typing import NamedTuple, Optional

import numpy as np

# Slaney's Auditory Toolbox scale (librosa.hz_to_mel / mel_to_hz, htk=False)
_F_SP = 200.0 / 3
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP          # 15
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    mels = f / _F_SP
    log_t = f >= _MIN_LOG_HZ
    return np.where(log_t, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ)
                    / _LOGSTEP, mels)


def mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    log_t = m >= _MIN_LOG_MEL
    return np.where(log_t, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def _key(sr, n_fft, n_mels, fmin, fmax):
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    return float(sr), int(n_fft), int(n_mels), float(fmin), fmax


@functools.lru_cache(maxsize=None)
def _filterbank(sr: float, n_fft: int, n_mels: int, fmin: float, fmax: float):
    if n_mels < 1 or n_fft < 2:
        raise ValueError("mel_filterbank needs n_mels >= 1 and n_fft >= 2")
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float32)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]      # float64 product, rounded once to float32
    empty = not np.all((mel_f[:-2] == 0) | (weights.max(axis=1) > 0))
    weights.setflags(write=False)
    return weights, empty


def mel_filterbank(sr, n_fft: int, n_mels: int = 128, fmin: float = 0.0,
                   fmax: Optional[float] = None) -> np.ndarray:
    """librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin,
    fmax=fmax): float32 [n_mels, n_fft//2 + 1] (read-only, cached).  A band that
    holds no bin is an all-zero row and draws librosa's warning."""
    weights, empty = _filterbank(*_key(sr, n_fft, n_mels, fmin, fmax))
    if empty:
        warnings.warn("Empty filters detected in mel frequency basis. Some channels will "
                      "produce empty responses. Try increasing your sampling rate (and fmax) "
                      "or reducing n_mels.", stacklevel=2)
    return weights


class MelBands(NamedTuple):
    """Row m of the filterbank is weights[off[m]:off[m+1]] on bins lo[m] ..."""
    lo: np.ndarray        # int32 [n_mels]
    off: np.ndarray       # int32 [n_mels + 1]
    weights: np.ndarray   # float32 [off[-1]] (at least one element)
    n_bins: int

    def dense(self) -> np.ndarray:
        out = np.zeros((len(self.lo), self.n_bins), dtype=np.float32)
        for m, lo in enumerate(self.lo):
            n = self.off[m + 1] - self.off[m]
            out[m, lo:lo + n] = self.weights[self.off[m]:self.off[m + 1]]
        return out


def compress_bands(basis: np.ndarray) -> MelBands:
    """Band tables of a matrix whose rows are each non-zero on one run of bins
    (asserted).  An all-zero row is a band of length 0."""
    n_mels, n_bins = basis.shape
    lo = np.zeros(n_mels, dtype=np.int32)
    off = np.zeros(n_mels + 1, dtype=np.int32)
    runs = []
    for m in range(n_mels):
        nz = np.flatnonzero(basis[m])
        if nz.size:
            first, last = int(nz[0]), int(nz[-1]) + 1
            assert nz.size == last - first, f"mel band {m} is not one run of bins"
            lo[m] = first
            runs.append(basis[m, first:last])
            off[m + 1] = off[m] + (last - first)
        else:
            off[m + 1] = off[m]
    weights = (np.concatenate(runs) if runs else np.zeros(1)).astype(np.float32)
    return check_bands(MelBands(lo, off, weights, n_bins))


def check_bands(b: MelBands) -> MelBands:
    """The host-side table check the C entry point cannot make (its tables live
    on the device): every run inside [0, n_bins) and inside the weights."""
    n = np.diff(b.off.astype(np.int64))
    if (len(b.off) != len(b.lo) + 1 or b.off[0] != 0 or np.any(n < 0) or np.any(b.lo < 0)
            or np.any(b.lo.astype(np.int64) + n > b.n_bins) or b.off[-1] > len(b.weights)):
        raise ValueError("mel band tables run outside the spectrum or the packed weights")
    return b


@functools.lru_cache(maxsize=None)
def _bands(key) -> MelBands:
    return compress_bands(mel_filterbank(*key))


def mel_bands(sr, n_fft, n_mels=128, fmin=0.0, fmax=None) -> MelBands:
    return _bands(_key(sr, n_fft, n_mels, fmin, fmax))


@functools.lru_cache(maxsize=None)
def _pinv(key) -> np.ndarray:
    p = np.ascontiguousarray(np.linalg.pinv(mel_filterbank(*key)), dtype=np.float32)
    p.setflags(write=False)
    return p


def mel_pinv(sr, n_fft, n_mels=128, fmin=0.0, fmax=None) -> np.ndarray:
    """np.linalg.pinv(mel_filterbank(...)): float32 [n_fft//2 + 1, n_mels]."""
    return _pinv(_key(sr, n_fft, n_mels, fmin, fmax))


# device copies, keyed (sr, n_fft, n_mels, fmin, fmax, device) like
# ops._device_window's; ops._release_device_caches drops them at exit
_DEVICE_CACHE: dict = {}


def device_bands(sr, n_fft, n_mels, fmin, fmax, device) -> MelBands:
    """mel_bands(...) with its three tables as tensors on `device`."""
    import torch
    key = ("bands",) + _key(sr, n_fft, n_mels, fmin, fmax) + (str(device),)
    d = _DEVICE_CACHE.get(key)
    if d is None:
        b = mel_bands(sr, n_fft, n_mels, fmin, fmax)
        d = MelBands(*(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                       for a in (b.lo, b.off, b.weights)), b.n_bins)
        _DEVICE_CACHE[key] = d
    return d


def device_pinv(sr, n_fft, n_mels, fmin, fmax, device):
    import torch
    key = ("pinv",) + _key(sr, n_fft, n_mels, fmin, fmax) + (str(device),)
    d = _DEVICE_CACHE.get(key)
    if d is None:
        d = torch.from_numpy(np.array(mel_pinv(sr, n_fft, n_mels, fmin, fmax))).to(device)
        _DEVICE_CACHE[key] = d
    return d
