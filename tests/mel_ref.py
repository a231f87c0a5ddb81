"""float64 numpy reference of the mel layer (test helper, not a test).

Written from the formulas of librosa.filters.mel (htk=False, norm="slaney",
dtype=float32) and librosa.feature.melspectrogram, independently of
ainp/mel.py: scalar mel-scale conversions, a dense matrix filled row by row,
no band compression.  The STFT comes from oracle.stft_ref.
"""
import math

import numpy as np

from oracle import stft_ref

F_SP = 200.0 / 3
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = 15.0
LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f: float) -> float:
    if f >= MIN_LOG_HZ:
        return MIN_LOG_MEL + math.log(f / MIN_LOG_HZ) / LOGSTEP
    return f / F_SP


def mel_to_hz(m: float) -> float:
    if m >= MIN_LOG_MEL:
        return MIN_LOG_HZ * math.exp(LOGSTEP * (m - MIN_LOG_MEL))
    return F_SP * m


def mel_points(n_mels, fmin, fmax):
    lo, hi = hz_to_mel(fmin), hz_to_mel(fmax)
    return [mel_to_hz(m) for m in np.linspace(lo, hi, n_mels + 2)]


def filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None) -> np.ndarray:
    """float32 [n_mels, n_fft//2+1]: triangle max(0, min(rising, falling)) in
    float64, rounded to float32 (librosa fills a float32 array), then times
    2 / (f[m+2] - f[m]) in float64 and rounded to float32 again (its in-place
    multiply of the float32 array by the float64 norms)."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    f = mel_points(n_mels, float(fmin), fmax)
    n_bins = n_fft // 2 + 1
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    out = np.zeros((n_mels, n_bins), dtype=np.float32)
    for m in range(n_mels):
        rising = (freqs - f[m]) / (f[m + 1] - f[m])
        falling = (f[m + 2] - freqs) / (f[m + 2] - f[m + 1])
        tri = np.maximum(0.0, np.minimum(rising, falling)).astype(np.float32)
        out[m] = (tri.astype(np.float64) * (2.0 / (f[m + 2] - f[m]))).astype(np.float32)
    return out


def project(X: np.ndarray, basis: np.ndarray, power: float) -> np.ndarray:
    """basis @ |X|**power in float64; X [..., F, T] complex."""
    mag = np.abs(X.astype(np.complex128))
    S = mag * mag if power == 2.0 else mag ** power
    return np.einsum("mf,...ft->...mt", basis.astype(np.float64), S)


def melspectrogram(y, sr, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None,
                   power=2.0) -> np.ndarray:
    """librosa.feature.melspectrogram(y=y, ...) in float64 (hann, center, zero pad)."""
    X = stft_ref.stft(np.asarray(y), n_fft, hop_length)
    return project(X, filterbank(sr, n_fft, n_mels, fmin, fmax), power)


def mel_to_linear(P: np.ndarray, M: np.ndarray) -> np.ndarray:
    """P [F, n_mels] @ M [..., n_mels, T], the float64 product of the operands
    as given (no square root)."""
    return np.einsum("fk,...kt->...ft", P.astype(np.float64), M.astype(np.float64))
