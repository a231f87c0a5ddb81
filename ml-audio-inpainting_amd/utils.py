"""Drop-in for the reference's utils.py (audio I/O, gap creation, STFT, mel).

Same names, signatures, return types and error behaviour as
/root/reference/utils.py; the STFT runs on the MI355X kernel
(ainp_stft / ainp_stft_features) instead of librosa.

  load_audio            utils.py:14-52   (WAV via the stdlib, FLAC on the native
                                          decoder ainp_flac_decode; other formats
                                          through soundfile when it is installed)
  save_audio            utils.py:54-89   (peak-normalised, WAV; FLAC via soundfile)
  create_gap_mask       utils.py:93-144  (host numpy, the reference's own RNG call)
  add_random_gap        utils.py:146-188 (host numpy, float64 result)
  extract_spectrogram   utils.py:192-234 (GPU, returns the complex STFT; power is
                                          validated then ignored)
  spectrogram_to_audio  utils.py:279-333  (GPU ISTFT / Griffin-Lim)
  extract_mel_spectrogram   utils.py:236-277 (GPU: ainp_stft + ainp_mel_fwd, the
                                          Slaney filterbank of ainp/mel.py)
  mel_spectrogram_to_audio  utils.py:335-393 (GPU: ainp_mel_inverse + Griffin-Lim;
                                          clamp_negative deviates from the
                                          reference's NaN, see its docstring)
  resample_audio, load_audio_batch   (not in the reference's utils.py) the
                                          polyphase resampler ainp_resample_poly:
                                          models/AudioReg/train.m:72's 48 kHz
                                          resample(), and load_audio for a batch
                                          with the resampling on the GPU
Plotting (visualize_spectrogram) is outside the hot path.
"""
from __future__ import annotations

import os
import wave
from pathlib import Path
from typing import Optional, Tuple, Union

import numpy as np

from config import DEFAULT_SAMPLE_RATE

# --- Audio I/O ---------------------------------------------------------------


def _read_wav(path: str) -> Tuple[np.ndarray, int]:
    with wave.open(path, "rb") as w:
        nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        x = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3)
        v = (b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8)
             | (b[:, 2].astype(np.int32) << 16))
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    elif width == 4:
        x = np.frombuffer(raw, "<i4").astype(np.float32) / float(1 << 31)
    else:
        raise ValueError(f"unsupported sample width {width}")
    return x.reshape(-1, nch), sr


def _is_flac(path: str) -> bool:
    try:
        with open(path, "rb") as f:
            head = f.read(4)
    except OSError:
        return False
    return head == b"fLaC" or (head[:3] == b"ID3" and str(path).lower().endswith(".flac"))


def _read_any(path: str) -> Tuple[np.ndarray, int]:
    """(frames, channels) float32 in [-1, 1) and the native rate."""
    if str(path).lower().endswith(".wav"):
        try:
            return _read_wav(str(path))
        except (wave.Error, EOFError):
            pass
    if _is_flac(str(path)):
        from ainp.audio_io import read_flac   # native decoder
        return read_flac(str(path))
    try:
        import soundfile as sf  # optional dependency (not in this image)
    except ImportError as e:
        raise RuntimeError(
            f"cannot decode {path}: only PCM WAV and FLAC are readable without "
            "soundfile") from e
    data, sr = sf.read(str(path), dtype="float32", always_2d=True)
    return data, sr


def load_audio(file_path: Union[str, Path], sample_rate: int = DEFAULT_SAMPLE_RATE,
               max_len: int = 5, mono: bool = True) -> Tuple[np.ndarray, int]:
    """utils.py:14-52: decode, resample to `sample_rate`, mix to mono, truncate
    or zero-pad to int(sample_rate*max_len) samples; IOError on any failure."""
    try:
        data, sr = _read_any(file_path)
        if mono:
            data = data.mean(axis=1)          # librosa.to_mono
        else:
            data = data.T.squeeze()
        if sr != sample_rate:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(sr), int(sample_rate))
            data = resample_poly(data, sample_rate // g, sr // g, axis=-1).astype(np.float32)
        audio_data = data.astype(np.float32)
        sr = sample_rate
        max_samples = int(sample_rate * max_len)
        if len(audio_data) > max_samples:
            audio_data = audio_data[:max_samples]
        else:
            audio_data = np.pad(audio_data, (0, max_samples - len(audio_data)), "constant")
        return audio_data, sr
    except Exception as e:
        raise IOError(f"Error loading audio file {file_path}: {str(e)}")


def resample_audio(audio, orig_sr: int, target_sr: int):
    """scipy.signal.resample_poly(audio, target_sr / g, orig_sr / g) with
    g = gcd(orig_sr, target_sr), along the last axis, on the GPU
    (ainp_resample_poly; MATLAB resample(x, p, q) of models/AudioReg/train.m:72).
    audio [n] or [rows, n], float32 or float64 (anything else is computed in
    float64): a numpy array comes back as a numpy array, a cuda tensor stays on
    the device; the dtype is kept."""
    import torch
    from math import gcd
    from ainp import ops
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if orig_sr < 1 or target_sr < 1:
        raise ValueError("sample rates must be positive")
    g = gcd(orig_sr, target_sr)
    if isinstance(audio, torch.Tensor):
        return ops.resample_poly(audio.contiguous(), target_sr // g, orig_sr // g)
    x = np.asarray(audio)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    y = ops.resample_poly(torch.from_numpy(np.ascontiguousarray(x)).cuda(), target_sr // g,
                          orig_sr // g)
    return y.cpu().numpy()


def load_audio_batch(file_paths, sample_rate: int = DEFAULT_SAMPLE_RATE, max_len=5,
                     mono: bool = True):
    """load_audio for a list of files, resampled on the GPU: every file is
    decoded on the host as load_audio decodes it (mono mean first), the files
    are grouped by native rate, and each group is one ainp_resample_poly launch
    that also truncates or zero-pads to int(sample_rate * max_len) samples.
    Returns a cuda float32 tensor [len(file_paths), int(sample_rate * max_len)]
    in input order; a file that fails to decode raises IOError naming it."""
    import torch
    from math import gcd
    from ainp import ops
    if not mono:
        raise ValueError("load_audio_batch returns one row per file: mono only")
    sample_rate = int(sample_rate)
    max_samples = int(sample_rate * max_len)
    clips, by_rate = [], {}
    for k, path in enumerate(file_paths):
        try:
            data, sr = _read_any(path)
            clips.append(np.ascontiguousarray(data.mean(axis=1), dtype=np.float32))
            by_rate.setdefault(int(sr), []).append(k)
        except Exception as e:
            raise IOError(f"Error loading audio file {path}: {str(e)}")
    out = torch.empty(len(clips), max_samples, device="cuda", dtype=torch.float32)
    for sr, rows in by_rate.items():
        g = gcd(sr, sample_rate)
        n = [len(clips[k]) for k in rows]
        # a multiple of four samples keeps every row 16-byte aligned
        stride = max(4, -(-max(n) // 4) * 4)
        host = np.zeros((len(rows), stride), dtype=np.float32)
        for j, k in enumerate(rows):
            host[j, :n[j]] = clips[k]
        y = ops.resample_poly(torch.from_numpy(host).cuda(), sample_rate // g, sr // g, n=n,
                              out_len=max_samples)
        out[torch.as_tensor(rows, device="cuda")] = y
    return out


def save_audio(audio_data: np.ndarray, file_path: Union[str, Path],
               sample_rate: int = DEFAULT_SAMPLE_RATE, normalize: bool = True,
               file_format: str = "flac") -> None:
    """utils.py:54-89: create parent dirs, peak-normalise
    (librosa.util.normalize: x / max|x|), write 16-bit PCM."""
    output_dir = Path(file_path).parent
    if output_dir and not output_dir.exists():
        try:
            output_dir.mkdir(parents=True, exist_ok=True)
        except Exception as e:
            raise IOError(f"Error creating directory {output_dir}: {str(e)}")
    audio_data = np.asarray(audio_data)
    if normalize:
        peak = np.max(np.abs(audio_data)) if audio_data.size else 0.0
        if peak > np.finfo(np.float32).tiny:
            audio_data = audio_data / peak
    try:
        if file_format.lower() == "wav" or str(file_path).lower().endswith(".wav"):
            pcm = np.clip(np.round(audio_data * 32767.0), -32768, 32767).astype("<i2")
            with wave.open(str(file_path), "wb") as w:
                w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
                w.setsampwidth(2)
                w.setframerate(int(sample_rate))
                w.writeframes(pcm.tobytes())
        elif file_format.lower() == "flac":
            # soundfile's FLAC / PCM_16 write on the native encoder (csrc/flac.cpp)
            from ainp.audio_io import write_flac
            write_flac(str(file_path), audio_data, int(sample_rate))
        else:
            import soundfile as sf
            sf.write(file_path, audio_data, sample_rate, format=file_format)
    except Exception as e:
        raise IOError(f"Error saving audio to {file_path}: {str(e)}")


# --- Gap Processing ----------------------------------------------------------


def create_gap_mask(audio_len_samples: int, gap_len_s: float,
                    sample_rate: int = DEFAULT_SAMPLE_RATE,
                    gap_start_s: Optional[float] = None) -> Tuple[np.ndarray, Tuple[int, int]]:
    """utils.py:93-144: 1 = signal, 0 = gap; random start in [0, S-g] inclusive."""
    gap_len_samples = int(gap_len_s * sample_rate)
    if gap_len_samples <= 0:
        return np.ones(audio_len_samples, dtype=np.float32), (0, 0)
    if gap_len_samples >= audio_len_samples:
        print(f"Warning: Gap length ({gap_len_s}s) >= audio length. Returning all zeros mask.")
        return np.zeros(audio_len_samples, dtype=np.float32), (0, audio_len_samples)
    max_start_sample = audio_len_samples - gap_len_samples
    if gap_start_s is None:
        gap_start_sample = np.random.randint(0, max_start_sample + 1)
    else:
        gap_start_sample = int(gap_start_s * sample_rate)
    gap_end_sample = gap_start_sample + gap_len_samples
    mask = np.ones(audio_len_samples, dtype=np.float32)
    mask[gap_start_sample:gap_end_sample] = 0.0
    return mask, (gap_start_sample, gap_end_sample)


def draw_gap_start(audio_len: int, gap_length: int) -> int:
    """The RNG draw of utils.py:179 (exclusive of audio_len - gap_length)."""
    return int(np.random.randint(0, audio_len - gap_length))


def insert_gap(audio_data: np.ndarray, gap_start_idx: int, gap_length: int) -> np.ndarray:
    """Zero [start, start+gap) by concatenation with float64 zeros (utils.py:180-183)."""
    silence = np.zeros(gap_length)
    return np.concatenate([audio_data[:gap_start_idx], silence,
                           audio_data[gap_start_idx + gap_length:]])


def add_random_gap(file_path: Union[str, Path], gap_len: float,
                   sample_rate: int = DEFAULT_SAMPLE_RATE,
                   mono: bool = True) -> Tuple[np.ndarray, Tuple[float, float]]:
    """utils.py:146-188: reload, random start in [0, S-g) (exclusive), float64
    result; ValueError when the gap is not shorter than the audio."""
    audio_data, sr = load_audio(file_path, sample_rate=sample_rate, mono=mono)
    gap_length = int(gap_len * sample_rate)
    audio_len = len(audio_data)
    if gap_length >= audio_len:
        raise ValueError(f"Gap length ({gap_length}s) exceeds audio length ({audio_len/sample_rate}s)")
    gap_start_idx = draw_gap_start(audio_len, gap_length)
    audio_new = insert_gap(audio_data, gap_start_idx, gap_length)
    return audio_new, (gap_start_idx / sample_rate, (gap_start_idx + gap_length) / sample_rate)


# --- STFT Processing -----------------------------------------------------------


def extract_spectrogram(audio_data, n_fft: int = 2048, hop_length: int = 512,
                        win_length: Optional[int] = None, window: str = "hann",
                        center: bool = True, power: float = 1.0):
    """utils.py:192-234: the complex STFT (librosa>=0.10 semantics) computed by
    ainp_stft on the GPU.  float32 input -> complex64, float64 -> complex128
    (as librosa).  numpy in -> numpy out; a torch cuda tensor stays on the GPU.
    `power` is validated and otherwise ignored, as in the reference (Q4)."""
    if power < 0:
        raise ValueError("Power must be non-negative")
    if win_length is None:
        win_length = n_fft
    import torch
    from ainp import ops
    if isinstance(audio_data, torch.Tensor):
        return ops.stft(audio_data, n_fft, hop_length, win_length, window, center)
    a = np.asarray(audio_data)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float32 if a.dtype.itemsize <= 4 else np.float64)
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.stft(t, n_fft, hop_length, win_length, window, center).cpu().numpy()


def db_to_amplitude(S_db, ref: float = 1.0):
    """librosa.db_to_amplitude: ref * 10**(0.05 * S_db) (host numpy, as the reference)."""
    return ref * np.power(10.0, 0.05 * np.asarray(S_db))


def spectrogram_to_audio(spectrogram, phase=None, phase_info: bool = False, n_fft=512,
                         n_iter=64, window="hann", hop_length=512, win_length=None,
                         center=True, random_state=None):
    """utils.py:279-333 on the GPU kernels (ainp_istft / ainp_stft / ainp_gl_update):
    a dB-scaled input (max < 0 and mean < 0) is converted back to amplitude;
    phase_info: the input is a complex spectrogram -> istft; phase given ->
    istft(S * exp(i phase)); otherwise Griffin-Lim (n_iter, momentum 0.99,
    random initial phases; random_state seeds them as in librosa).
    numpy in -> numpy out (as the reference); torch cuda tensors stay on the GPU."""
    import torch
    from ainp import ops
    as_numpy = not isinstance(spectrogram, torch.Tensor)
    S = spectrogram
    if as_numpy:
        S = np.asarray(S)
        if not np.iscomplexobj(S) and np.max(S) < 0 and np.mean(S) < 0:
            S = db_to_amplitude(S)
        S = torch.from_numpy(np.ascontiguousarray(S)).cuda()
    elif not S.is_complex() and bool((S.max() < 0) & (S.mean() < 0)):
        S = torch.from_numpy(db_to_amplitude(S.cpu().numpy())).to(S.device)
    kw = dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window,
              center=center)
    if phase_info:
        if not S.is_complex():
            S = S.to(torch.complex64)
        y = ops.istft(S.contiguous(), **kw)
    elif phase is not None:
        ph = torch.as_tensor(np.asarray(phase) if as_numpy else phase).to(S.device, torch.float32)
        y = ops.istft(mag=S.to(torch.float32).contiguous(), phase=ph.contiguous(), **kw)
    else:
        y = ops.griffinlim(S.to(torch.float32).contiguous(), n_iter=n_iter,
                           hop_length=hop_length, win_length=win_length, n_fft=n_fft,
                           window=window, center=center, random_state=random_state)
    return y.cpu().numpy() if as_numpy else y


def inpaint_phase(audio, mask, magnitude, n_fft=512, hop_length=None, win_length=None,
                  n_iter=64, momentum=0.99, return_resid=False):
    """Blind counterpart of spectrogram_to_audio(..., phase=original_phase) for
    a gapped signal (not in the reference): fill the samples where `mask` is 0
    so that the frames around them have the linear magnitudes `magnitude`
    [n_fft/2+1, 1 + len // hop_length], by the gap-constrained Griffin-Lim of
    ainp_gap_phase (ainp.gap_phase.gap_phase_fill; float64, deterministic, no
    phase of the clean signal needed).  The observed samples come back
    bit-identical; the values `audio` holds inside the gaps are the start.
    hop_length defaults to win_length // 4.  [S] or [B, S]; numpy in -> numpy
    out, a torch cuda tensor stays on the GPU."""
    import torch
    from ainp.gap_phase import gap_phase_fill
    win_length = n_fft if win_length is None else win_length
    hop_length = win_length // 4 if hop_length is None else hop_length
    as_numpy = not isinstance(audio, torch.Tensor)
    a = audio
    if as_numpy:
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float32 if a.dtype.itemsize <= 4 else np.float64)
        a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    m = torch.as_tensor(np.asarray(mask) if not isinstance(mask, torch.Tensor) else mask)
    A = torch.as_tensor(np.asarray(magnitude) if not isinstance(magnitude, torch.Tensor)
                        else magnitude).to(a.device, torch.float32)
    res = gap_phase_fill(a, m.to(a.device), A, n_fft, hop_length, win_length, n_iter=n_iter,
                         momentum=momentum, return_resid=return_resid)
    if not as_numpy:
        return res
    if return_resid:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy()


def extract_mel_spectrogram(audio_data, sample_rate: int = DEFAULT_SAMPLE_RATE,
                            n_fft: int = 2048, hop_length: int = 512, n_mels: int = 128,
                            fmin: float = 0.0, fmax: Optional[float] = None,
                            power: float = 2.0):
    """utils.py:236-277 -> librosa.feature.melspectrogram on the GPU: the STFT
    (win_length = n_fft, hann, center=True, zero padding) by ainp_stft, then
    mel_basis @ |X|**power by ainp_mel_fwd with the Slaney filterbank of
    librosa.filters.mel (ainp/mel.py); the power spectrogram is never stored.
    float32 in -> float32 out, float64 -> float64 (as librosa).  numpy in ->
    numpy out; a torch cuda tensor stays on the GPU."""
    if power < 0:
        raise ValueError("Power must be non-negative")
    import torch
    from ainp import ops
    kw = dict(sr=sample_rate, n_fft=n_fft, hop_length=hop_length, n_mels=n_mels, fmin=fmin,
              fmax=fmax, power=power)
    if isinstance(audio_data, torch.Tensor):
        return ops.mel_spectrogram(audio_data, **kw)
    a = np.asarray(audio_data)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float32 if a.dtype.itemsize <= 4 else np.float64)
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.mel_spectrogram(t, **kw).cpu().numpy()


def mel_spectrogram_to_audio(mel_spectrogram, sample_rate: int = DEFAULT_SAMPLE_RATE,
                             n_fft: int = 2048, hop_length: int = 512, n_iter: int = 32,
                             n_mels: int = 128, fmin: float = 0.0,
                             fmax: Optional[float] = None, power: float = 2.0, *,
                             clamp_negative: bool = True, random_state=None):
    """utils.py:335-393 on the GPU: linear = pinv(mel_basis) @ mel (pinv on the
    host, as the reference; the product by ainp_mel_inverse), its square root
    when power == 2.0 exactly, then Griffin-Lim (n_iter, librosa's defaults:
    win_length = n_fft, hann, center, momentum 0.99, random initial phases;
    random_state seeds them as in librosa).  Returns hop_length * (T - 1)
    samples, float32.  numpy in -> numpy out; a torch cuda tensor stays on the GPU.

    Deviation (clamp_negative, keyword-only, not in the reference): the
    pseudo-inverse product is slightly negative in a few bins (measured: 0.3 % of
    the entries and 97 % of the frames at 16 kHz / n_fft 2048 / 128 mels; 3 % and
    100 % at n_fft 128 / 20 mels), the reference's np.sqrt turns those into NaN
    and the overlap-add spreads them over the whole signal, which its own tests
    (len > 0, not allclose(0)) do not notice.  clamp_negative=True (default)
    zeroes negative values before the sqrt; clamp_negative=False reproduces the
    reference's NaN.  With power != 2.0 no sqrt is taken and the negative
    magnitudes go to Griffin-Lim as they are, as in the reference."""
    import torch
    from ainp import ops
    as_numpy = not isinstance(mel_spectrogram, torch.Tensor)
    M = mel_spectrogram
    if as_numpy:
        M = torch.from_numpy(np.ascontiguousarray(np.asarray(M))).cuda()
    M = M.to(torch.float32).contiguous()
    linear = ops.mel_to_linear(M, sr=sample_rate, n_fft=n_fft, n_mels=n_mels, fmin=fmin,
                               fmax=fmax, power=power, clamp_negative=clamp_negative)
    y = ops.griffinlim(linear, n_iter=n_iter, hop_length=hop_length, n_fft=n_fft,
                       random_state=random_state)
    return y.cpu().numpy() if as_numpy else y


def visualize_spectrogram(*args, **kwargs):
    raise NotImplementedError("plotting is outside the hot path (DESIGN.md §1)")
