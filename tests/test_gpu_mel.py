"""GPU parity of the mel kernels (csrc/mel.hip) and the utils drop-ins built on
them, against the float64 reference of tests/mel_ref.py.

Bounds (u = 2**-24, float32 unit round-off):
  mel_fwd      every term w * |X|^p is non-negative, so the standard fma-chain
               bound is relative to the result itself: |d| <= (maxband + 3) u ref
               (maxband terms summed, 3 u for forming |X|^p); float64: 1e-12 ref.
  mel_inverse  the dot-product bound |d| <= (n_mels + 2) u (|P| |M|).
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import mel_ref
from ainp import mel, ops, synth

pytestmark = pytest.mark.gpu

SR = 16000
U = 2.0 ** -24
# name: (n_fft, n_mels, hop, batch, T, fmin, fmax)
SHAPES = {
    "tile_plus_tail": (64, 8, 16, 3, 70, 0.0, None),
    "empty_bands_one_frame": (64, 40, 16, 1, 1, 0.0, None),
    "bins_outside_bands": (128, 20, 32, 1, 65, 300.0, 3400.0),
    "default": (2048, 128, 512, 1, 32, 0.0, None),
}


def _cfg(name):
    n_fft, n_mels, hop, batch, T, fmin, fmax = SHAPES[name]
    return (SR, n_fft, n_mels, fmin, fmax)


@functools.lru_cache(maxsize=None)
def _basis(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")        # the empty-band warning of one shape
        return mel.mel_filterbank(*_cfg(name)), mel.mel_bands(*_cfg(name))


def _bands_dev(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mel.device_bands(*_cfg(name), "cuda")


@functools.lru_cache(maxsize=None)
def _spectrum(name, dtype):
    """The device's own STFT of `batch` synthetic clips, copied back:
    complex [batch, F, T] (computed once per shape and precision)."""
    n_fft, n_mels, hop, batch, T, fmin, fmax = SHAPES[name]
    n = hop * (T - 1) + hop // 2
    y = np.stack([synth.synthetic_clip(11 + b, n, SR) for b in range(batch)]).astype(dtype)
    X = ops.stft(torch.from_numpy(y).cuda(), n_fft, hop).cpu().numpy()
    assert X.shape == (batch, n_fft // 2 + 1, T)
    return X


@functools.lru_cache(maxsize=None)
def _mel_power(name):
    """M = basis @ |X|^2 as float32 [batch, n_mels, T] (host), the mel_inverse input."""
    M = mel_ref.project(_spectrum(name, np.float32), _basis(name)[0], 2.0).astype(np.float32)
    return M


# ------------------------------------------------------------------ mel_fwd
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("power", [1.0, 2.0, 1.5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_mel_fwd_matches_float64(name, power, dtype):
    basis, bands = _basis(name)
    X = _spectrum(name, dtype)
    out = ops.mel_fwd(torch.from_numpy(X).cuda(), _bands_dev(name), power)
    assert out.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
    got = out.cpu().numpy()
    ref = mel_ref.project(X, basis, power)
    assert got.shape == ref.shape == (X.shape[0], SHAPES[name][1], X.shape[2])
    maxband = int(np.diff(bands.off).max())
    rel = (maxband + 3) * U if dtype == np.float32 else 1e-12
    d = np.abs(got.astype(np.float64) - ref)
    live = ref > 0
    print(f"{name} p={power} {np.dtype(dtype).name}: max |d|/ref = "
          f"{(d[live] / ref[live]).max():.3e}, bound {rel:.3e}")
    assert np.all(d <= rel * ref)
    empty = basis.max(axis=1) == 0
    assert np.all(got[:, empty, :] == 0)          # rows of empty bands: exactly 0
    if name == "empty_bands_one_frame":
        assert empty.sum() == 7


# ------------------------------------------------------------- end to end
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_extract_mel_spectrogram_end_to_end(dtype):
    import utils
    y = synth.synthetic_clip(3, SR, SR).astype(dtype)
    got = utils.extract_mel_spectrogram(y, SR)
    assert isinstance(got, np.ndarray) and got.dtype == dtype
    ref = mel_ref.melspectrogram(y, SR)
    assert got.shape == ref.shape == (128, 32)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"extract_mel_spectrogram {np.dtype(dtype).name}: max err / max = {err:.3e}")
    assert err <= 1e-4
    # a cuda tensor stays on the GPU, same values
    t = utils.extract_mel_spectrogram(torch.from_numpy(y).cuda(), SR)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert np.array_equal(t.cpu().numpy(), got)


def test_power_two_is_power_one_of_the_squared_magnitude():
    """mel(power=2) == mel(power=1) of |X|^2 (what the reference's
    test_extract_mel_spectrogram_power_values means to check).  The two differ
    by the rounding of |X|^2 per term (2 u) and of two different fma chains
    (maxband u each): (2 maxband + 4) u relative, all terms being non-negative."""
    name = "default"
    X = _spectrum(name, np.float32)
    Xd = torch.from_numpy(X).cuda()
    kw = dict(sr=SR, n_fft=2048, n_mels=128)
    p2 = ops.mel_spectrogram(S=Xd, power=2.0, **kw).cpu().numpy()
    sq = (X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2).astype(np.float32)
    p1 = ops.mel_spectrogram(S=torch.from_numpy(sq.astype(np.complex64)).cuda(), power=1.0,
                             **kw).cpu().numpy()
    maxband = int(np.diff(_basis(name)[1].off).max())
    d = np.abs(p2.astype(np.float64) - p1)
    assert np.all(d <= (2 * maxband + 4) * U * p2)
    # and the mel of the audio is the mel of its STFT
    y = torch.from_numpy(synth.synthetic_clip(5, SR, SR)).cuda()
    a = ops.mel_spectrogram(y, sr=SR)
    b = ops.mel_spectrogram(S=ops.stft(y), sr=SR)
    assert torch.equal(a, b)


# -------------------------------------------------------------- mel_inverse
@pytest.mark.parametrize("name", list(SHAPES))
def test_mel_inverse_matches_float64_and_epilogues(name):
    n_mels = SHAPES[name][1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = mel.mel_pinv(*_cfg(name))
        Pd = mel.device_pinv(*_cfg(name), "cuda")
    M = _mel_power(name)
    Md = torch.from_numpy(M).cuda()
    raw = ops.mel_inverse(Pd, Md, 0).cpu().numpy()
    ref = mel_ref.mel_to_linear(P, M)
    assert raw.shape == ref.shape == (M.shape[0], P.shape[0], M.shape[2])
    scale = mel_ref.mel_to_linear(np.abs(P), np.abs(M))
    d = np.abs(raw.astype(np.float64) - ref)
    print(f"{name}: max |d| / (|P||M|) = {(d[scale > 0] / scale[scale > 0]).max():.3e}, "
          f"bound {(n_mels + 2) * U:.3e}")
    assert np.all(d <= (n_mels + 2) * U * scale)

    neg = raw < 0
    print(f"{name}: {neg.mean():.2%} of the pseudo-inverse product is negative")
    if name != "empty_bands_one_frame":     # 33 bins from 33 live bands: an exact inverse
        assert neg.any()
    with np.errstate(invalid="ignore"):
        want = np.sqrt(raw)
    # sqrt: NaN exactly where the product is negative, sqrt of the same bits elsewhere
    s = ops.mel_inverse(Pd, Md, ops.MEL_SQRT).cpu().numpy()
    assert np.array_equal(np.isnan(s), neg)
    assert np.all(np.abs(s[~neg] - want[~neg]) <= 2 * np.spacing(want[~neg]))
    # sqrt of max(x, 0): zeros there instead, everything finite
    c = ops.mel_inverse(Pd, Md, ops.MEL_SQRT | ops.MEL_CLAMP).cpu().numpy()
    assert np.all(np.isfinite(c)) and np.all(c[neg] == 0)
    assert np.array_equal(c[~neg], s[~neg])
    # the clamp alone shows the pre-epilogue bits are the same under every epilogue
    m = ops.mel_inverse(Pd, Md, ops.MEL_CLAMP).cpu().numpy()
    assert np.array_equal(m[~neg], raw[~neg]) and np.all(m[neg] == 0)


def test_mel_to_linear_flags_follow_power():
    name = "bins_outside_bands"
    sr, n_fft, n_mels, fmin, fmax = _cfg(name)
    Md = torch.from_numpy(_mel_power(name)).cuda()
    kw = dict(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax)
    raw = ops.mel_to_linear(Md, power=1.0, **kw)
    assert bool((raw < 0).any())                  # power != 2: the bare product, untouched
    assert torch.equal(raw, ops.mel_to_linear(Md, power=1.0, clamp_negative=False, **kw))
    assert bool(torch.isnan(ops.mel_to_linear(Md, power=2.0, clamp_negative=False, **kw)).any())
    assert bool(torch.isfinite(ops.mel_to_linear(Md, power=2.0, **kw)).all())


# --------------------------------------------------------------- round trip
def test_mel_round_trip():
    """After the reference's test_full_reconstruction_mel_spectrogram."""
    import utils
    kw = dict(n_fft=512, hop_length=128, n_mels=40)
    y = synth.synthetic_clip(7, SR, SR)
    M = utils.extract_mel_spectrogram(y, SR, **kw)
    T = M.shape[1]
    audio = utils.mel_spectrogram_to_audio(M, SR, n_iter=8, random_state=0, **kw)
    assert isinstance(audio, np.ndarray) and audio.shape == (128 * (T - 1),)
    assert np.all(np.isfinite(audio))
    M2 = utils.extract_mel_spectrogram(audio, SR, **kw)
    n = min(T, M2.shape[1])
    corr = np.corrcoef(M[:, :n].ravel(), M2[:, :n].ravel())[0, 1]
    print(f"round trip: mel correlation {corr:.4f}")
    assert corr > 0
    # the reference's behaviour, kept as a documented quirk: NaN audio
    bad = utils.mel_spectrogram_to_audio(M, SR, n_iter=8, random_state=0,
                                         clamp_negative=False, **kw)
    assert bad.shape == audio.shape and np.isnan(bad).any()


# -------------------------------------------------------------- determinism
def test_results_are_bit_identical_from_call_to_call():
    name = "tile_plus_tail"
    Xd = torch.from_numpy(_spectrum(name, np.float32)).cuda()
    bands = _bands_dev(name)
    for power in (2.0, 1.5):
        assert torch.equal(ops.mel_fwd(Xd, bands, power), ops.mel_fwd(Xd, bands, power))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Pd = mel.device_pinv(*_cfg(name), "cuda")
    Md = torch.from_numpy(_mel_power(name)).cuda()
    for flags in (0, ops.MEL_SQRT | ops.MEL_CLAMP):
        assert torch.equal(ops.mel_inverse(Pd, Md, flags), ops.mel_inverse(Pd, Md, flags))
