"""CPU-only checks of the mel layer: the host filterbank (ainp/mel.py) against
the independent float64 reference (tests/mel_ref.py) and known answers, the
band tables the device reads, and argument validation of ainp_mel_fwd /
ainp_mel_inverse before any launch."""
import warnings

import numpy as np
import pytest

import mel_ref
from ainp import mel

# (sr, n_fft, n_mels, fmin, fmax)
CONFIGS = [
    (16000, 2048, 128, 0.0, None),
    (16000, 512, 40, 0.0, None),
    (16000, 128, 20, 300.0, 3400.0),   # 40 bins outside every band
    (16000, 64, 40, 0.0, None),        # 7 empty bands
    (22050, 2048, 128, 0.0, None),
]


def _basis(cfg):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mel.mel_filterbank(*cfg)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_filterbank_matches_reference_to_one_ulp(cfg):
    got = _basis(cfg)
    ref = mel_ref.filterbank(*cfg)
    assert got.dtype == np.float32 and got.shape == (cfg[2], cfg[1] // 2 + 1)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref)))
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp)
    assert np.array_equal(got == 0, ref == 0)


def test_filterbank_known_answers():
    # librosa's documentation prints 0.016 for this entry of filters.mel(sr=22050, n_fft=2048)
    b = _basis((22050, 2048, 128, 0.0, None))
    assert b[0, 0] == 0.0
    np.testing.assert_allclose(b[0, 1], 0.016182853, rtol=1e-6)
    b = _basis((16000, 512, 40, 0.0, None))
    # (numpy's default print of these is [0.0005696 0.00047467 0.00037974 0.0002848])
    np.testing.assert_allclose(b[39, 250:254],
                               [0.0005696034, 0.00047466953, 0.0003797356, 0.0002848017],
                               rtol=1e-6)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_band_structure(cfg):
    b = _basis(cfg)
    for m, row in enumerate(b):
        nz = np.flatnonzero(row)
        if nz.size:
            assert nz[-1] - nz[0] + 1 == nz.size, f"row {m} support is not contiguous"
    assert (b != 0).sum(axis=0).max() <= 2        # a bin feeds at most two bands
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bands = mel.mel_bands(*cfg)
    assert bands.lo.dtype == np.int32 and bands.off.dtype == np.int32
    assert bands.weights.dtype == np.float32 and bands.n_bins == b.shape[1]
    assert len(bands.lo) == cfg[2] and len(bands.off) == cfg[2] + 1
    assert np.array_equal(bands.dense(), b)       # the device tables are the matrix, exactly
    assert np.all(bands.lo + np.diff(bands.off) <= bands.n_bins)


def test_empty_bands_and_uncovered_bins():
    with pytest.warns(UserWarning, match="Empty filters"):
        b = mel.mel_filterbank(16000, 64, 40)
    assert int((b.max(axis=1) == 0).sum()) == 7
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bands = mel.mel_bands(16000, 64, 40)
    assert int((np.diff(bands.off) == 0).sum()) == 7
    b = _basis((16000, 128, 20, 300.0, 3400.0))
    assert int(((b != 0).sum(axis=0) == 0).sum()) == 40


def test_slaney_rows_have_unit_area():
    b = _basis((16000, 2048, 128, 0.0, None))
    area = b.astype(np.float64).sum(axis=1) * 16000 / 2048
    assert area.min() >= 0.98 and area.max() <= 1.02


def test_compress_bands_rejects_a_split_row():
    bad = np.zeros((2, 8), dtype=np.float32)
    bad[0, [1, 2, 4]] = 1.0
    with pytest.raises(AssertionError, match="not one run"):
        mel.compress_bands(bad)
    lo = np.array([6], dtype=np.int32)
    off = np.array([0, 4], dtype=np.int32)
    with pytest.raises(ValueError, match="outside"):
        mel.check_bands(mel.MelBands(lo, off, np.ones(4, np.float32), 8))


def test_pinv_is_the_float32_pseudo_inverse():
    cfg = (16000, 128, 20, 300.0, 3400.0)
    P = mel.mel_pinv(*cfg)
    assert P.dtype == np.float32 and P.shape == (65, 20)
    np.testing.assert_array_equal(P, np.linalg.pinv(_basis(cfg)))


def test_bad_arguments_fail_without_launching():
    """Argument validation happens before any HIP call (no GPU needed)."""
    from ainp import _lib
    L = _lib.lib
    p = 16                      # a non-null pointer that is never dereferenced

    def fwd(spec=p, dtype=0, n_sig=1, n_bins=65, T=4, lo=p, off=p, w=p, nw=10, n_mels=8,
            power=2.0, out=p):
        return L.ainp_mel_fwd(spec, dtype, n_sig, n_bins, T, lo, off, w, nw, n_mels, power, out,
                              None)

    bad_fwd = [dict(spec=None), dict(lo=None), dict(off=None), dict(w=None), dict(out=None),
               dict(n_mels=0), dict(n_bins=1), dict(T=0), dict(n_sig=-1), dict(power=-1.0),
               dict(power=float("nan")), dict(power=float("inf")), dict(dtype=2), dict(nw=-1)]
    for kw in bad_fwd:
        assert fwd(**kw) == -1, kw
        assert b"ainp_mel_fwd" in L.ainp_last_error(), kw

    def inv(pinv=p, mel_=p, n_sig=1, n_bins=65, n_mels=8, T=4, flags=0, out=p):
        return L.ainp_mel_inverse(pinv, mel_, n_sig, n_bins, n_mels, T, flags, out, None)

    bad_inv = [dict(pinv=None), dict(mel_=None), dict(out=None), dict(n_mels=0), dict(n_bins=1),
               dict(T=0), dict(n_sig=-1), dict(flags=4), dict(flags=-1)]
    for kw in bad_inv:
        assert inv(**kw) == -1, kw
        assert b"ainp_mel_inverse" in L.ainp_last_error(), kw


def test_negative_power_raises_before_touching_the_gpu():
    import utils
    with pytest.raises(ValueError, match="Power must be non-negative"):
        utils.extract_mel_spectrogram(np.zeros(1024, np.float32), 16000, power=-1.0)
