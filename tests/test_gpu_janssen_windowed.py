"""GPU tests of the window-wise Janssen rows (csrc/janssen_windows.hip around
ainp_janssen_ex, through ainp.janssen.janssen_windowed and
models/model_eval.run_ar_evaluation) against the dense float64 restatement of
segmentation_inp.m in tests/janssen_windowed_ref.py.

Bound of the parity cases: 1e-9 * max|clean gap|, the project's bound for small
shapes.  At these shapes two independent float64 CPU solvers differ by at most
1.8e-10 and float32 input moves the result by at least 2.2e-8
(test_cpu_janssen_windowed.py measures both).  Bundled clip: 1e-8 * max|gap|,
as the other end-to-end tests.  Every test prints its measured figure; DESIGN
§14 records them.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import janssen_ref as R
import janssen_windowed_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")

# lpc on every case and shape, Burg on the first two cases
PARITY = [(c, t, "lpc") for c in W.CASES for t in W.WTYPES] + \
         [(c, t, "arburg") for c in W.CASES[:2] for t in W.WTYPES]


def _gapped(case):
    w, a, s0, e0, p, maxit, n = case
    mask = np.ones(n, bool)
    mask[s0:e0] = False
    return W.case_signal(case), mask


@pytest.mark.parametrize("case,wtype,method", PARITY,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{t}-{m}" for c, t, m in PARITY])
def test_parity(case, wtype, method):
    from ainp.janssen import janssen_windowed
    w, a, s0, e0, p, maxit, n = case
    x, mask = _gapped(case)
    out, info = janssen_windowed(x, mask, p=p, w=w, a=a, wtype=wtype, maxit=maxit,
                                 method=method, return_history=True)
    ref = W.case_reference(case, wtype, method)               # [maxit, h]
    scale = np.max(np.abs(x[s0:e0]))
    assert len(info) == 1 and (info[0]["signal"], info[0]["start"], info[0]["end"]) == (0, s0, e0)
    assert info[0]["iters"] and all(i == maxit for i in info[0]["iters"])
    hist = info[0]["history"]
    assert hist.shape == ref.shape
    d_hist = np.max(np.abs(hist - ref)) / scale
    d = np.max(np.abs(out[s0:e0] - ref[-1])) / scale
    print(f"windowed {wtype} {method} {case[:4]}: final {d:.3e}, history {d_hist:.3e}")
    assert d <= 1e-9 and d_hist <= 1e-9
    assert np.array_equal(out[s0:e0], hist[-1])
    assert out.dtype == np.float64 and np.array_equal(out[mask], x[mask])


def test_repeats_and_history_columns():
    """Two calls give the same bits; column k of the history is a fresh run
    with maxit = k + 1."""
    from ainp.janssen import janssen_windowed
    case = W.CASES[4]                                         # all-missing windows included
    w, a, s0, e0, p, maxit, n = case
    x, mask = _gapped(case)
    for wtype in W.WTYPES:
        out, info = janssen_windowed(x, mask, p=p, w=w, a=a, wtype=wtype, maxit=maxit,
                                     return_history=True)
        again, info2 = janssen_windowed(x, mask, p=p, w=w, a=a, wtype=wtype.upper(),
                                        maxit=maxit, return_history=True)
        assert np.array_equal(out, again)
        assert np.array_equal(info[0]["history"], info2[0]["history"])
        assert np.array_equal(janssen_windowed(x, mask, p=p, w=w, a=a, wtype=wtype, maxit=maxit),
                              out)
        for k in range(maxit):
            fresh = janssen_windowed(x, mask, p=p, w=w, a=a, wtype=wtype, maxit=k + 1)
            assert np.array_equal(fresh[s0:e0], info[0]["history"][k]), (wtype, k)


def test_batch_of_signals_gaps_and_shapes_is_the_separate_calls():
    from ainp.janssen import janssen_windowed
    p, w, a, maxit = 16, 128, 32, 3
    sigs = [R.sinusoid_mix(n, noise=1e-3, seed=i) for i, n in enumerate((1500, 1201, 1800))]
    gaps = [((300, 340), (1000, 1001)), ((531, 555), (900, 1000)), ((40, 70), (1700, 1760))]
    masks = []
    for x, gs in zip(sigs, gaps):
        m = np.ones(len(x), bool)
        for s0, e0 in gs:
            m[s0:e0] = False
        masks.append(m)
    both = janssen_windowed(sigs, masks, p=p, w=w, a=a, wtype=("hann", "RECT", "tukey"),
                            maxit=maxit, return_history=True)
    assert sorted(both) == ["hann", "rect", "tukey"]
    for wtype in W.WTYPES:
        outs, info = both[wtype]
        assert [(g["signal"], g["start"], g["end"]) for g in info] == [
            (i, s0, e0) for i, gs in enumerate(gaps) for s0, e0 in gs]
        for i, (x, m) in enumerate(zip(sigs, masks)):
            alone, hist = janssen_windowed(x, m, p=p, w=w, a=a, wtype=wtype, maxit=maxit,
                                           return_history=True)
            assert np.array_equal(outs[i], alone), (wtype, i)
            assert np.array_equal(outs[i][m], x[m])
            mine = [g for g in info if g["signal"] == i]
            for g, h in zip(mine, hist):
                assert g["iters"] == h["iters"]
                assert np.array_equal(g["history"], h["history"])
    # without the history, and as a 2-D batch with NaN marking the gaps: the same bits
    plain = janssen_windowed(sigs, masks, p=p, w=w, a=a, wtype=("hann", "rect", "tukey"),
                             maxit=maxit)
    for wtype in W.WTYPES:
        for i in range(3):
            assert np.array_equal(plain[wtype][i], both[wtype][0][i])
    marked = np.stack([sigs[0], sigs[0][::-1]]).copy()
    marked[:, 300:340] = np.nan
    out = janssen_windowed(torch.from_numpy(marked), p=p, w=w, a=a, maxit=maxit)
    assert out.shape == marked.shape and np.all(np.isfinite(out))
    m0 = np.ones(1500, bool)
    m0[300:340] = False
    assert np.array_equal(out[0], janssen_windowed(sigs[0], m0, p=p, w=w, a=a, maxit=maxit))


def test_silent_context_gives_a_zero_gap():
    from ainp.janssen import janssen_windowed
    x = np.zeros(2000)
    x[1500:] = R.sinusoid_mix(500)                            # beyond every window of the gap
    mask = np.ones(2000, bool)
    mask[900:980] = False
    x[900:980] = 7.0                                          # whatever the gap holds is ignored
    out, info = janssen_windowed(x, mask, p=32, w=256, a=64, maxit=4, return_history=True)
    assert np.all(out[900:980] == 0.0) and np.array_equal(out[mask], x[mask])
    assert info[0]["iters"] == [0] * 6
    assert np.all(np.isnan(info[0]["history"]))


def test_gap_wise_entry_point_is_unchanged():
    from ainp.janssen import janssen_inpaint, janssen_windowed
    case = W.CASES[0]
    x, mask = _gapped(case)
    before, h0 = janssen_inpaint(x, mask, p=32, w=300, maxit=4, return_history=True)
    janssen_windowed(x, mask, p=32, w=256, a=64, wtype=W.WTYPES, maxit=4)
    after, h1 = janssen_inpaint(x, mask, p=32, w=300, maxit=4, return_history=True)
    assert np.array_equal(before, after)
    assert np.array_equal(h0[0]["history"], h1[0]["history"])
    ref, _, _ = R.janssen(x[600:1280], 300, 80, 32, 4)
    assert np.max(np.abs(after[900:980] - ref[300:380])) <= 1e-9 * np.max(np.abs(x[900:980]))


def test_run_ar_evaluation_janssen_hann(tmp_path):
    import utils
    from models import model_eval
    from models.AudioReg import gap_sdr
    clip = "81-121543-0008.flac"
    src = tmp_path / "in"
    src.mkdir()
    shutil.copy(os.path.join(FLAC, clip), src / clip)
    p, w, a, maxit = 64, 512, 128, 2
    sdrs = model_eval.run_ar_evaluation(str(src), str(tmp_path / "out"),
                                        algorithm="janssen_hann", p=p, w=w, a=a, maxit=maxit)
    assert list(sdrs) == [clip] and np.isfinite(sdrs[clip])
    out = tmp_path / "out" / f"{os.path.splitext(clip)[0]}_janssen_hann_inpainted.flac"
    assert out.exists()
    audio, sr = utils.load_audio(os.path.join(FLAC, clip))
    audio = audio.astype(np.float64)
    written, wsr = utils.load_audio(str(out))
    assert wsr == sr and len(written) == len(audio)
    s0, h = int(2.0 * sr), int(0.08 * sr)
    res, lo = W.inpaint_gap(audio, s0, s0 + h, p, maxit, w, a, "hann")
    ref = audio.copy()
    ref[s0:s0 + h] = res[s0 - lo:s0 + h - lo, -1]
    mask = np.ones(len(audio), bool)
    mask[s0:s0 + h] = False
    from ainp.janssen import janssen_windowed
    got = janssen_windowed(audio, mask, p=p, w=w, a=a, maxit=maxit)
    assert sdrs[clip] == gap_sdr(audio, got, mask)
    d = np.max(np.abs(got[s0:s0 + h] - ref[s0:s0 + h])) / np.max(np.abs(ref[s0:s0 + h]))
    print(f"run_ar_evaluation janssen_hann: gap SDR {sdrs[clip]:.3f} dB, "
          f"against the reference {d:.3e}")
    assert d <= 1e-8
