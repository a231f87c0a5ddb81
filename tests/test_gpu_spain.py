"""GPU tests of A-SPAIN / S-SPAIN (csrc/spain.hip between the gather and the
overlap-add of csrc/janssen_windows.hip, through ainp.spain.spain_inpaint and
models/model_eval.run_spain_evaluation) against the float64 NumPy restatement
in tests/spain_ref.py.

Bound of the parity cases: 1e-9 * max|clean gap|, the project's bound for small
shapes.  The hard threshold is discontinuous, so the bound holds only on inputs
where no selection is a near-tie and no objective lies at epsilon;
test_cpu_spain.py asserts both on the reference alone for every case used here,
and that two float64 formulations of the transforms agree well inside the bound
while float32 input misses it.  Bundled clip: the larger of 1e-8 * max|gap| and
ten times what the two CPU formulations differ by on that input.  Every test
prints its measured figure; DESIGN §14.1 records them.  Measured on an MI355X:
parity gap <= 9.0e-15 and objectives <= 3.7e-13 over all cases, the largest
transform's objectives 1.1e-15, the bundled clip 2.7e-15.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import janssen_ref as R
import spain_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")

ALGS, PARITY, OTHER = S.ALGS, S.PARITY, S.OTHER


def _check(out, info, x, mask, s0, e0, ref, tag):
    scale = np.max(np.abs(x[s0:e0]))
    d = np.max(np.abs(out[s0:e0] - ref["out"][s0:e0])) / scale
    obj, robj = info["objective"], ref["obj"]
    assert obj.shape == robj.shape, (obj.shape, robj.shape)
    fin = np.isfinite(robj)
    assert np.array_equal(np.isfinite(obj), fin) and np.all(np.isnan(obj[~fin]))
    d_obj = np.max(np.abs(obj[fin] - robj[fin]) / robj[fin])
    print(f"{tag}: gap {d:.3e}, objective {d_obj:.3e}, iterations {info['iters']}")
    assert info["iters"] == ref["iters"]
    assert d <= 1e-9 and d_obj <= 1e-9
    assert out.dtype == np.float64 and np.array_equal(out[mask], x[mask])


@pytest.mark.parametrize("case,alg,eps", PARITY,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{g}-{e}" for c, g, e in PARITY])
def test_parity(case, alg, eps):
    from ainp.spain import spain_inpaint
    w, a, s0, e0, n = case
    x, mask = S.case_signal(case), S.case_mask(case)
    out, info = spain_inpaint(x, mask, algorithm=alg, w=w, a=a, epsilon=eps, return_history=True)
    assert len(info) == 1 and (info[0]["signal"], info[0]["start"], info[0]["end"]) == (0, s0, e0)
    _check(out, info[0], x, mask, s0, e0, S.case_reference(case, alg, eps), f"{alg} {case} {eps}")


@pytest.mark.parametrize("case,kw", OTHER, ids=["red1-w64", "red4-w64", "s2-r3-w128"])
@pytest.mark.parametrize("alg", ALGS)
def test_other_frames_and_schedules(case, kw, alg):
    from ainp.spain import spain_inpaint
    w, a, s0, e0, n = case
    x, mask = S.case_signal(case), S.case_mask(case)
    out, info = spain_inpaint(x, mask, algorithm=alg.upper(), w=w, a=a, return_history=True, **kw)
    _check(out, info[0], x, mask, s0, e0, S.case_reference(case, alg, 0.1, **kw),
           f"{alg} {case} {kw}")


@pytest.mark.parametrize("alg", ALGS)
def test_largest_transform(alg):
    """w 4096, red 2: M 8192, the whole LDS budget."""
    from ainp.spain import spain_inpaint
    B = S.BIG
    x, mask = S.big_signal()
    out, info = spain_inpaint(x, mask, algorithm=alg, w=B["w"], a=B["a"], red=B["red"],
                              maxit=B["maxit"], return_history=True)
    _check(out, info[0], x, mask, B["s0"], B["e0"], S.big_reference(alg), f"{alg} largest")


def test_equal_magnitudes_go_to_the_lower_index():
    """A unit impulse has a flat spectrum: H_1 of the first pass chooses among
    exactly equal magnitudes, and the objectives of the passes after it tell
    which bin it kept (test_cpu_spain.py: the other rule moves them by more than
    1e-6, and no later selection is a near-tie)."""
    from ainp import ops
    row, obs, g0, h = S.tie_row()
    for alg, solver in (("aspain", S.aspain), ("sspain", S.sspain)):
        for red in (1, 2):
            rec, objs = solver(row, obs, red=red, epsilon=1e-3, maxit=4)
            sol = torch.from_numpy(np.stack([row, row])).cuda()
            iters, hist = ops.spain(sol, [g0, g0], [h, h], algorithm=alg, red=red, epsilon=1e-3,
                                    maxit=4, return_history=True)
            got, hist = sol.cpu().numpy(), hist.cpu().numpy()
            d_obj = np.max(np.abs(hist[0] - objs) / np.array(objs))
            d = np.max(np.abs(got[0] - rec))
            print(f"{alg} red {red}: objectives {d_obj:.3e}, row {d:.3e}")
            assert iters.tolist() == [4, 4] and d_obj <= 1e-9 and d <= 1e-9
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0][obs], row[obs])


def test_batch_is_the_separate_calls_and_repeats():
    from ainp.spain import spain_inpaint
    w, a = 128, 32
    sigs = [R.sinusoid_mix(n, noise=1e-3, seed=i) for i, n in enumerate((1500, 1201, 1800))]
    gaps = [((300, 340), (1000, 1001)), ((531, 555), (900, 1000)), ((40, 70), (1700, 1760))]
    masks = []
    for x, gs in zip(sigs, gaps):
        m = np.ones(len(x), bool)
        for s0, e0 in gs:
            m[s0:e0] = False
        masks.append(m)
    for alg in ALGS:
        outs, info = spain_inpaint(sigs, masks, algorithm=alg, w=w, a=a, return_history=True)
        again, info2 = spain_inpaint(sigs, masks, algorithm=alg, w=w, a=a, return_history=True)
        assert [(g["signal"], g["start"], g["end"]) for g in info] == [
            (i, s0, e0) for i, gs in enumerate(gaps) for s0, e0 in gs]
        rows = 0
        for i, (x, m) in enumerate(zip(sigs, masks)):
            assert np.array_equal(outs[i], again[i])
            alone, hist = spain_inpaint(x, m, algorithm=alg, w=w, a=a, return_history=True)
            assert np.array_equal(outs[i], alone), (alg, i)
            assert np.array_equal(outs[i][m], x[m])
            for g, h in zip([g for g in info if g["signal"] == i], hist):
                assert g["iters"] == h["iters"] and len(g["iters"]) > 0
                assert np.array_equal(g["objective"], h["objective"], equal_nan=True)
                rows += len(g["iters"])
        for g, g2 in zip(info, info2):
            assert np.array_equal(g["objective"], g2["objective"], equal_nan=True)
        plain = spain_inpaint(sigs, masks, algorithm=alg, w=w, a=a)
        assert all(np.array_equal(p, o) for p, o in zip(plain, outs))
        print(f"{alg}: {rows} windows of 3 signals in one launch give the bits of separate calls")
    marked = np.stack([sigs[0], sigs[0][::-1]]).copy()
    marked[:, 300:340] = np.nan
    out = spain_inpaint(torch.from_numpy(marked), w=w, a=a)
    assert out.shape == marked.shape and out.dtype == np.float64 and np.all(np.isfinite(out))
    m0 = np.ones(1500, bool)
    m0[300:340] = False
    assert np.array_equal(out[0], spain_inpaint(sigs[0], m0, w=w, a=a))


def test_no_rows():
    from ainp.spain import spain_inpaint
    x = R.sinusoid_mix(700, noise=1e-3)
    out, info = spain_inpaint(x, np.ones(700, bool), w=64, a=16, return_history=True)
    assert info == [] and np.array_equal(out, x)
    # a 200-sample gap under windows of 64: the nine windows centred on 288 .. 416 hold no
    # observed sample, have no row and add zeros; the 96 samples [304, 400) lie under
    # these alone (sample 400 meets one more window, at its zero first tap)
    w, a, s0, e0, n = S.LONG_GAP
    x, mask = S.case_signal(S.LONG_GAP), S.case_mask(S.LONG_GAP)
    for alg in ALGS:
        out, info = spain_inpaint(x, mask, algorithm=alg, w=w, a=a, return_history=True)
        ref = S.case_reference(S.LONG_GAP, alg)
        zeros = np.flatnonzero(ref["out"][s0:e0] == 0.0)
        assert set(range(304 - s0, 400 - s0)) <= set(zeros.tolist())
        assert np.all(out[s0:e0][zeros] == 0.0)
        print(f"{alg}: {len(zeros)} samples under all-missing windows alone stay zero")
        _check(out, info[0], x, mask, s0, e0, ref, f"{alg} {S.LONG_GAP}")


def test_run_spain_evaluation(tmp_path):
    import utils
    from models import model_eval
    from models.AudioReg import gap_sdr, spain_inpaint
    clip = "81-121543-0008.flac"
    src = tmp_path / "in"
    src.mkdir()
    shutil.copy(os.path.join(FLAC, clip), src / clip)
    w, a = 1024, 256
    sdrs = model_eval.run_spain_evaluation(str(src), str(tmp_path / "out"), w=w, a=a)
    assert list(sdrs) == [clip] and np.isfinite(sdrs[clip])
    out = tmp_path / "out" / f"{os.path.splitext(clip)[0]}_aspain_inpainted.flac"
    assert out.exists()
    audio, sr = utils.load_audio(os.path.join(FLAC, clip))
    audio = audio.astype(np.float64)
    written, wsr = utils.load_audio(str(out))
    assert wsr == sr and len(written) == len(audio)
    s0, h = int(2.0 * sr), int(0.08 * sr)
    mask = np.ones(len(audio), bool)
    mask[s0:s0 + h] = False
    got = spain_inpaint(audio, mask, w=w, a=a)
    assert sdrs[clip] == gap_sdr(audio, got, mask)
    ref, two = S.clip_reference(audio, s0, s0 + h, w, a)
    scale = np.max(np.abs(audio[s0:s0 + h]))
    bound = max(1e-8, 10.0 * two)
    d = np.max(np.abs(got[s0:s0 + h] - ref[s0:s0 + h])) / scale
    ref_sdr = R.gap_sdr(audio, ref, s0, h)
    # d SDR = (20 / ln 10) d|err| / |err|, and |err| moves by at most bound * scale * sqrt(h)
    err = np.linalg.norm(audio[s0:s0 + h] - ref[s0:s0 + h])
    sdr_tol = 20.0 / np.log(10.0) * bound * scale * np.sqrt(h) / err
    print(f"run_spain_evaluation aspain: gap SDR {sdrs[clip]:.3f} dB (reference {ref_sdr:.3f} dB, "
          f"allowed {sdr_tol:.1e}), gap against the reference {d:.3e}, two CPU formulations "
          f"{two:.3e}, bound {bound:.1e}")
    assert d <= bound
    assert abs(sdrs[clip] - ref_sdr) <= sdr_tol
