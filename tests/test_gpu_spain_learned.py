"""GPU tests of SPAIN over the whole signal with a unitary basis
(csrc/spain_learned.hip through ainp.spain_learned.spain_learned_inpaint and
models/model_eval.run_spain_learned_evaluation) against the float64 NumPy
restatement in tests/spain_learned_ref.py.

The bound is the project's: the gap within 1e-9 * max|clean gap|, every
objective within 1e-9 (relative), the pass counts equal, observed samples
bit-equal.  test_cpu_spain_learned.py asserts on the reference alone that every
input used here is far from a tie and from epsilon, and that the bound lies
between float64 round-off and what float32 input moves.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import spain_learned_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")
BOUND = 1e-9


def _check(out, info, clean, obs, ref, tag):
    scale = np.max(np.abs(clean[~obs]))
    Ls = len(clean)
    d = np.max(np.abs(out[~obs] - ref["out"][:Ls][~obs])) / scale
    obj, robj = info["objective"], ref["obj"]
    assert obj.shape == robj.shape, (obj.shape, robj.shape)
    fin = np.isfinite(robj)
    assert np.array_equal(np.isfinite(obj), fin) and np.all(np.isnan(obj[~fin]))
    d_obj = np.max(np.abs(obj[fin] - robj[fin]) / robj[fin])
    print(f"{tag}: gap {d:.3e}, objective {d_obj:.3e}, passes {info['iters']}")
    assert info["iters"] == ref["iters"]
    assert d <= BOUND and d_obj <= BOUND
    assert out.dtype == np.float64 and np.array_equal(out[obs], clean[obs])


def _run(name, alg, with_basis, **kw):
    from ainp.spain_learned import spain_learned_inpaint
    clean, obs, U, w, a, M = R.case_input(name)
    out, info = spain_learned_inpaint(clean, obs, basis=U if with_basis else None, algorithm=alg,
                                      w=w, a=a, M=M, epsilon=R.EPSILON, return_history=True, **kw)
    assert len(info) == 1 and info[0]["signal"] == 0
    return clean, obs, out, info[0]


@pytest.mark.parametrize("with_basis", [False, True], ids=["I", "U"])
@pytest.mark.parametrize("alg", R.ALGS)
@pytest.mark.parametrize("name", R.PARITY)
def test_parity(name, alg, with_basis):
    clean, obs, out, info = _run(name, alg, with_basis)
    _check(out, info, clean, obs, R.case_reference(name, alg, with_basis),
           f"{name} {alg} {'U' if with_basis else 'I'}")


@pytest.mark.parametrize("alg", R.ALGS)
def test_explicit_identity_is_the_path_without_a_basis(alg):
    from ainp.spain_learned import spain_learned_inpaint
    clean, obs, _, w, a, M = R.case_input("w64")
    kw = dict(algorithm=alg, w=w, a=a, M=M, return_history=True)
    plain, hp = spain_learned_inpaint(clean, obs, **kw)
    eye, he = spain_learned_inpaint(clean, obs, basis=np.eye(M // 2 + 1), **kw)
    assert he[0]["iters"] == hp[0]["iters"]
    assert np.abs(eye - plain).max() <= BOUND * R.gap_scale("w64")
    fin = np.isfinite(hp[0]["objective"])
    assert np.array_equal(np.isfinite(he[0]["objective"]), fin)
    assert np.max(np.abs(he[0]["objective"][fin] / hp[0]["objective"][fin] - 1)) <= BOUND
    _check(eye, he[0], clean, obs, R.case_reference("w64", alg, False), f"identity {alg}")


def test_equal_magnitudes_go_to_the_lower_row():
    """A unit impulse at a frame centre has an exactly flat spectrum there: H_1
    of the first pass chooses among equal magnitudes, and the objectives of the
    passes after it tell which row it kept (test_cpu_spain_learned.py: the other
    rule moves them by more than 1e-6, and no other selection is a near-tie)."""
    from ainp.spain_learned import spain_learned_inpaint
    T = R.TIE
    x, obs = R.tie_input()
    for alg in R.ALGS:
        out, info = spain_learned_inpaint(x, obs, algorithm=alg, w=T["w"], a=T["a"], M=T["M"],
                                          epsilon=T["epsilon"], maxit=T["maxit"],
                                          return_history=True)
        ref = R.tie_reference(alg)
        d_obj = np.max(np.abs(info[0]["objective"] - ref["obj"]) / ref["obj"])
        d = np.max(np.abs(out - ref["out"]))
        print(f"tie {alg}: objectives {d_obj:.3e}, signal {d:.3e}")
        assert info[0]["iters"] == ref["iters"] == T["maxit"]
        assert d_obj <= BOUND and d <= BOUND
        assert np.array_equal(out[obs], x[obs])


@pytest.mark.parametrize("alg", R.ALGS)
def test_largest_transform(alg):
    """M 2048, w 1024, a 256 with a basis: the longest LDS transform, the largest
    basis (1025 x 1025, every edge tile of the product live) and 32 frames.
    After 8 passes A-SPAIN's smallest objective may still be the first, whose
    iterate is the gapped input, so the eight objectives carry the check: each
    depends on every transform, product and selection before it."""
    from ainp.spain_learned import spain_learned_inpaint
    B = R.BIG
    clean, obs = R.signal(B["L"]), R.mask(B["L"], B["gaps"])
    out, info = spain_learned_inpaint(clean, obs, basis=R.basis(B["M"] // 2 + 1, B["level"]),
                                      algorithm=alg, w=B["w"], a=B["a"], M=B["M"],
                                      epsilon=R.EPSILON, maxit=B["maxit"], return_history=True)
    _check(out, info[0], clean, obs, R.big_reference(alg), f"largest {alg}")


@pytest.mark.parametrize("with_basis", [False, True], ids=["I", "U"])
@pytest.mark.parametrize("alg", R.ALGS)
def test_other_schedule(alg, with_basis):
    name, extra = R.SCHEDULE
    clean, obs, out, info = _run(name, alg.upper(), with_basis, **dict(extra))
    _check(out, info, clean, obs, R.case_reference(name, alg, with_basis, extra=extra),
           f"{name} {alg} {dict(extra)}")


def test_nothing_missing_comes_back_unchanged():
    from ainp.spain_learned import spain_learned_inpaint
    x = R.signal(700)
    out, info = spain_learned_inpaint(x, np.ones(700, bool), w=64, a=16, return_history=True)
    assert np.array_equal(out, x) and info[0]["iters"] == 0
    assert info[0]["objective"].shape == (65,) and np.all(np.isnan(info[0]["objective"]))
    # and next to a signal with a gap
    clean, obs, _, w, a, M = R.case_input("w64")
    outs, info = spain_learned_inpaint([x, clean], [np.ones(700, bool), obs], w=w, a=a, M=M,
                                       return_history=True)
    assert np.array_equal(outs[0], x) and info[0]["iters"] == 0
    _check(outs[1], info[1], clean, obs, R.case_reference("w64", "aspain", False), "after a whole one")


def test_batch_is_the_separate_calls_and_repeats(monkeypatch):
    """Signals of one call are independent problems with their own stops; a third
    one of another length is another group.  The bits do not depend on the
    batch, on the call, or on how often the host looks at the stop flags."""
    from ainp.spain_learned import spain_learned_inpaint
    one, m1, U, w, a, M = R.case_input("w64")
    two, m2 = R.case_input("w64_quiet")[:2]
    short, m3 = R.signal(500) * 0.5, R.mask(500, ((200, 215),))       # pads to 512
    sigs, masks = [one, two, short], [m1, m2, m3]
    for alg in R.ALGS:
        kw = dict(basis=U, algorithm=alg, w=w, a=a, M=M, return_history=True)
        outs, info = spain_learned_inpaint(sigs, masks, **kw)
        again, info2 = spain_learned_inpaint(sigs, masks, **kw)
        assert [h["iters"] for h in info[:2]] == [R.case_reference(n, alg, True)["iters"]
                                                  for n in ("w64", "w64_quiet")]
        for i, (x, m) in enumerate(zip(sigs, masks)):
            alone, hist = spain_learned_inpaint(x, m, **kw)
            assert np.array_equal(outs[i], alone) and np.array_equal(again[i], alone)
            assert info[i]["iters"] == hist[0]["iters"] == info2[i]["iters"]
            assert np.array_equal(info[i]["objective"], hist[0]["objective"], equal_nan=True)
            assert np.array_equal(info2[i]["objective"], hist[0]["objective"], equal_nan=True)
        if alg == "sspain":
            assert info[0]["iters"] != info[1]["iters"]              # two stops in one launch
        for chunk in ("1", "7", "0"):
            monkeypatch.setenv("AINP_SPAIN_LEARNED_CHUNK", chunk)
            other, info3 = spain_learned_inpaint(sigs, masks, **kw)
            monkeypatch.delenv("AINP_SPAIN_LEARNED_CHUNK")
            for i in range(3):
                assert np.array_equal(other[i], outs[i]) and info3[i]["iters"] == info[i]["iters"]
                assert np.array_equal(info3[i]["objective"], info[i]["objective"], equal_nan=True)
    # the 2-D layout with NaN marks, as a tensor
    marked = np.stack([np.where(m1, one, np.nan), np.where(m2, two, np.nan)])
    out = spain_learned_inpaint(torch.from_numpy(marked), w=w, a=a, M=M)
    assert out.shape == marked.shape
    assert np.array_equal(out[0], spain_learned_inpaint(one, m1, w=w, a=a, M=M))


def test_run_spain_learned_evaluation(tmp_path):
    """The files are written and the gap SDRs are the reference's
    (test_cpu_spain_learned.py: the clip's runs are clear of ties and of epsilon).
    With so few passes A-SPAIN's smallest objective is the first, so its result
    is the gapped clip and its SDR 0 dB on both sides; S-SPAIN's is not."""
    import utils
    from models import model_eval
    from models.AudioReg import gap_sdr
    E = R.EVAL
    clip = E["clip"]
    src = tmp_path / "in"
    src.mkdir()
    shutil.copy(os.path.join(FLAC, clip), src / clip)
    w, a, M, maxit = E["w"], E["a"], E["M"], E["maxit"]
    audio, sr = utils.load_audio(os.path.join(FLAC, clip))
    audio = audio.astype(np.float64)
    s0, h = int(2.0 * sr), int(0.08 * sr)
    obs = np.ones(len(audio), bool)
    obs[s0:s0 + h] = False
    U = R.basis(M // 2 + 1, E["level"])
    for basis, suffix in ((None, "global"), (U, "learned")):
        for alg in R.ALGS:
            sdrs = model_eval.run_spain_learned_evaluation(
                str(src), str(tmp_path / "out"), basis=basis, algorithm=alg, w=w, a=a, maxit=maxit)
            assert list(sdrs) == [clip] and np.isfinite(sdrs[clip])
            out = tmp_path / "out" / f"{os.path.splitext(clip)[0]}_{alg}_{suffix}_inpainted.flac"
            assert out.exists()
            written, wsr = utils.load_audio(str(out))
            assert wsr == sr and len(written) == len(audio)
            ref = R.padded_reference(audio, obs, basis, alg, w, a, M, maxit=maxit)
            ref_sdr = gap_sdr(audio, ref["out"][:len(audio)], obs)
            print(f"run_spain_learned_evaluation {alg} {suffix}: gap SDR {sdrs[clip]:.6f} dB, "
                  f"reference {ref_sdr:.6f} dB")
            assert abs(sdrs[clip] - ref_sdr) <= 1e-6
