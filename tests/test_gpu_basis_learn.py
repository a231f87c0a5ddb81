"""GPU tests of the basis learning (csrc/basis_learn.hip and ainp_spain_dgt of
csrc/spain_learned.hip through ainp.basis_learn, ainp.spain_learned and
models/model_eval) against the float64 NumPy restatement in
tests/basis_learn_ref.py.

The bound is derived in test_cpu_basis_learn.py on the reference alone: U within
BOUND_U = 5e-12 (max abs), P, D and the sparsities within BOUND_OBJ = 1e-13
(relative), iteration counts, levels and kept flags equal.  The same file
asserts that every case used here stays clear of gap_tol at every gap check and
of a tie in every accept / reject decision.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import basis_learn_ref as R
import spain_learned_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")
BOUND_U = 5e-12
BOUND_OBJ = 1e-13


def _learn(X, **kw):
    from ainp.basis_learn import learn_basis
    return learn_basis(X, gap_tol=R.GAP_TOL, return_trace=True, **kw)


def _check(U, info, ref, tag):
    tr, rt = info["trace"], ref["trace"]
    assert tr.shape == rt.shape, (tr.shape, rt.shape)
    fin = np.isfinite(rt[:, 0])
    assert np.array_equal(np.isfinite(tr), np.isfinite(rt)) and np.all(np.isnan(tr[~fin]))
    rel = lambda c: float(np.max(np.abs(tr[fin, c] - rt[fin, c]) / np.abs(rt[fin, c])))
    d_u = float(np.abs(U - ref["U"]).max())
    d_s = max(abs(info[k] - ref[k]) / ref[k] for k in ("sparsity_init", "sparsity_final"))
    print(f"{tag}: U {d_u:.3e}, P {rel(2):.3e}, D {rel(3):.3e}, sparsity {max(rel(4), d_s):.3e}, "
          f"iterations {tr[fin, 1].astype(int).tolist()}, kept {tr[fin, 5].astype(int).tolist()}")
    assert np.array_equal(tr[fin, 0], rt[fin, 0])            # levels
    assert np.array_equal(tr[fin, 1], rt[fin, 1])            # iteration counts
    assert np.array_equal(tr[fin, 5], rt[fin, 5])            # kept / undone
    assert U.dtype == np.complex128 and U.shape == ref["U"].shape
    assert d_u <= BOUND_U
    assert max(rel(2), rel(3), rel(4), d_s) <= BOUND_OBJ
    assert np.abs(U @ U.conj().T - np.eye(len(U))).max() <= 1e-10


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity(name):
    """Every shape and branch: one column, fewer columns than a wave, columns
    that are no multiple of a wave, more than a workgroup has lanes, a zero row
    and column (step 0: no NaN), the level at both ends of its range, the
    reject-and-halve branch, and the largest K."""
    U, info = _learn(R.case_input(name), **R.CASES[name][1])
    assert np.all(np.isfinite(U))
    _check(U, info, R.case_reference(name), name)


def test_chunks_and_repeats_give_the_same_bits(monkeypatch):
    """How often the host looks at the stop flag changes nothing, nor does the call."""
    X = R.case_input("k17_m24")
    kw = dict(level_init=0.05, cnt_max=3, max_iters=3000)
    U0, i0 = _learn(X, **kw)
    U1, i1 = _learn(X, **kw)
    assert np.array_equal(U0, U1) and np.array_equal(i0["trace"], i1["trace"], equal_nan=True)
    assert np.all(i0["trace"][:3, 1] < 3000)
    for chunk in ("1", "7", "32", "0"):
        monkeypatch.setenv("AINP_BASIS_LEARN_CHUNK", chunk)
        U2, i2 = _learn(X, **kw)
        monkeypatch.delenv("AINP_BASIS_LEARN_CHUNK")
        assert np.array_equal(U0, U2), chunk
        assert np.array_equal(i0["trace"], i2["trace"], equal_nan=True), chunk
        assert (i0["sparsity_init"], i0["sparsity_final"]) == \
            (i2["sparsity_init"], i2["sparsity_final"])


def test_out_of_range_arguments_raise_before_a_launch():
    from ainp import ops
    from ainp.basis_learn import learn_basis
    X = R.case_input("k5_m3")
    bad = [dict(level_init=0.0), dict(level_init=0.3), dict(epsilon=0.0), dict(cnt_max=0),
           dict(cnt_max=65), dict(gap_tol=-1.0), dict(check=0), dict(check=11, max_iters=10),
           dict(max_iters=(1 << 20) + 1)]
    for kw in bad:
        with pytest.raises(ValueError):
            learn_basis(X, **kw)
    for shape in ((4, 3), (16, 3), (5, 0), (5,)):
        with pytest.raises(ValueError):
            learn_basis(np.ones(shape, complex))
    with pytest.raises(ValueError, match="finite"):
        learn_basis(np.full((5, 3), np.nan, complex))
    # the operator itself checks shapes on the host and the C entry names the rule
    Xd = torch.from_numpy(np.array(X).view(np.float64).reshape(5, 3, 2)).cuda()
    out = lambda *s: torch.empty(s, device="cuda", dtype=torch.float64)
    ws = torch.empty(1 << 16, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="trace"):
        torch.ops.ainp.basis_learn(Xd, 0.02, 0.001, 4, 1e-5, 100, 10, out(5, 5, 2), out(2),
                                   out(3, 6), ws)
    with pytest.raises(RuntimeError, match="level_init"):
        torch.ops.ainp.basis_learn(Xd, 0.5, 0.001, 4, 1e-5, 100, 10, out(5, 5, 2), out(2),
                                   out(4, 6), ws)
    with pytest.raises(ValueError):
        ops.basis_learn(Xd[:, :, :1].contiguous())
    with pytest.raises(ValueError):
        ops.spain_dgt(torch.zeros(1, 100, device="cuda", dtype=torch.float64), w=16, a=4)


def test_spain_training_frames():
    from ainp.basis_learn import spain_training_frames
    for name, context in (("w64", None), ("w64", 3), ("w16_odd_frames", None), ("w16_wraps", 2)):
        w, a, M, L, gaps = S.CASES[name][:5]
        for Ls in (L, L - 10):                            # a whole number of frames, and padding
            x, obs = S.signal(Ls), S.mask(Ls, gaps)
            X = spain_training_frames(x, obs, w, a, M, context=context)
            ref, frames = R.training_frames(x, obs, w, a, M, context)
            assert X.dtype == np.complex128 and X.shape == ref.shape == (M // 2 + 1, len(frames))
            d = np.abs(X - ref).max() / np.abs(ref).max()
            print(f"{name} Ls {Ls} context {context}: {len(frames)} frames, {d:.3e}")
            assert d <= 1e-13
    with pytest.raises(ValueError, match="no frame"):
        spain_training_frames(S.signal(64), S.mask(64, ((10, 50),)), 32, 8, 64)


def test_inpaint_with_a_learned_basis():
    """End to end on the synthetic signal of the spain_learned tests: basis
    "learn" is spain_learn_basis on the signal's own frames, passed on; the other
    values of basis run as they did."""
    from models.AudioReg import spain_learn_basis, spain_learned_inpaint
    from ainp.spain_learned import check_basis
    clean, obs, Ur, w, a, M = S.case_input("w64")
    opts = dict(cnt_max=4, max_iters=4000)
    U, info = spain_learn_basis(clean, obs, w, a, M, return_trace=True, **opts)
    assert np.array_equal(check_basis(U, M), U)
    assert info["sparsity_final"] < info["sparsity_init"]
    for alg in S.ALGS:
        kw = dict(algorithm=alg, w=w, a=a, M=M, return_history=True)
        # every other value of basis: the same bits before and after a learning call
        plain, hp = spain_learned_inpaint(clean, obs, **kw)
        given, hg = spain_learned_inpaint(clean, obs, basis=Ur, **kw)
        learned, hl = spain_learned_inpaint(clean, obs, basis=dict(opts), **kw)
        plain2, hp2 = spain_learned_inpaint(clean, obs, **kw)
        given2, hg2 = spain_learned_inpaint(clean, obs, basis=Ur, **kw)
        assert np.array_equal(plain, plain2) and np.array_equal(given, given2)
        assert np.array_equal(hp[0]["objective"], hp2[0]["objective"], equal_nan=True)
        assert np.array_equal(hg[0]["objective"], hg2[0]["objective"], equal_nan=True)
        assert hg[0]["iters"] == S.case_reference("w64", alg, True)["iters"]
        explicit, he = spain_learned_inpaint(clean, obs, basis=U, **kw)
        assert np.array_equal(learned, explicit) and hl[0]["iters"] == he[0]["iters"]
        assert np.array_equal(hl[0]["objective"], he[0]["objective"], equal_nan=True)
        assert np.array_equal(learned[obs], clean[obs]) and np.all(np.isfinite(learned))
        print(f"{alg}: gap SDR learned {S.gap_sdr(clean, learned, obs):.2f} dB, random basis "
              f"{S.gap_sdr(clean, given, obs):.2f} dB, none {S.gap_sdr(clean, plain, obs):.2f} dB")
    # two signals learn one basis each, each its own launch sequence
    short, m2 = S.signal(500) * 0.5, S.mask(500, ((200, 215),))
    outs = spain_learned_inpaint([clean, short], [obs, m2], basis=dict(opts), w=w, a=a, M=M, maxit=8)
    for x, m, out in zip((clean, short), (obs, m2), outs):
        Ui = spain_learn_basis(x, m, w, a, M, **opts)
        assert np.array_equal(out, spain_learned_inpaint(x, m, basis=Ui, w=w, a=a, M=M, maxit=8))
    # the string form is spain_learn_basis with its defaults
    out = spain_learned_inpaint(short, m2, basis="learn", w=w, a=a, M=M, maxit=8)
    Ui = spain_learn_basis(short, m2, w, a, M)
    assert np.array_equal(out, spain_learned_inpaint(short, m2, basis=Ui, w=w, a=a, M=M, maxit=8))


def test_run_spain_learned_evaluation_learns(tmp_path):
    import utils
    from models import model_eval
    E = S.EVAL
    clip = E["clip"]
    src = tmp_path / "in"
    src.mkdir()
    shutil.copy(os.path.join(FLAC, clip), src / clip)
    sdrs = model_eval.run_spain_learned_evaluation(
        str(src), str(tmp_path / "out"), basis=dict(context=8, cnt_max=2, max_iters=500),
        algorithm="sspain", w=E["w"], a=E["a"], maxit=E["maxit"])
    assert list(sdrs) == [clip] and np.isfinite(sdrs[clip])
    out = tmp_path / "out" / f"{os.path.splitext(clip)[0]}_sspain_learned_inpainted.flac"
    assert out.exists()
    audio, sr = utils.load_audio(os.path.join(FLAC, clip))
    written, wsr = utils.load_audio(str(out))
    assert wsr == sr and len(written) == len(audio)
