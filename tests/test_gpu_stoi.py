"""ainp_stoi on the GPU against the float64 numpy oracle (tests/stoi_ref.py),
STOI and ESTOI.  The bound is 100 times the pair's measured sensitivity to a
relative 1e-13 perturbation of both inputs (tests/test_cpu_stoi.py prints it
for the fixtures): the margin covers the kernel's FFT factorisation and
summation order.  Frame counts, the sentinel and the all-zero score are exact,
and a row's score is the same bits alone, in a ragged batch and on a second
launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = [f.name for f in S.FIXTURES]


def _dev(rows):
    """A list of 1-D float64 arrays -> a zero-padded [rows, stride] cuda tensor."""
    stride = max(2, -(-max(len(r) for r in rows) // 2) * 2)
    host = np.zeros((len(rows), stride))
    for i, r in enumerate(rows):
        host[i, :len(r)] = r
    return torch.from_numpy(host).cuda()


def _run(clean, restored, clean_row, extended):
    from ainp import ops
    rows = _dev(clean + restored)
    score, frames = ops.stoi(rows[:len(clean)], rows[len(clean):], [len(c) for c in clean],
                             clean_row, extended)
    return score.cpu().numpy(), frames.cpu().numpy()


@pytest.mark.parametrize("name", FIX)
def test_matches_oracle(name):
    f = S.BY_NAME[name]
    bound = 100.0 * S.sensitivity(name)
    for extended in (False, True):
        want, T = S.reference(name, extended)
        got, frames = _run([f.clean], [f.restored], [0], extended)
        err = abs(got[0] - want)
        ratio = err / S.sensitivity(name) if S.sensitivity(name) else 0.0
        print(f"{name} {'ESTOI' if extended else 'STOI'}: got {got[0]!r} want {want!r} "
              f"err {err:.2e} bound {bound:.2e} err/sensitivity {ratio:.3f}")
        assert frames.tolist() == [T]
        if T < S.N:
            assert got[0] == 1e-5
        if name == "zeros":
            assert got[0] == 0.0
        assert err <= bound


@pytest.mark.parametrize("extended", [False, True])
def test_ragged_batch_is_bit_equal_to_single_pairs(extended):
    names = ["len4224", "silence", "len8000"]
    clean = [S.BY_NAME[n].clean for n in names]
    clean_row = [2, 0, 0, 1, 2, 2, 0]
    rng = np.random.default_rng(77)
    restored = [S.BY_NAME[names[c]].restored + 0.01 * k * rng.standard_normal(len(clean[c]))
                for k, c in enumerate(clean_row)]
    got, frames = _run(clean, restored, clean_row, extended)
    again, frames2 = _run(clean, restored, clean_row, extended)
    assert np.array_equal(got, again) and np.array_equal(frames, frames2)
    assert frames.tolist() == [S.reference(n, extended)[1] for n in names]
    assert 0 < frames[1] < S.frames(9000)
    assert len(set(got.tolist())) == len(clean_row) and np.all(np.isfinite(got))
    for r, c in enumerate(clean_row):
        alone, fr = _run([clean[c]], [restored[r]], [0], extended)
        assert alone[0] == got[r], (r, c, alone[0], got[r])
        assert fr[0] == frames[c]
        want, _ = S.score(clean[c], restored[r], extended)
        assert abs(got[r] - want) <= 100.0 * S.pair_sensitivity(clean[c], restored[r])


def _resampled(x):
    from ainp import ops
    return ops.resample_poly(torch.from_numpy(np.ascontiguousarray(x)).cuda(), 5, 8).cpu().numpy()


def test_16k_input_is_the_oracle_on_the_resampled_signals():
    from ainp.stoi import stoi
    clean = S.speechlike(9600, 21)                      # 0.6 s at 16 kHz
    restored = clean + 0.03 * np.random.default_rng(22).standard_normal(9600)
    restored[4000:4600] = 0.0
    x10, y10 = _resampled(clean), _resampled(restored)
    assert x10.size == 6000 and S.threshold_margin(x10) >= 1e-6
    bound = 100.0 * S.pair_sensitivity(x10, y10)
    for extended in (False, True):
        got = stoi(clean, restored, fs=16000, extended=extended)
        want, T = S.score(x10, y10, extended)
        print(f"16 kHz {'ESTOI' if extended else 'STOI'}: got {got!r} want {want!r} "
              f"bound {bound:.2e}")
        assert isinstance(got, float) and T == 45
        assert abs(got - want) <= bound
    # k restored signals against one clean signal, and the batch layouts
    k3 = np.stack([restored, clean, 0.5 * restored])
    got = stoi(clean, k3, fs=16000)
    assert got.shape == (3,) and got[0] == stoi(clean, restored, fs=16000)
    assert abs(got[1] - 1.0) <= 1e-12
    lst = stoi([clean, clean[:8000]], [k3, restored[:8000]], fs=16000)
    assert np.array_equal(lst[0], got) and isinstance(lst[1], float)
    bat = stoi(np.stack([clean, clean]), np.stack([restored, clean]), fs=16000)
    assert bat.shape == (2,) and bat[0] == got[0] and bat[1] == got[1]


def test_stoi_curve_of_a_janssen_history():
    from ainp.janssen import janssen_inpaint
    from ainp.stoi import stoi, stoi_curve
    clean = S.speechlike(16000, 31)                     # 1 s at 16 kHz
    mask = np.ones(16000, bool)
    mask[8000:8160] = False
    restored, info = janssen_inpaint(clean, mask, p=32, w=1024, maxit=3, return_history=True)
    assert len(info) == 1 and info[0]["iters"] == 3
    curve = stoi_curve(clean, mask, info, fs=16000)
    assert curve.shape == (3,) and np.all(np.isfinite(curve))
    x10, y10 = _resampled(clean), _resampled(restored)
    assert S.threshold_margin(x10) >= 1e-6
    bound = 100.0 * S.pair_sensitivity(x10, y10)
    last = stoi(clean, restored, fs=16000)
    print(f"curve {curve.tolist()} stoi(clean, restored) {last!r} bound {bound:.2e}")
    assert abs(curve[-1] - last) <= bound
    assert abs(last - S.score(x10, y10)[0]) <= bound
    # an iteration that was not completed is NaN from there on
    cut = [dict(info[0], history=info[0]["history"].copy())]
    cut[0]["history"][1:] = np.nan
    c2 = stoi_curve(clean, mask, cut, fs=16000)
    assert c2[0] == curve[0] and np.all(np.isnan(c2[1:]))


def test_run_stoi_evaluation(tmp_path):
    import utils
    from ainp.stoi import stoi
    from models import model_eval as ME
    src, rec = tmp_path / "in", tmp_path / "out"
    for i, n_rest in enumerate((16000, 15000)):        # the second pair is truncated
        clean = S.speechlike(16000, 41 + i)
        restored = clean + 0.02 * np.random.default_rng(51 + i).standard_normal(16000)
        utils.save_audio(clean, str(src / f"clip{i}.flac"), sample_rate=16000)
        utils.save_audio(restored[:n_rest], str(rec / f"clip{i}_janssen_inpainted.flac"),
                         sample_rate=16000)
    utils.save_audio(S.speechlike(16000, 43), str(src / "alone.flac"), sample_rate=16000)
    for extended in (False, True):
        got = ME.run_stoi_evaluation(str(src), str(rec), "janssen", extended=extended)
        assert sorted(got) == ["clip0.flac", "clip1.flac"]
        for i in range(2):
            c, sr = utils._read_any(str(src / f"clip{i}.flac"))
            r, sr2 = utils._read_any(str(rec / f"clip{i}_janssen_inpainted.flac"))
            assert sr == sr2 == 16000
            n = min(len(c), len(r))
            want = stoi(c.mean(axis=1).astype(np.float64)[:n],
                        r.mean(axis=1).astype(np.float64)[:n], fs=16000, extended=extended)
            assert got[f"clip{i}.flac"] == want and 0.0 < want < 1.0


def test_operator_refuses_on_the_host():
    from ainp import ops
    from ainp import stoi as st
    x = torch.zeros(2, 4096, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="clean_row"):
        ops.stoi(x, x, [4096, 4096], [0, 2])
    with pytest.raises(ValueError, match="every n"):
        ops.stoi(x, x, [4096, 4097], [0, 1])
    with pytest.raises(RuntimeError, match="clean_row"):     # the ABI's own check
        torch.ops.ainp.stoi(x, x, torch.tensor([4096, 4096], dtype=torch.int32),
                            torch.tensor([0, 2], dtype=torch.int32),
                            torch.tensor([4096, 4096, 0, 2], dtype=torch.int32, device="cuda"),
                            False, torch.empty(1 << 20, dtype=torch.float64, device="cuda"),
                            torch.empty(2, dtype=torch.float64, device="cuda"),
                            torch.empty(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="limit"):
        st.stoi(np.zeros(st.MAX_LEN + 1), np.zeros(st.MAX_LEN + 1), fs=10000)
