"""GPU tests of the Janssen autoregressive baseline (csrc/janssen.hip through
ops.janssen, ainp/janssen.py and models/model_eval.run_janssen_evaluation)
against the dense float64 reference tests/janssen_ref.py.

Bounds.  Small shapes (condition number 5e2 .. 4e3): two independent float64
solvers differ by <= 1.3e-13 of the largest gap sample, rounding the input to
float32 moves the result by 3e-8 .. 5e-8; the bound 1e-9 * max|gap| leaves four
orders of margin and still fails with any float32 step in the chain.  At the
reference size (condition number 9e5) solvers differ by 6e-11 .. 1.3e-10 and
float32 input moves the result by 8e-7: bound 1e-7 * max|gap|.
Measured on an MI355X (each test prints its figure): small shapes 2e-16 ..
6.6e-14 for the final gap and up to 4.0e-13 over the history, 4.2e-12 with
the gap at sample 0 (context on one side only), 1.2e-10 at the reference size,
4.8e-13 for the bundled clip.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import janssen_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")

# (w, h, p, maxit): p < h three times (one h no multiple of anything), p >= h, h = 1,
# an odd p (the lag sums pair the lags up)
SHAPES = [(256, 64, 32, 10), (192, 48, 16, 10), (512, 100, 64, 10), (96, 24, 40, 10),
          (128, 1, 24, 10), (80, 20, 33, 10)]


def _segment(w, h, seed):
    return R.sinusoid_mix(2 * w + h, noise=1e-3, seed=seed)


def _run(rows, p, maxit, stride=None, history=False):
    """rows: [(x, gap_start, gap_len)] -> (sol [n, stride] numpy, iters, history)."""
    from ainp import ops
    stride = stride or max(len(x) for x, _, _ in rows)
    batch = np.zeros((len(rows), stride))
    for i, (x, _, _) in enumerate(rows):
        batch[i, :len(x)] = x
    sol = torch.from_numpy(batch).cuda()
    iters, hist = ops.janssen(sol, [len(x) for x, _, _ in rows], [s for _, s, _ in rows],
                              [h for _, _, h in rows], p, maxit, return_history=history)
    torch.cuda.synchronize()
    return sol.cpu().numpy(), iters.cpu().numpy(), None if hist is None else hist.cpu().numpy()


def _rel(got, ref, s, h):
    return np.max(np.abs(got[s:s + h] - ref[s:s + h])) / np.max(np.abs(ref[s:s + h]))


@pytest.fixture(scope="module")
def refs():
    """The dense reference of every small shape, computed once."""
    out = {}
    for i, (w, h, p, maxit) in enumerate(SHAPES):
        x = _segment(w, h, seed=10 + i)
        out[(w, h, p, maxit)] = (x, R.janssen(x, w, h, p, maxit))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "w%d_h%d_p%d_it%d" % s)
def test_parity_small(shape, refs):
    w, h, p, maxit = shape
    x, (ref, ref_hist, ref_done) = refs[shape]
    xin = x.copy()
    xin[w:w + h] = np.nan                       # whatever the gap holds is ignored
    sol, iters, hist = _run([(xin, w, h)], p, maxit, history=True)
    assert ref_done == maxit and iters[0] == maxit
    d = _rel(sol[0], ref, w, h)
    dh = np.max(np.abs(hist[0, :, :h] - ref_hist)) / np.max(np.abs(ref[w:w + h]))
    print(f"janssen parity {shape}: final {d:.3e}, history {dh:.3e}")
    assert d <= 1e-9 and dh <= 1e-9
    obs = np.r_[0:w, w + h:2 * w + h]
    assert np.array_equal(sol[0][obs], x[obs])      # observed samples bit for bit
    assert np.array_equal(hist[0, -1, :h], sol[0, w:w + h])


def test_parity_mixed_batch(refs):
    """One launch over three shapes with a common p: n, gap_start and gap_len
    differ per row, stride > every n, and one gap sits off-centre."""
    p, maxit = 32, 10
    rows, want = [], []
    for i, (w, h) in enumerate(((256, 64), (192, 48), (512, 100))):
        x = _segment(w, h, seed=20 + i)
        s = w - 37 * i                           # 256, 155, 438
        rows.append((x, s, h))
        want.append(R.janssen(x, s, h, p, maxit)[0])
    sol, iters, _ = _run(rows, p, maxit, stride=1200)
    assert iters.tolist() == [maxit] * 3
    for (x, s, h), ref, got in zip(rows, want, sol):
        d = _rel(got, ref, s, h)
        print(f"janssen parity mixed n={len(x)} s={s} h={h}: {d:.3e}")
        assert d <= 1e-9
        obs = np.r_[0:s, s + h:len(x)]
        assert np.array_equal(got[obs], x[obs])
        assert np.all(got[len(x):] == 0)         # the padding of the row is not touched


def test_gap_at_segment_edges():
    """Clipped segments: the gap starts at sample 0 / ends at the last sample."""
    p, maxit, h = 16, 4, 20
    x = _segment(150, h, seed=31)[:200]
    rows = [(x, 0, h), (x, len(x) - h, h)]
    sol, iters, _ = _run(rows, p, maxit)
    assert iters.tolist() == [maxit, maxit]
    for (xx, s, hh), got in zip(rows, sol):
        ref = R.janssen(xx, s, hh, p, maxit)[0]
        d = _rel(got, ref, s, hh)
        print(f"janssen parity edge s={s}: {d:.3e}")
        assert d <= 1e-9


def test_parity_reference_size():
    """w = 4096, h = 1280, p = 512 (train.m's 80 ms gap at 16 kHz), maxit = 2."""
    w, h, p, maxit = 4096, 1280, 512, 2
    x = R.harmonic_signal(2 * w + h, seed=1)
    ref, _, done = R.janssen(x, w, h, p, maxit)
    sol, iters, _ = _run([(x, w, h)], p, maxit)
    assert done == maxit and iters[0] == maxit
    d = _rel(sol[0], ref, w, h)
    print(f"janssen parity reference size: {d:.3e}")
    assert d <= 1e-7
    obs = np.r_[0:w, w + h:2 * w + h]
    assert np.array_equal(sol[0][obs], x[obs])


def test_history_equals_fresh_runs_and_calls_repeat():
    w, h, p, maxit = 192, 48, 16, 5
    x = _segment(w, h, seed=41)
    sol, iters, hist = _run([(x, w, h)], p, maxit, history=True)
    sol2, iters2, hist2 = _run([(x, w, h)], p, maxit, history=True)
    assert np.array_equal(sol, sol2) and np.array_equal(hist, hist2)     # same bits
    assert iters[0] == iters2[0] == maxit
    for k in range(maxit):
        fresh, it, _ = _run([(x, w, h)], p, k + 1)
        assert it[0] == k + 1
        assert np.array_equal(hist[0, k, :h], fresh[0, w:w + h]), k


def test_silent_segment_and_its_neighbours():
    w, h, p, maxit = 192, 48, 16, 6
    x = _segment(w, h, seed=51)
    alone, _, _ = _run([(x, w, h)], p, maxit)
    silent = np.zeros(2 * w + h)
    sol, iters, hist = _run([(x, w, h), (silent, w, h), (x, w, h)], p, maxit, history=True)
    assert iters.tolist() == [maxit, 0, maxit]
    assert np.all(sol[1] == 0)
    assert np.all(np.isnan(hist[1]))             # no iteration completed, nothing recorded
    assert np.array_equal(sol[0], alone[0]) and np.array_equal(sol[2], alone[0])


def test_overflow_stops_the_segment():
    """Finite observed samples near 1e160: r[0] overflows, so the segment stops
    before its first iterate (the reference's lpc returns NaN there and chol
    breaks) -- 0 iterations, the gap stays zero, nothing is recorded, the
    observed samples and the batch neighbour are untouched.  (A stop after a
    completed iteration needs an overflow that only the filled gap causes; the
    gap adds about a ninth to r[0] while the recursion's own products already
    need a factor 4 of headroom, so no valid input reaches it reliably.)"""
    w, h, p, maxit = 192, 48, 16, 4
    base = _segment(w, h, seed=61)
    big = base * 1e160
    assert np.all(np.isfinite(big))
    alone, _, _ = _run([(base, w, h)], p, maxit)
    sol, iters, hist = _run([(big, w, h), (base, w, h)], p, maxit, history=True)
    assert iters.tolist() == [0, maxit]
    assert np.all(sol[0, w:w + h] == 0)
    obs = np.r_[0:w, w + h:2 * w + h]
    assert np.array_equal(sol[0][obs], big[obs])
    assert np.all(np.isnan(hist[0]))
    assert np.array_equal(sol[1], alone[0])
    assert np.array_equal(hist[1, -1, :h], alone[0, w:w + h])


def test_wrapper_refuses_bad_tables():
    from ainp import ops
    sol = torch.zeros(1, 300, dtype=torch.float64, device="cuda")
    for n, s, h in ((301, 10, 5), (300, 296, 5), (300, -1, 5), (300, 10, 0), (16, 2, 5)):
        with pytest.raises(ValueError):
            ops.janssen(sol, [n], [s], [h], 16, 3)
    with pytest.raises(TypeError):
        ops.janssen(sol.float(), [300], [10], [5], 16, 3)


def _load(name):
    import utils
    audio, sr = utils.load_audio(os.path.join(FLAC, name))
    return audio.astype(np.float64), sr


def test_janssen_inpaint_end_to_end():
    """One bundled clip, the 80 ms gap at 2.0 s, w = 1024, p = 128, maxit = 5."""
    from ainp.janssen import gap_sdr, janssen_inpaint
    audio, sr = _load("81-121543-0008.flac")
    s, h, w, p, maxit = int(2.0 * sr), int(0.08 * sr), 1024, 128, 5
    mask = np.ones(len(audio), bool)
    mask[s:s + h] = False
    out, info = janssen_inpaint(audio, mask, p=p, w=w, maxit=maxit, return_history=True)
    assert out.dtype == np.float64 and out.shape == audio.shape
    assert np.array_equal(out[mask], audio[mask])            # outside the gap: the input
    ref, ref_hist, _ = R.janssen(audio[s - w:s + h + w], w, h, p, maxit)
    d = np.max(np.abs(out[s:s + h] - ref[w:w + h])) / np.max(np.abs(ref[w:w + h]))
    print(f"janssen_inpaint end to end: {d:.3e}, gap SDR {gap_sdr(audio, out, mask):.2f} dB")
    assert d <= 1e-8
    assert len(info) == 1 and info[0]["iters"] == maxit
    assert (info[0]["start"], info[0]["end"]) == (s, s + h)
    assert np.array_equal(info[0]["history"][-1], out[s:s + h])
    # NaN-marked input and a torch tensor give the same bits
    marked = audio.copy()
    marked[~mask] = np.nan
    assert np.array_equal(janssen_inpaint(torch.from_numpy(marked), p=p, w=w, maxit=maxit), out)


def test_run_janssen_evaluation(tmp_path):
    from models import model_eval
    from models.AudioReg import gap_sdr, janssen_inpaint  # noqa: F401  (the re-exports)
    clips = ["81-121543-0008.flac", "1241-121103-0021.flac"]
    src = tmp_path / "in"
    src.mkdir()
    for c in clips:
        shutil.copy(os.path.join(FLAC, c), src / c)
    sdrs = model_eval.run_janssen_evaluation(str(src), str(tmp_path / "out"), p=64, w=512, maxit=3)
    assert sorted(sdrs) == sorted(clips)
    for c in clips:
        assert np.isfinite(sdrs[c]), (c, sdrs[c])
        out = tmp_path / "out" / (os.path.splitext(c)[0] + "_janssen_inpainted.flac")
        assert out.exists() and out.stat().st_size > 0
    print("run_janssen_evaluation gap SDRs:", sdrs)
