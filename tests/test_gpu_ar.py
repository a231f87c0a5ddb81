"""GPU tests of the Burg estimator inside Janssen and of the forward/backward
AR extrapolation (csrc/ar_fit.h, csrc/janssen.hip, csrc/ar_extrapolate.hip
through ops.janssen / ops.ar_extrapolate, ainp/janssen.py and
models/model_eval.run_ar_evaluation) against the float64 numpy references of
tests/ar_ref.py.

Bounds (those of test_gpu_janssen.py).  Small shapes, 1e-9 * max|gap|: float64
Burg references that differ only in summation order or accumulation width
differ by at most 8.0e-13 on these inputs, rounding the input to float32 moves
the result by 1.2e-8 .. 6.2e-8.  Reference size, 1e-7: float64 and long-double
Burg differ by 5.0e-14 there.  Extrapolation, 1e-9: reference against reference
gives <= 7e-16 ("lpc") and <= 4.8e-13 ("arburg").  Bundled clip, 1e-8: Burg
reference variants differ by 1.5e-13.
Burg's layout (csrc/ar_fit.h): lane t of 512 keeps elements 32 t .. 32 t + 31 of
the two error vectors, a wave 2048; the vectors of a segment of n samples have
n - 1 elements, so n = 2050 puts one element into the second wave, n = 2048
leaves the first wave one short, n = 34 / 32 do the same to a lane.
Every test prints its measured figure; DESIGN §14 records them.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import ar_ref as A
import janssen_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")

SHAPES = [(256, 64, 32, 10), (192, 48, 16, 10), (512, 100, 64, 10), (96, 24, 40, 10),
          (128, 1, 24, 10), (80, 20, 33, 10)]


def _segment(w, h, seed):
    return R.sinusoid_mix(2 * w + h, noise=1e-3, seed=seed)


def _batch(rows, stride=None):
    stride = stride or max(len(x) for x, _, _ in rows)
    batch = np.zeros((len(rows), stride))
    for i, (x, _, _) in enumerate(rows):
        batch[i, :len(x)] = x
    return torch.from_numpy(batch).cuda()


def _run(rows, p, maxit, stride=None, history=False, method="arburg"):
    """rows: [(x, gap_start, gap_len)] -> (sol [n, stride] numpy, iters, history)."""
    from ainp import ops
    sol = _batch(rows, stride)
    iters, hist = ops.janssen(sol, [len(x) for x, _, _ in rows], [s for _, s, _ in rows],
                              [h for _, _, h in rows], p, maxit, return_history=history,
                              method=method)
    torch.cuda.synchronize()
    return sol.cpu().numpy(), iters.cpu().numpy(), None if hist is None else hist.cpu().numpy()


def _extrapolate(rows, p, w, method, stride=None):
    from ainp import ops
    sol = _batch(rows, stride)
    status = ops.ar_extrapolate(sol, [len(x) for x, _, _ in rows], [s for _, s, _ in rows],
                                [h for _, _, h in rows], p, w, method=method)
    torch.cuda.synchronize()
    return sol.cpu().numpy(), status.cpu().numpy()


def _rel(got, ref, s, h):
    return np.max(np.abs(got[s:s + h] - ref[s:s + h])) / np.max(np.abs(ref[s:s + h]))


def _obs(n, s, h):
    return np.r_[0:s, s + h:n]


# ------------------------------------------------------------ Janssen + Burg
@pytest.fixture(scope="module")
def refs():
    """The dense reference of every small shape, computed once."""
    out = {}
    for i, (w, h, p, maxit) in enumerate(SHAPES):
        x = _segment(w, h, seed=10 + i)
        out[(w, h, p, maxit)] = (x, A.janssen(x, w, h, p, maxit))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "w%d_h%d_p%d_it%d" % s)
def test_burg_parity_small(shape, refs):
    w, h, p, maxit = shape
    x, (ref, ref_hist, ref_done) = refs[shape]
    xin = x.copy()
    xin[w:w + h] = np.nan                       # whatever the gap holds is ignored
    sol, iters, hist = _run([(xin, w, h)], p, maxit, history=True)
    assert ref_done == maxit and iters[0] == maxit
    d = _rel(sol[0], ref, w, h)
    dh = np.max(np.abs(hist[0, :, :h] - ref_hist)) / np.max(np.abs(ref[w:w + h]))
    print(f"janssen+burg parity {shape}: final {d:.3e}, history {dh:.3e}")
    assert d <= 1e-9 and dh <= 1e-9
    obs = _obs(len(x), w, h)
    assert np.array_equal(sol[0][obs], x[obs])      # observed samples bit for bit
    assert np.array_equal(hist[0, -1, :h], sol[0, w:w + h])


# (n, s, h, p, maxit): one element in the second wave / the first wave one
# short; the same for a lane; error vectors that shrink to length 2; the gap at
# sample 0 and at the last sample
EDGES = [(2050, 1000, 30, 16, 3), (2048, 1000, 30, 16, 3), (34, 12, 4, 8, 3), (32, 12, 4, 8, 3),
         (42, 10, 4, 40, 3), (200, 0, 20, 16, 4), (200, 180, 20, 16, 4)]


@pytest.mark.parametrize("edge", EDGES, ids=lambda e: "n%d_s%d_h%d_p%d_it%d" % e)
def test_burg_edge_shapes(edge):
    n, s, h, p, maxit = edge
    x = R.sinusoid_mix(n, noise=1e-3, seed=70 + n % 7)
    ref, _, done = A.janssen(x, s, h, p, maxit)
    sol, iters, _ = _run([(x, s, h)], p, maxit)
    assert done == maxit and iters[0] == maxit
    d = _rel(sol[0], ref, s, h)
    print(f"janssen+burg edge {edge}: {d:.3e}")
    assert d <= 1e-9
    assert np.array_equal(sol[0][_obs(n, s, h)], x[_obs(n, s, h)])


def test_burg_mixed_batch():
    """One launch over three n / gap_start / gap_len, stride > every n."""
    p, maxit = 32, 10
    rows, want = [], []
    for i, (w, h) in enumerate(((256, 64), (192, 48), (512, 100))):
        x = _segment(w, h, seed=20 + i)
        s = w - 37 * i
        rows.append((x, s, h))
        want.append(A.janssen(x, s, h, p, maxit)[0])
    sol, iters, _ = _run(rows, p, maxit, stride=1200)
    assert iters.tolist() == [maxit] * 3
    for (x, s, h), ref, got in zip(rows, want, sol):
        d = _rel(got, ref, s, h)
        print(f"janssen+burg mixed n={len(x)} s={s} h={h}: {d:.3e}")
        assert d <= 1e-9
        assert np.array_equal(got[_obs(len(x), s, h)], x[_obs(len(x), s, h)])
        assert np.all(got[len(x):] == 0)         # the padding of the row is not touched


def test_burg_full_register_range():
    """n = 16384: every lane's 32 elements of both vectors are in use."""
    n, s, h, p, maxit = 16384, 8000, 16, 8, 2
    x = R.sinusoid_mix(n, noise=1e-3, seed=81)
    ref, _, done = A.janssen(x, s, h, p, maxit)
    sol, iters, _ = _run([(x, s, h)], p, maxit)
    assert done == maxit and iters[0] == maxit
    d = _rel(sol[0], ref, s, h)
    print(f"janssen+burg n = 16384: {d:.3e}")
    assert d <= 1e-9
    assert np.array_equal(sol[0][_obs(n, s, h)], x[_obs(n, s, h)])


def test_burg_parity_reference_size():
    """w = 4096, h = 1280, p = 512 (train.m's 80 ms gap at 16 kHz), maxit = 2."""
    w, h, p, maxit = 4096, 1280, 512, 2
    x = _segment(w, h, seed=1)
    ref, _, done = A.janssen(x, w, h, p, maxit)
    sol, iters, _ = _run([(x, w, h)], p, maxit)
    assert done == maxit and iters[0] == maxit
    d = _rel(sol[0], ref, w, h)
    print(f"janssen+burg reference size: {d:.3e}")
    assert d <= 1e-7
    assert np.array_equal(sol[0][_obs(len(x), w, h)], x[_obs(len(x), w, h)])


def test_burg_history_equals_fresh_runs_and_calls_repeat():
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


def test_burg_silent_segment_and_its_neighbours():
    w, h, p, maxit = 192, 48, 16, 6
    x = _segment(w, h, seed=51)
    alone, _, _ = _run([(x, w, h)], p, maxit)
    silent = np.zeros(2 * w + h)
    sol, iters, hist = _run([(x, w, h), (silent, w, h), (x, w, h)], p, maxit, history=True)
    assert iters.tolist() == [maxit, 0, maxit]
    assert np.all(sol[1] == 0)
    assert np.all(np.isnan(hist[1]))             # no iteration completed, nothing recorded
    assert np.array_equal(sol[0], alone[0]) and np.array_equal(sol[2], alone[0])


def test_positional_op_call_is_still_lpc():
    """torch.ops.ainp.janssen with the nine arguments it had runs "lpc"."""
    from ainp import ops
    w, h, p, maxit = 192, 48, 16, 4
    x = _segment(w, h, seed=61)
    want, iters, _ = _run([(x, w, h)], p, maxit, method="lpc")
    sol = _batch([(x, w, h)])
    tabs = [torch.tensor([v], dtype=torch.int32, device="cuda") for v in (len(x), w, h)]
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.ops.ainp.janssen(sol, *tabs, p, maxit, None, done, None)
    torch.cuda.synchronize()
    assert done.item() == maxit == iters[0]
    assert np.array_equal(sol.cpu().numpy(), want)
    burg, _, _ = _run([(x, w, h)], p, maxit, method="ArBurg")      # case-insensitive
    assert not np.array_equal(burg, want)
    with pytest.raises(ValueError, match="method"):
        ops.janssen(sol, [len(x)], [w], [h], p, maxit, method="yule")


# ------------------------------------------------------------- extrapolation
# (pre, post, h, p, w): plain; w cuts the contexts; unequal and barely long
# enough contexts with an odd p; h = 1 (pure postdiction); h > p, no multiple of 64
XSHAPES = [(256, 256, 64, 32, 4096), (256, 256, 64, 32, 64), (40, 200, 16, 32, 4096),
           (200, 34, 16, 33, 4096), (128, 128, 1, 24, 4096), (96, 96, 100, 40, 4096)]


@pytest.fixture(scope="module")
def xsignals():
    return {sh: R.sinusoid_mix(sh[0] + sh[1] + sh[2], noise=1e-3, seed=100 + i)
            for i, sh in enumerate(XSHAPES)}


@pytest.mark.parametrize("method", ["lpc", "arburg"])
@pytest.mark.parametrize("shape", XSHAPES, ids=lambda s: "pre%d_post%d_h%d_p%d_w%d" % s)
def test_extrapolation_parity(shape, method, xsignals):
    pre, post, h, p, w = shape
    x = xsignals[shape]
    ref, ref_status = A.extrapolate(x, pre, h, p, w, method)
    xin = x.copy()
    xin[pre:pre + h] = np.nan                   # whatever the gap holds is ignored
    sol, status = _extrapolate([(xin, pre, h)], p, w, method)
    d = _rel(sol[0], ref, pre, h)
    print(f"extrapolation parity {shape} {method}: {d:.3e}")
    assert status[0] == ref_status == 1
    assert d <= 1e-9
    obs = _obs(len(x), pre, h)
    assert np.array_equal(sol[0][obs], x[obs])      # observed samples bit for bit
    sol2, _ = _extrapolate([(xin, pre, h)], p, w, method)
    assert np.array_equal(sol, sol2)                # two calls, the same bits


@pytest.mark.parametrize("method", ["lpc", "arburg"])
def test_extrapolation_mixed_batch(method):
    p, w = 32, 300
    rows = []
    for i, (pre, post, h) in enumerate(((256, 256, 64), (120, 400, 48), (512, 90, 100))):
        rows.append((R.sinusoid_mix(pre + post + h, noise=1e-3, seed=120 + i), pre, h))
    sol, status = _extrapolate(rows, p, w, method, stride=1200)
    assert status.tolist() == [1, 1, 1]
    for (x, s, h), got in zip(rows, sol):
        ref, _ = A.extrapolate(x, s, h, p, w, method)
        d = _rel(got, ref, s, h)
        print(f"extrapolation mixed n={len(x)} s={s} h={h} {method}: {d:.3e}")
        assert d <= 1e-9
        assert np.array_equal(got[_obs(len(x), s, h)], x[_obs(len(x), s, h)])
        assert np.all(got[len(x):] == 0)


@pytest.mark.parametrize("method", ["lpc", "arburg"])
def test_extrapolation_constant_context(method):
    """A constant pre-context predicts its mean: status 0, the segment is still
    filled, and its neighbour in the batch is unaffected."""
    pre, post, h, p, w = 100, 200, 10, 16, 4096
    x = R.sinusoid_mix(pre + post + h, noise=1e-3, seed=130)
    flat = x.copy()
    flat[:pre] = 0.25
    ref, ref_status = A.extrapolate(flat, pre, h, p, w, method)
    sol, status = _extrapolate([(flat, pre, h), (x, pre, h)], p, w, method)
    alone, _ = _extrapolate([(x, pre, h)], p, w, method)
    assert ref_status == 0 and status.tolist() == [0, 1]
    d = _rel(sol[0], ref, pre, h)
    print(f"extrapolation constant context {method}: {d:.3e}")
    assert d <= 1e-9
    assert sol[0, pre] == 0.25                  # weight 1 at the first sample: the mean
    assert np.array_equal(sol[1], alone[0])
    assert np.array_equal(sol[0][_obs(len(x), pre, h)], flat[_obs(len(x), pre, h)])


def test_extrapolation_wrapper_refuses_bad_tables():
    from ainp import ops
    sol = torch.zeros(1, 300, dtype=torch.float64, device="cuda")
    # beyond the stride, outside the segment, h = 0, pre-context 16 = p, post-context 15
    for n, s, h in ((301, 100, 5), (300, 296, 5), (300, 100, 0), (300, 16, 5), (300, 280, 5)):
        with pytest.raises(ValueError):
            ops.ar_extrapolate(sol, [n], [s], [h], 16, 4096)
    with pytest.raises(ValueError):
        ops.ar_extrapolate(sol, [300], [100], [5], 16, 10)          # w cuts both to 10 <= p
    with pytest.raises(TypeError):
        ops.ar_extrapolate(sol.float(), [300], [100], [5], 16, 4096)


# ---------------------------------------------------------------- end to end
def _load(name):
    import utils
    audio, sr = utils.load_audio(os.path.join(FLAC, name))
    return audio.astype(np.float64), sr


@pytest.fixture(scope="module")
def clip():
    audio, sr = _load("81-121543-0008.flac")
    s, h = int(2.0 * sr), int(0.08 * sr)
    mask = np.ones(len(audio), bool)
    mask[s:s + h] = False
    return audio, mask, s, h


def test_janssen_inpaint_arburg_end_to_end(clip):
    """The bundled clip, the 80 ms gap at 2.0 s, p = 512, w = 4096, maxit = 2."""
    from ainp.janssen import janssen_inpaint
    audio, mask, s, h = clip
    w, p, maxit = 4096, 512, 2
    out, info = janssen_inpaint(audio, mask, p=p, w=w, maxit=maxit, return_history=True,
                                method="arburg")
    ref, _, done = A.janssen(audio[s - w:s + h + w], w, h, p, maxit)
    d = np.max(np.abs(out[s:s + h] - ref[w:w + h])) / np.max(np.abs(ref[w:w + h]))
    print(f"janssen_inpaint arburg end to end: {d:.3e}")
    assert done == maxit and info[0]["iters"] == maxit
    assert d <= 1e-8
    assert np.array_equal(out[mask], audio[mask])


@pytest.mark.parametrize("method", ["lpc", "arburg"])
def test_ar_extrapolate_end_to_end(clip, method):
    from ainp.janssen import ar_extrapolate, gap_sdr
    audio, mask, s, h = clip
    w, p = 4096, 512
    out, info = ar_extrapolate(audio, mask, p=p, w=w, method=method, return_status=True)
    ref, _ = A.extrapolate(audio[s - w:s + h + w], w, h, p, w, method)
    d = np.max(np.abs(out[s:s + h] - ref[w:w + h])) / np.max(np.abs(ref[w:w + h]))
    print(f"ar_extrapolate {method} end to end: {d:.3e}, gap SDR {gap_sdr(audio, out, mask):.2f} dB")
    assert d <= 1e-8
    assert out.dtype == np.float64 and np.array_equal(out[mask], audio[mask])
    assert len(info) == 1 and info[0]["status"] == 1
    assert (info[0]["start"], info[0]["end"]) == (s, s + h)
    marked = audio.copy()
    marked[~mask] = np.nan                      # NaN-marked torch input: the same bits
    assert np.array_equal(ar_extrapolate(torch.from_numpy(marked), p=p, w=w, method=method), out)


def test_run_ar_evaluation(tmp_path):
    import utils
    from models import model_eval
    from models.AudioReg import ar_extrapolate, gap_sdr, janssen_inpaint
    clips = ["81-121543-0008.flac", "1241-121103-0021.flac"]
    src = tmp_path / "in"
    src.mkdir()
    for c in clips:
        shutil.copy(os.path.join(FLAC, c), src / c)
    p, w, maxit = 64, 512, 3
    for algorithm, method, suffix in (("janssen", "lpc", "janssen"),
                                      ("janssen", "arburg", "janssen_arburg"),
                                      ("extrapolation", "lpc", "extrapolation"),
                                      ("extrapolation", "arburg", "extrapolation_arburg")):
        sdrs = model_eval.run_ar_evaluation(str(src), str(tmp_path / "out"), algorithm=algorithm,
                                            method=method, p=p, w=w, maxit=maxit)
        assert sorted(sdrs) == sorted(clips)
        for c in clips:
            audio, sr = _load(c)
            s, h = int(2.0 * sr), int(0.08 * sr)
            mask = np.ones(len(audio), bool)
            mask[s:s + h] = False
            if algorithm == "janssen":
                want = janssen_inpaint(audio, mask, p=p, w=w, maxit=maxit, method=method)
            else:
                want = ar_extrapolate(audio, mask, p=p, w=w, method=method)
            assert sdrs[c] == gap_sdr(audio, want, mask), (algorithm, method, c)
            out = tmp_path / "out" / f"{os.path.splitext(c)[0]}_{suffix}_inpainted.flac"
            assert out.exists()
            written, wsr = utils.load_audio(str(out))
            assert wsr == sr and len(written) == len(audio)
        print(f"run_ar_evaluation {algorithm} {method} gap SDRs:", sdrs)
