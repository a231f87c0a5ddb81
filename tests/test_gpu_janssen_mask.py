"""GPU tests of Janssen inpainting for any mask (csrc/janssen_mask.hip through
ops.janssen_mask, ainp/janssen.py::janssen_inpaint_mask and
models/model_eval.run_janssen_mask_evaluation) against the dense float64
reference tests/janssen_mask_ref.py.

Bounds.  The rows of CASES (sinusoid_mix, noise 1e-3, maxit = 10) all complete
their 10 iterations in the reference; condition numbers 1e0 .. 1.1e3, 7.6e4
with the runs at both ends of the row.  Solving the reference's systems by LU
instead of Cholesky moves the result by 0 .. 1.5e-14 of the largest missing
sample (7.0e-12 with the runs at both ends); rounding the input to float32
moves it by 7.1e-9 .. 5.0e-7.  The project's bound for the gap-wise kernel,
1e-9 * max|missing|, on the final iterate and on the whole history, therefore
sits >= 140 times above the solver spread and >= 7 times below the float32
shift for every row (far_runs has the smallest shift, 7.1e-9; every other row
>= 17 times).  At the reference size (two 40 ms gaps 30 ms apart, p = 512,
condition 3.5e5) the solver spread is 3.2e-11 and the float32 shift 9.2e-8:
bound 1e-8 * max|missing| (the 1e-7 of the one-gap test would let a float32
step through at this shape).
Measured on an MI355X (each test prints its figure): the rows of CASES 1.7e-15
.. 2.4e-14 for the final iterate and up to 1.1e-13 over the history ("arburg"
up to 3.9e-13), 5.3e-12 / 1.9e-11 with the runs at both ends (53 times inside
the bound), 2.0e-14 .. 3.4e-13 against the one-run kernel, 4.4e-11 at the
reference size, 2.5e-13 / 6.5e-13 through janssen_inpaint_mask (45.5 and
51.2 dB).
"""
import os
import shutil

import numpy as np
import pytest
import torch

import ar_ref
import janssen_mask_ref as R
from test_gpu_janssen import SHAPES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")
MAXIT = 10


def _scatter(lo, hi, count, seed):
    return np.sort(np.random.default_rng(seed).choice(np.arange(lo, hi), count, replace=False))


# name: (n, missing, p, seed of the signal)
CASES = {
    "one_sample": (300, np.array([150]), 24, 101),
    "coupled_runs": (600, R.runs((200, 240), (255, 272)), 32, 102),
    "far_runs": (700, R.runs((200, 233), (420, 451)), 32, 103),
    "runs_15_16_17": (700, R.runs((100, 115), (300, 316), (500, 517)), 40, 104),
    "every_7th": (640, np.arange(160, 480, 7), 33, 105),
    "both_ends": (400, R.runs((0, 20), (380, 400)), 16, 106),
    "scattered_100": (512, _scatter(64, 448, 100, 7), 48, 107),
    "dense_block": (256, R.runs((100, 110), (120, 131), (140, 141)), 64, 108),
    "scattered_300": (2048, _scatter(256, 1792, 300, 8), 128, 109),
}
BURG_CASES = ("coupled_runs", "runs_15_16_17", "scattered_100")


def _signal(name):
    n, miss, p, seed = CASES[name]
    return R.sinusoid_mix(n, noise=1e-3, seed=seed), miss, p


def _run(rows, p, maxit, stride=None, history=False, method="lpc"):
    """rows: [(x, missing)] -> (sol [n, stride] numpy, iters, history)."""
    from ainp import ops
    stride = stride or max(len(x) for x, _ in rows)
    batch = np.zeros((len(rows), stride))
    for i, (x, _) in enumerate(rows):
        batch[i, :len(x)] = x
    sol = torch.from_numpy(batch).cuda()
    iters, hist = ops.janssen_mask(sol, [len(x) for x, _ in rows], [m for _, m in rows], p, maxit,
                                   return_history=history, method=method)
    torch.cuda.synchronize()
    return sol.cpu().numpy(), iters.cpu().numpy(), None if hist is None else hist.cpu().numpy()


@pytest.fixture(scope="module")
def refs():
    """The dense reference of every row of CASES ("lpc"), computed once."""
    out = {}
    for name in CASES:
        x, miss, p = _signal(name)
        out[name] = R.janssen(x, miss, p, MAXIT)
    return out


def _check(name, method, ref, ref_hist, ref_done):
    x, miss, p = _signal(name)
    xin = x.copy()
    xin[miss] = np.nan                          # whatever the missing samples hold is ignored
    sol, iters, hist = _run([(xin, miss)], p, MAXIT, history=True, method=method)
    assert ref_done == MAXIT and iters[0] == MAXIT
    top = np.max(np.abs(ref[miss]))
    d = np.max(np.abs(sol[0][miss] - ref[miss])) / top
    dh = np.max(np.abs(hist[0, :, :len(miss)] - ref_hist)) / top
    print(f"janssen_mask parity {name} {method}: final {d:.3e}, history {dh:.3e}")
    assert d <= 1e-9 and dh <= 1e-9
    obs = np.setdiff1d(np.arange(len(x)), miss)
    assert np.array_equal(sol[0][obs], x[obs])      # observed samples bit for bit
    assert np.array_equal(hist[0, -1, :len(miss)], sol[0][miss])


@pytest.mark.parametrize("name", list(CASES))
def test_parity(name, refs):
    _check(name, "lpc", *refs[name])


@pytest.mark.parametrize("name", BURG_CASES)
def test_parity_burg(name):
    x, miss, p = _signal(name)
    _check(name, "arburg", *R.janssen(x, miss, p, MAXIT, fit=ar_ref.arburg))


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "w%d_h%d_p%d_it%d" % s)
def test_agrees_with_the_single_run_kernel(shape):
    """One run per row: the Cholesky path and ops.janssen's Toeplitz recursion
    solve the same systems (not to the bit: the solvers differ)."""
    from ainp import ops
    w, h, p, maxit = shape
    x = R.sinusoid_mix(2 * w + h, noise=1e-3, seed=10 + SHAPES.index(shape))
    sol, iters, _ = _run([(x, np.arange(w, w + h))], p, maxit)
    one = torch.from_numpy(x[None].copy()).cuda()
    it1, _ = ops.janssen(one, [len(x)], [w], [h], p, maxit)
    one = one.cpu().numpy()
    assert iters[0] == maxit and int(it1[0]) == maxit
    d = np.max(np.abs(sol[0] - one[0])) / np.max(np.abs(one[0, w:w + h]))
    print(f"janssen_mask vs janssen {shape}: {d:.3e}")
    assert d <= 1e-9


def test_mixed_batch():
    """One launch: rows of different n and h (1, 48, 100), stride > every n, one
    empty list (0 iterations, untouched) and -- straight through the torch op,
    past the host check -- one descending list (-1, untouched)."""
    from ainp import _lib
    p, maxit, stride = 24, MAXIT, 700
    x1 = R.sinusoid_mix(300, noise=1e-3, seed=101)
    x48 = R.sinusoid_mix(420, noise=1e-3, seed=121)
    x100 = R.sinusoid_mix(512, noise=1e-3, seed=107)
    m48 = R.runs((150, 180), (190, 208))
    m100 = CASES["scattered_100"][1]
    rows = [(x1, np.array([150])), (x48, m48), (x100, m100), (x48, np.zeros(0, np.int64)),
            (x48, np.array([200, 199, 150]))]
    batch = np.full((len(rows), stride), 7.0)    # the padding is not zero: it must stay
    for i, (x, _) in enumerate(rows):
        batch[i, :len(x)] = x
    before = batch.copy()
    sol = torch.from_numpy(batch).cuda()
    lists = [m for _, m in rows]
    off = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int32)
    idx = np.concatenate(lists).astype(np.int32)
    n = np.array([len(x) for x, _ in rows], np.int32)
    ws = torch.empty(_lib.lib.ainp_janssen_mask_workspace(len(rows), stride, p, 100, 0),
                     dtype=torch.uint8, device="cuda")
    iters = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
    torch.ops.ainp.janssen_mask(sol, torch.from_numpy(n).cuda(), torch.from_numpy(off).cuda(),
                                torch.from_numpy(idx).cuda(), 100, p, maxit, 0, None, iters, ws)
    torch.cuda.synchronize()
    sol = sol.cpu().numpy()
    assert iters.cpu().tolist() == [maxit, maxit, maxit, 0, -1]
    assert np.array_equal(sol[3], before[3]) and np.array_equal(sol[4], before[4])
    for r, (x, miss) in enumerate(rows[:3]):
        ref = R.janssen(x, miss, p, maxit)[0]
        d = np.max(np.abs(sol[r][miss] - ref[miss])) / np.max(np.abs(ref[miss]))
        print(f"janssen_mask mixed n={len(x)} h={len(miss)}: {d:.3e}")
        assert d <= 1e-9
        obs = np.setdiff1d(np.arange(stride), miss)
        assert np.array_equal(sol[r][obs], before[r][obs])   # observed samples and padding


def test_history_equals_fresh_runs_and_calls_repeat():
    x, miss, p = _signal("coupled_runs")
    maxit = 5
    sol, iters, hist = _run([(x, miss)], p, maxit, history=True)
    sol2, iters2, hist2 = _run([(x, miss)], p, maxit, history=True)
    assert np.array_equal(sol, sol2) and np.array_equal(hist, hist2)     # same bits
    assert iters[0] == iters2[0] == maxit
    for k in range(maxit):
        fresh, it, _ = _run([(x, miss)], p, k + 1)
        assert it[0] == k + 1
        assert np.array_equal(hist[0, k], fresh[0][miss]), k


def test_silent_and_overflow_rows_between_good_ones():
    x, miss, p = _signal("coupled_runs")
    maxit = 6
    alone, _, alone_hist = _run([(x, miss)], p, maxit, history=True)
    big = x * 1e160
    assert np.all(np.isfinite(big))
    sol, iters, hist = _run([(x, miss), (np.zeros(len(x)), miss), (x, miss), (big, miss),
                             (x, miss)], p, maxit, history=True)
    assert iters.tolist() == [maxit, 0, maxit, 0, maxit]
    assert np.all(sol[1] == 0) and np.all(sol[3][miss] == 0)
    obs = np.setdiff1d(np.arange(len(x)), miss)
    assert np.array_equal(sol[3][obs], big[obs])
    assert np.all(np.isnan(hist[1])) and np.all(np.isnan(hist[3]))
    for r in (0, 2, 4):
        assert np.array_equal(sol[r], alone[0]) and np.array_equal(hist[r], alone_hist[0])


def test_parity_reference_size():
    """Two 40 ms gaps 30 ms apart at 16 kHz, w = 4096, p = 512, maxit = 2."""
    p, maxit = 512, 2
    x = R.harmonic_signal(9952, seed=1)
    miss = R.runs((4096, 4736), (5216, 5856))
    ref, _, done = R.janssen(x, miss, p, maxit)
    sol, iters, _ = _run([(x, miss)], p, maxit)
    assert done == maxit and iters[0] == maxit
    d = np.max(np.abs(sol[0][miss] - ref[miss])) / np.max(np.abs(ref[miss]))
    print(f"janssen_mask parity reference size: {d:.3e}")
    assert d <= 1e-8
    obs = np.setdiff1d(np.arange(len(x)), miss)
    assert np.array_equal(sol[0][obs], x[obs])


def test_wrapper_refuses_bad_tables():
    from ainp import ops
    sol = torch.zeros(1, 300, dtype=torch.float64, device="cuda")
    for n, miss in ((301, [10]), (300, [300]), (300, [-1, 4]), (300, [5, 5]), (300, [9, 8]),
                    (16, [2])):
        with pytest.raises(ValueError):
            ops.janssen_mask(sol, [n], [miss], 16, 3)
    with pytest.raises(ValueError):
        ops.janssen_mask(sol, [300], [[1], [2]], 16, 3)
    with pytest.raises(TypeError):
        ops.janssen_mask(sol.float(), [300], [[10]], 16, 3)


def _mask(n, *gaps):
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


def test_inpaint_mask_equals_janssen_inpaint_bit_for_bit():
    """Well-separated gaps, two signals: both take the one-run launch."""
    from ainp.janssen import janssen_inpaint, janssen_inpaint_mask
    sigs = [R.sinusoid_mix(2400, noise=1e-3, seed=131), R.sinusoid_mix(1500, noise=1e-3, seed=132)]
    masks = [_mask(2400, (400, 440), (1500, 1530)), _mask(1500, (20, 50))]
    kw = dict(p=24, w=300, maxit=6)
    a, ia = janssen_inpaint(sigs, masks, return_history=True, **kw)
    b, ib = janssen_inpaint_mask(sigs, masks, return_history=True, **kw)
    for method in ("lpc", "arburg"):
        a2 = janssen_inpaint(sigs, masks, method=method, **kw)
        b2 = janssen_inpaint_mask(sigs, masks, method=method, **kw)
        assert all(np.array_equal(u, v) for u, v in zip(a2, b2)), method
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert len(ia) == len(ib) == 3
    for da, db in zip(ia, ib):
        assert (da["signal"], da["start"], da["end"], da["iters"]) == \
            (db["signal"], db["start"], db["end"], db["iters"])
        assert np.array_equal(da["history"], db["history"])


def test_inpaint_mask_merged_clusters():
    """A coupled pair (15 samples apart) plus a separate gap in one signal."""
    from ainp.janssen import janssen_inpaint_mask, plan_mask_segments
    p, w, maxit = 32, 300, MAXIT
    clean = R.sinusoid_mix(3000, noise=1e-3, seed=141)
    mask = _mask(3000, (500, 540), (555, 572), (2000, 2030))
    marked = clean.copy()
    marked[~mask] = np.nan
    out, info = janssen_inpaint_mask(marked, p=p, w=w, maxit=maxit, return_history=True)
    assert out.dtype == np.float64 and out.shape == clean.shape
    assert np.array_equal(out[mask], clean[mask])
    plan = plan_mask_segments([mask], w, p)
    assert plan.runs.tolist() == [2, 1] and len(info) == 2
    for r, d in enumerate(info):
        assert sorted(d) == ["end", "history", "iters", "missing", "signal", "start"]
        lo, n, miss = int(plan.lo[r]), int(plan.n[r]), plan.missing[r]
        ref, ref_hist, done = R.janssen(clean[lo:lo + n], miss, p, maxit)
        assert d["iters"] == done == maxit and d["signal"] == 0
        assert np.array_equal(d["missing"], lo + miss)
        assert (d["start"], d["end"]) == (lo + miss[0], lo + miss[-1] + 1)
        top = np.max(np.abs(ref[miss]))
        e = np.max(np.abs(out[lo + miss] - ref[miss])) / top
        eh = np.max(np.abs(d["history"] - ref_hist)) / top
        sdr = R.set_sdr(clean, out, lo + miss)
        print(f"janssen_inpaint_mask cluster {r}: final {e:.3e}, history {eh:.3e}, "
              f"SDR {sdr:.2f} dB")
        assert d["history"].shape == (maxit, len(miss))
        assert e <= 1e-9 and eh <= 1e-9
        assert sdr > 40.0


def test_run_janssen_mask_evaluation(tmp_path):
    from models import model_eval
    from models.AudioReg import janssen_inpaint_mask, plan_mask_segments  # noqa: F401
    clips = ["81-121543-0008.flac", "1241-121103-0021.flac"]
    src = tmp_path / "in"
    src.mkdir()
    for c in clips:
        shutil.copy(os.path.join(FLAC, c), src / c)
    kw = dict(p=64, w=512, maxit=3)
    want = model_eval.run_janssen_evaluation(str(src), str(tmp_path / "one"), **kw)
    got = model_eval.run_janssen_mask_evaluation(str(src), str(tmp_path / "mask"), **kw)
    assert got == want                       # the default gap: the same figures exactly
    two = model_eval.run_janssen_mask_evaluation(str(src), str(tmp_path / "two"),
                                                 gaps=((2.0, 0.04), (2.06, 0.04)), **kw)
    assert sorted(two) == sorted(clips)
    for c in clips:
        assert np.isfinite(two[c]), (c, two[c])
        out = tmp_path / "two" / (os.path.splitext(c)[0] + "_janssen_mask_inpainted.flac")
        assert out.exists() and out.stat().st_size > 0
    print("run_janssen_mask_evaluation SDRs:", got, two)
