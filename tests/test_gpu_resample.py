"""GPU parity of the polyphase resampler (csrc/resample.hip) and of what is
built on it (ops.resample_poly, utils.resample_audio, utils.load_audio_batch,
model_eval.export_48k_pairs) against the float64 closed form of
tests/resample_ref.py, element by element.

Bound, with u = 2**-24 (float32) or 2**-53 (float64), tpp = taps per phase and
S[m] = sum_i |x[i]| |h[...]|:

    |y[m] - ref[m]| <= (tpp + 3) u S[m]

tpp products summed by fma in any order, one u for the coefficient's rounding
to the element type, two of slack.  A wrong tap, phase or edge is off by
O(|x|).  Tile boundaries come from the host plan, not from constants.
"""
import functools
import os
import wave

import numpy as np
import pytest
import torch

import resample_ref
from ainp import _lib, ops
from ainp import resample as rs

pytestmark = pytest.mark.gpu

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
TDT = {"float32": torch.float32, "float64": torch.float64}
RATIOS = [(3, 1), (1, 3), (2, 1), (160, 441), (441, 160), (5, 7)]


def _n_for_outputs(n_out, up, down):
    """The smallest n_in with ceil(n_in up / down) >= n_out."""
    n = -(-(n_out * down) // up)
    while resample_ref.out_len(n, up, down) < n_out:
        n += 1
    while n > 1 and resample_ref.out_len(n - 1, up, down) >= n_out:
        n -= 1
    return n


def _lengths(up, down, dtype):
    p = rs.plan(up, down, dtype)
    one_tile = _n_for_outputs(p.tile, p.up, p.down)
    out = {
        "one": 1,
        "two": 2,
        "both_edges": max(3, p.half // p.up - 1),           # shorter than half / up
        "tile_minus": one_tile - 1,
        "tile": one_tile,                                   # the first tile exactly full
        "tile_plus": one_tile + 1,
        "three_tiles_tail": _n_for_outputs(3 * p.tile + p.tile // 3 + 1, p.up, p.down),
        "divisible": 3 * p.down,                            # n up divisible by down
    }
    if p.down > 1:
        out["not_divisible"] = 3 * p.down + 1
    assert out["both_edges"] < p.half / p.up
    if p.up <= p.down:       # downsampling reaches every output count: exactly one tile
        assert resample_ref.out_len(one_tile, up, down) == p.tile
    assert resample_ref.out_len(one_tile - 1, up, down) < p.tile
    assert resample_ref.out_len(out["three_tiles_tail"], up, down) > 3 * p.tile
    return out


def _signal(n, dtype, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.5 * np.sin(0.031 * t + 0.3) + 0.25 * rng.standard_normal(n)
    return x.astype(dtype)


@functools.lru_cache(maxsize=None)
def _case(up, down, n, dtype, seed=0):
    """(x in the element type, float64 reference, bound); computed once, read-only."""
    x = _signal(n, dtype, seed + 7919 * n + up)
    ref = resample_ref.resample(x, up, down)
    bound = (resample_ref.taps_per_phase(up, down) + 3) * U[dtype] * resample_ref.abs_sum(
        x, up, down)
    for a in (x, ref, bound):
        a.setflags(write=False)
    return x, ref, bound


def _check(y, ref, bound, what):
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    y = np.asarray(y, dtype=np.float64)
    assert np.all(np.isfinite(y)), what
    err = np.abs(y - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"{what}: max err / bound {worst:.3f}")
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (what, bad[:5], err[bad[:5]], bound[bad[:5]])


# ----------------------------------------------------------- single signals
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_matches_the_closed_form(up, down, dtype):
    for name, n in _lengths(up, down, dtype).items():
        x, ref, bound = _case(up, down, n, dtype)
        y = ops.resample_poly(torch.from_numpy(np.array(x)).cuda(), up, down)
        assert y.dtype == TDT[dtype] and y.is_cuda
        _check(y.cpu().numpy(), ref, bound, f"({up},{down}) {dtype} {name} n={n}")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_common_factor_changes_no_bit(dtype):
    n = _lengths(3, 1, dtype)["three_tiles_tail"]
    x = torch.from_numpy(np.array(_case(3, 1, n, dtype)[0])).cuda()
    assert torch.equal(ops.resample_poly(x, 6, 2), ops.resample_poly(x, 3, 1))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_unit_ratio_is_an_exact_copy(dtype):
    assert rs.plan(4, 4, dtype).route == rs.RS_COPY
    for n in (1, 2, 255, 2049, 5000):
        x = torch.from_numpy(_signal(n, dtype, 5)).cuda()
        assert torch.equal(ops.resample_poly(x, 4, 4), x)
    # with the zero fill and the truncation of every other ratio
    x = torch.from_numpy(_signal(24, dtype, 6).reshape(2, 12)).cuda()
    x[1, 5:] = float("nan")
    y = ops.resample_poly(x, 4, 4, n=[12, 5], out_len=15)
    assert torch.equal(y[0, :12], x[0]) and torch.equal(y[1, :5], x[1, :5])
    assert not y[0, 12:].any() and not y[1, 5:].any()
    assert torch.equal(ops.resample_poly(x, 4, 4, n=[12, 5], out_len=4), x[:, :4])


# ------------------------------------------------------------- ragged batch
@pytest.mark.parametrize("up,down,dtype", [(3, 1, "float64"), (160, 441, "float32"),
                                           (5, 7, "float32"), (1, 3, "float64")])
def test_ragged_batch(up, down, dtype):
    ln = _lengths(up, down, dtype)
    ns = [1, ln["both_edges"], ln["tile_plus"], ln["not_divisible"] if down > 1 else 7,
          ln["three_tiles_tail"]]
    assert len(set(ns)) == 5
    stride = max(ns) + 9
    host = np.full((5, stride), np.nan, dtype=dtype)      # nothing past a row's end is read
    for r, n in enumerate(ns):
        host[r, :n] = _case(up, down, n, dtype)[0]
    x = torch.from_numpy(host).cuda()
    n_outs = [resample_ref.out_len(n, up, down) for n in ns]
    longest = max(n_outs)

    def check_rows(y, out_len, what):
        assert y.shape == (5, out_len)
        y = y.cpu().numpy()
        for r, n in enumerate(ns):
            _, ref, bound = _case(up, down, n, dtype)
            k = min(n_outs[r], out_len)
            _check(y[r, :k], ref[:k], bound[:k], f"({up},{down}) {dtype} {what} row {r} n={n}")
            assert not y[r, k:].any() and not np.signbit(y[r, k:]).any(), (what, r)

    full = ops.resample_poly(x, up, down, n=ns)
    check_rows(full, longest, "default")
    # the lengths as a device tensor are the same launch
    n_dev = torch.tensor(ns, dtype=torch.int32, device="cuda")
    assert torch.equal(ops.resample_poly(x, up, down, n=n_dev), full)
    # padded: exact zeros in the tail of every row, the rest unchanged
    padded = ops.resample_poly(x, up, down, n=ns, out_len=longest + 37)
    check_rows(padded, longest + 37, "padded")
    assert torch.equal(padded[:, :longest], full)
    # truncated: the prefix
    cut = longest - 5 if longest > 8 else longest - 1
    short = ops.resample_poly(x, up, down, n=n_dev, out_len=cut)
    check_rows(short, cut, "truncated")
    assert torch.equal(short, full[:, :cut])


# -------------------------------------------------------------- both routes
@pytest.mark.parametrize("dtype,route", [("float64", rs.RS_GLOBAL_TABLE),
                                         ("float32", rs.RS_LDS_TABLE)])
def test_both_table_routes(dtype, route):
    assert rs.plan(1009, 1000, dtype).route == route
    x, ref, bound = _case(1009, 1000, 300, dtype)
    y = ops.resample_poly(torch.from_numpy(np.array(x)).cuda(), 1009, 1000)
    _check(y.cpu().numpy(), ref, bound, f"(1009,1000) {dtype} {rs.ROUTE_NAMES[route]}")


# -------------------------------------------------------------- error paths
def test_error_paths():
    y = ops.resample_poly(torch.empty(0, 16, device="cuda"), 3, 1)
    assert y.shape == (0, 48)
    with pytest.raises(_lib.AinpError, match=r"\(-1\).*bad argument"):
        ops.resample_poly(torch.zeros(8, device="cuda"), 0, 1)
    with pytest.raises(_lib.AinpError, match=r"\(-1\).*bad argument"):
        ops.resample_poly(torch.zeros(8, device="cuda"), 3, -1)
    with pytest.raises(TypeError):
        ops.resample_poly(torch.zeros(8, device="cuda", dtype=torch.float16), 3, 1)
    with pytest.raises(ValueError):
        ops.resample_poly(torch.zeros(2, 8, device="cuda"), 3, 1, n=[8, 9])


# -------------------------------------------------------------------- utils
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_utils_resample_audio(dtype):
    import utils
    n = 1600                                         # 0.1 s at 16 kHz
    x, ref, bound = _case(3, 1, n, dtype, seed=11)
    y = utils.resample_audio(np.array(x), 16000, 48000)
    assert isinstance(y, np.ndarray) and y.dtype == np.dtype(dtype) and y.shape == (3 * n,)
    _check(y, ref, bound, f"resample_audio numpy {dtype}")
    yt = utils.resample_audio(torch.from_numpy(np.array(x)).cuda(), 16000, 48000)
    assert isinstance(yt, torch.Tensor) and yt.is_cuda and yt.dtype == TDT[dtype]
    assert np.array_equal(yt.cpu().numpy(), y)


def _write_wav(path, data, sr):
    pcm = np.clip(np.round(np.atleast_2d(data.T).T * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def test_utils_load_audio_batch(tmp_path):
    import utils
    specs = [(8000, 0.3, 1), (44100, 0.2, 2), (16000, 0.6, 1)]
    paths = []
    for k, (sr, secs, nch) in enumerate(specs):
        n = int(sr * secs)
        data = np.stack([0.8 * _signal(n, "float64", 20 + k + c) for c in range(nch)], axis=1)
        paths.append(str(tmp_path / f"clip{k}.wav"))
        _write_wav(paths[-1], data, sr)
    out = utils.load_audio_batch(paths, sample_rate=16000, max_len=0.5)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
    assert out.shape == (3, 8000)
    out = out.cpu().numpy()
    for k, (path, (sr, secs, nch)) in enumerate(zip(paths, specs)):
        want, got_sr = utils.load_audio(path, sample_rate=16000, max_len=0.5)
        assert got_sr == 16000 and want.shape == (8000,)
        if sr == 16000:
            assert np.array_equal(out[k], want)          # no resampling: exact
            continue
        mono = utils._read_any(path)[0].mean(axis=1)
        S = resample_ref.abs_sum(mono, 16000, sr)
        S = np.pad(S, (0, max(0, 8000 - len(S))))[:8000]
        bound = 2 * (resample_ref.taps_per_phase(16000, sr) + 3) * U["float32"] * S
        _check(out[k], want.astype(np.float64), bound, f"load_audio_batch {sr} Hz")
        assert not out[k, resample_ref.out_len(len(mono), 16000, sr):].any()
    with pytest.raises(IOError, match="missing.wav"):
        utils.load_audio_batch([paths[0], str(tmp_path / "missing.wav")])


# --------------------------------------------------------------- model_eval
def test_export_48k_pairs(tmp_path):
    import utils
    from models import model_eval
    src, rec, out = (str(tmp_path / d) for d in ("clean", "restored", "pairs"))
    n = 4000                                          # 0.25 s at 16 kHz
    for k in range(2):
        clean = 0.4 * _signal(n, "float64", 40 + k)
        restored = clean.copy()
        restored[1000:1100] *= 0.5                    # a fake "restored" copy
        utils.save_audio(clean, os.path.join(src, f"clip{k}.flac"), 16000, normalize=False)
        utils.save_audio(restored, os.path.join(rec, f"clip{k}_janssen_inpainted.flac"), 16000,
                         normalize=False)
    utils.save_audio(0.4 * _signal(n, "float64", 50), os.path.join(src, "unpaired.flac"), 16000,
                     normalize=False)
    pairs = model_eval.export_48k_pairs(src, rec, out, "janssen")
    assert [tuple(os.path.basename(p) for p in pair) for pair in pairs] == [
        (f"clip{k}_signal.wav", f"clip{k}_janssen_solution.wav") for k in range(2)]
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for pair in pairs for p in pair)
    tpp = resample_ref.taps_per_phase(3, 1)
    for k, (signal_wav, solution_wav) in enumerate(pairs):
        for wav, flac in ((signal_wav, os.path.join(src, f"clip{k}.flac")),
                          (solution_wav, os.path.join(rec, f"clip{k}_janssen_inpainted.flac"))):
            with wave.open(wav, "rb") as w:
                assert w.getframerate() == 48000 and w.getnchannels() == 1
                assert w.getnframes() == 3 * n
                pcm = np.frombuffer(w.readframes(3 * n), "<i2")
            x = utils._read_any(flac)[0].mean(axis=1).astype(np.float64)
            ref = resample_ref.resample(x, 3, 1)
            bound = 1.0 / 32767 + (tpp + 3) * U["float64"] * resample_ref.abs_sum(x, 3, 1)
            # save_audio stores round(32767 y)
            _check(pcm / 32767.0, ref, bound, os.path.basename(wav))
