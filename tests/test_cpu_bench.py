"""CPU tests of bench.py's --dump-outputs writer (no GPU work)."""
import os

import numpy as np
import pytest
import torch

import bench


def _arrays():
    g = torch.Generator().manual_seed(3)
    outputs = {"y": torch.randn(4, 5, 7, generator=g),
               "big": torch.randn(bench.DUMP_FULL + 1000, generator=g),
               "target": torch.complex(torch.randn(6, 3, generator=g), torch.randn(6, 3, generator=g)),
               "loss": torch.tensor(2.5, dtype=torch.float64)}
    state = [("grad.w", torch.randn(bench.DUMP_SAMPLE + 17, generator=g)),
             ("param.b", torch.randn(9, generator=g).to(torch.bfloat16))]
    return outputs, state


def test_dump_outputs_writes_float32_whole_or_seeded_sample(tmp_path):
    outputs, state = _arrays()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    total = bench.dump_outputs(a, outputs, state)
    assert bench.dump_outputs(b, outputs, state) == total
    names = sorted(os.listdir(a))
    assert names == sorted(n + ".npy" for n in list(outputs) + [n for n, _ in state])
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) == total <= bench.DUMP_LIMIT_BYTES
    # small tensors whole, in their own shape; complex as (re, im) pairs
    np.testing.assert_array_equal(got["y"], outputs["y"].numpy())
    np.testing.assert_array_equal(got["target"], torch.view_as_real(outputs["target"]).numpy())
    assert got["loss"].shape == () and got["loss"] == np.float32(2.5)
    np.testing.assert_array_equal(got["param.b"], state[1][1].float().numpy())
    # large tensors: a sample of the cap's size, every value taken from the
    # tensor in index order, the same indices in every run
    assert got["big"].shape == (bench.DUMP_FULL,)
    assert got["grad.w"].shape == (bench.DUMP_SAMPLE,)
    assert np.isin(got["grad.w"], state[0][1].numpy()).all()
    for n in names:
        np.testing.assert_array_equal(got[n[:-4]], np.load(os.path.join(b, n)))
    # the sample follows the data: a changed element at a sampled index shows
    changed = state[0][1].clone()
    changed += 1.0
    bench.dump_outputs(b, {}, [("grad.w", changed)])
    np.testing.assert_allclose(np.load(os.path.join(b, "grad.w.npy")), got["grad.w"] + 1.0,
                               rtol=0, atol=1e-6)


def test_dump_outputs_refuses_to_exceed_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), {"y": torch.zeros(17)})
