"""The window-wise algorithms give the bits they gave before their two layouts
shared one gather and one overlap-add (csrc/janssen_windows.hip):
ainp.janssen.janssen_windowed, janssen_windowed_mask and ainp.spain.spain_inpaint
(H and OMP) on the cases of tests/golden/gen_window_outputs.py against
tests/golden/window_outputs.npz, which the package wrote before that change.

Bit equality is the bar: the solvers between the two streams are the same
kernels, both streams sum in a fixed order, and the unified overlap-add visits
the covering windows of a sample in the ascending order in which the per-gap
kernel picked them out of its loop over all windows.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location(
        "gen_window_outputs", os.path.join(GOLDEN, "gen_window_outputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _gen()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "window_outputs.npz")) as f:
        want = {k: f[k] for k in f.files}
    assert sorted({k.split("/")[0] for k in want}) == sorted(gen.CASES)
    return want


@pytest.mark.parametrize("name", list(gen.CASES))
def test_window_outputs_are_the_parents_bits(name, golden):
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.split("/")[0] == name}
    got = gen.run_case(name)
    assert sorted(got) == sorted(want) and want
    for key, w in want.items():
        g = got[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, key)
        if key.endswith((".iters", ".where", ".atoms")):
            assert g.tolist() == w.tolist(), (name, key)
        else:
            assert np.array_equal(g, w, equal_nan=True), (name, key)
