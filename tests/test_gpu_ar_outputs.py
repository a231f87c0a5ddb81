"""The five public entries of the audio-regression rows (janssen_inpaint with
both estimators, ar_extrapolate, janssen_windowed with three shapes in one
call, spain_inpaint with both algorithms) return the bytes they returned before
their host paths were merged into two batch drivers and one window planner:
every returned signal, the per-gap ranges, iteration counts / status and
histories, by sha256 against tests/golden/ar_outputs.json, which the package
wrote before the change (tests/golden/gen_ar_outputs.py; the kernels sum in a
fixed order and use no atomics, so the bytes are reproducible)."""
import importlib.util
import json
import os

import pytest
import torch  # noqa: F401  (before ainp: torch brings its own HIP runtime)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_ar_outputs",
                                                  os.path.join(GOLDEN, "gen_ar_outputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _gen()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ar_outputs.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(gen.CASES)
    return want


@pytest.mark.parametrize("name", list(gen.CASES))
def test_ar_bytes_unchanged(name, golden):
    assert gen.run_case(name) == golden[name]
