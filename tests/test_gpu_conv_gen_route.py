"""The GAN's general convolution computes what it computed before its routing
moved into csrc/conv_gen_route.h: one small case per kernel (and per main-loop
variant of the channel-last kernels) through the public ops.conv_gen, with the
bytes of y, of the BatchNorm partials and of the memoised bf16 channel-last
copy compared by sha256 against tests/golden/conv_gen_outputs.json, which the
library wrote before the change (tests/golden/gen_conv_gen_outputs.py; the
kernels use no atomics, so the bytes are reproducible).  Each case also
asserts that the plan names the kernel the case is meant for.  The cases under
AINP_SPLITK_TILE=0 (the per-channel split-K epilogue and, on the channel-last
entry, the transposing pass that then writes the bf16 copy) run in one fresh
child process: the library reads that variable once per process."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen_conv_gen_outputs.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_gen_outputs.json")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_conv_gen_outputs", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _gen()


@pytest.fixture(scope="module")
def golden():
    want = json.load(open(FIXTURE))
    assert sorted(want) == sorted(c["name"] for c in gen.CASES)
    return want


def _plan(ops, c):
    k, hin, win = c["k"], c["hin"], c["win"]
    h0, w0 = (hin // 2, win // 2) if c["up0"] else (hin, win)
    crop = c["crop"] or (0, 0)
    return ops.conv_gen_plan(2, c["c0"], h0, w0, c["c1"], hin, win, c["cout"], hin, win, k, k,
                             c["stride"], (k - 1) // 2, crop[0], crop[1], c["bf16"], c["stats"],
                             c["out16"] and c["bf16"])


HERE = [c for c in gen.CASES if not c["env"]]


@pytest.mark.parametrize("case", HERE, ids=[c["name"] for c in HERE])
def test_conv_gen_bytes_unchanged(case, golden, monkeypatch):
    assert gen.run_case(case) == golden[case["name"]]
    _check_plan(case, golden[case["name"]], monkeypatch)


def test_conv_gen_bytes_unchanged_per_channel_splitk_epilogue(golden, monkeypatch):
    assert [c["env"] for c in gen.ENV_CASES] == [{"AINP_SPLITK_TILE": "0"}] * len(gen.ENV_CASES)
    got = gen.run_in_child(gen.ENV_CASES)
    for case in gen.ENV_CASES:
        want = golden[case["name"]]
        assert got[case["name"]] == want, case["name"]
        assert want["stats"] is not None
        assert (want["y16"] is not None) == case["out16"]
        # split-K with the copy wanted, whoever writes it (here: this process's environment)
        _check_plan(case, want, monkeypatch)


def _check_plan(case, want, monkeypatch):
    from ainp import ops
    # the kernel the case is meant for
    monkeypatch.setattr(ops, "CONV_NHWC16_SMALL", case["small"])
    prev = ops.conv16_set_variant(-1)
    try:
        if case["variant"] is not None:
            ops.conv16_set_variant(case["variant"])
        plan = _plan(ops, case)
    finally:
        ops.conv16_set_variant(prev)
    kernel = case["kernel"]
    if kernel == gen.NHWC16:
        v = case["variant"] if case["variant"] is not None else prev
        kernel = ("nhwc16_tiles", "nhwc16_ring", "nhwc16_wide",
                  "nhwc16_wide" if case["cout"] > 64 else "nhwc16_tiles")[v]
    assert plan.kernel == kernel and plan.refusal is None
    assert plan.entry == (1 if kernel.startswith("nhwc16") else 0)
    assert plan.y16_ok == (want["y16"] is not None)
    assert (plan.nsplit > 1) == ("splitk" in case["name"] or case["name"].startswith(
        ("nhwc16_two_sources", "nhwc16_expanded_src")))
