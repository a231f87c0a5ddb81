"""The GEMM family computes what it computed before its split-K rule and the
256 x 256 tile route moved into csrc/gemm_route.h and ops.split_k: one small
case per public entry and per route (ragged M and N tails, splits that stand
and splits that fall back to one chunk), with the bytes of every output
compared by sha256 against tests/golden/gemm_outputs.json, which the library
wrote before the change (tests/golden/gen_gemm_outputs.py; none of the kernels
uses atomics, so the bytes are reproducible).  Each ainp_gemm_bf16nt case also
asserts that the library's route query names the tile the case is meant for,
and the split-K cases that the planner still picks the split they were chosen
for (tests/golden/gemm_plans.json)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen_gemm_outputs.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_outputs.json")
PLANS = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_gemm_outputs", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _gen()
TILES = {gen.G16: 0, gen.G256: 1, gen.G256B: 2}     # include/ainp.h AINP_GEMM_TILE_*


@pytest.fixture(scope="module")
def golden():
    want = json.load(open(FIXTURE))
    assert sorted(want) == sorted(gen.CASES)
    return want


@pytest.mark.parametrize("name", list(gen.CASES))
def test_gemm_bytes_unchanged(name, golden):
    assert gen.run_case(name) == golden[name]


@pytest.mark.parametrize("name", list(gen.BF16NT))
def test_gemm_bf16nt_case_takes_its_tile(name):
    from ainp import ops
    M, N, K, nsplit, launched, tile = gen.BF16NT[name]
    S, _ = ops.split_k(K, nsplit, ops.splitk_granule(ops.FAMILY_G16))
    assert S == launched
    assert ops.gemm_bf16nt_tile(M, N, K, S) == TILES[tile]


def test_split_cases_are_split_by_the_recorded_plan():
    """wgrad_bf16_km and gemm_bf16nt_splitk run with S > 1: the split the
    planner gave before the change, which it still gives."""
    from ainp import ops
    plans = json.load(open(PLANS))
    for (M, N, K, ms), S in gen.PLAN_SPLITK.items():
        assert S > 1 and plans["_splitk_bf16"][f"{M},{N},{K},{ms}"] == S
        assert ops._splitk_bf16(M, N, K, max_split=ms) == S
    for key, S in gen.PLAN_G256.items():
        assert S > 1 and plans["g256_splits"][key][0][0] == S
        assert ops.g256_splits((tuple(int(v) for v in key.split(",")),))[0][0] == S
