"""Table of every host-only conv3x3 query of libainp.so over a fixed grid of
channel pairs, shapes, flags and routing environments.

    python tests/golden/gen_conv_route_queries.py            # writes conv_route_queries.json
    python tests/golden/gen_conv_route_queries.py --emit     # this process's environment, to stdout

The fixture was written by the library as it stood before the routing moved
into csrc/conv_route.h; tests/test_cpu_conv_route.py asserts that the library
still answers the same (the routing environment is read once per process, so
each environment is one child process).
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB = os.path.join(ROOT, "ml-audio-inpainting_amd", "ainp", "libainp.so")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_route_queries.json")

PAIRS = [(1, 16), (16, 32), (32, 64), (32, 16), (16, 1), (2, 16), (16, 2), (64, 32), (16, 16),
         (16, 64), (64, 64), (8, 24), (3, 64)]
# the last has C * H * W * 4 past 2^31 for every C: the non-persistent branches
SHAPES = [(1, 1, 1), (2, 9, 49), (4, 257, 334), (32, 257, 334), (2, 257, 1001), (1, 23000, 23400)]
CONV_BF16 = 2
ENVS = {
    "default": {},
    "exact": {"AINP_CONV_EXACT": "1"},
    "x6_tiled": {"AINP_CONV_X6_TILED": "1"},
    "small_rows0": {"AINP_SMALL_ROWS": "0"},
    "x6_occ16_4": {"AINP_X6_OCC16": "4"},
}
ROUTING_VARS = ("AINP_CONV_EXACT", "AINP_CONV_X6_TILED", "AINP_SMALL_ROWS", "AINP_DGRAD_BNR",
                "AINP_CONV16_DMA", "AINP_DGRAD16_DMA", "AINP_WGRAD16_DMA", "AINP_X6_OCC16")
# per (pair, shape) cell, in this order
COLUMNS = ["stat_rows_ex", "stat_rows_ex_bf16", "dy16_ok", "io16_ok", "cl_ok", "dgrad_cfnt_ok",
           "wgrad_workspace", "dgrad_bnr_workspace"]


def emit():
    lib = ctypes.CDLL(LIB)
    i64, ci = ctypes.c_int64, ctypes.c_int
    shape5 = [i64, ci, ci, i64, i64]
    lib.ainp_conv3x3_fwd_stat_parts.restype = ci
    lib.ainp_conv3x3_fwd_stat_parts.argtypes = [i64, i64, i64]
    lib.ainp_conv3x3_fwd_stat_rows_ex.restype = i64
    lib.ainp_conv3x3_fwd_stat_rows_ex.argtypes = shape5 + [ci]
    for name, res in (("dy16_ok", ci), ("io16_ok", ci), ("cl_ok", ci), ("dgrad_cfnt_ok", ci),
                      ("wgrad_workspace", ctypes.c_size_t), ("dgrad_bnr_workspace", i64)):
        f = getattr(lib, "ainp_conv3x3_" + name)
        f.restype, f.argtypes = res, shape5
    table = []
    for cin, cout in PAIRS:
        for n, h, w in SHAPES:
            a = (n, cin, cout, h, w)
            table.append([lib.ainp_conv3x3_fwd_stat_rows_ex(*a, 0),
                          lib.ainp_conv3x3_fwd_stat_rows_ex(*a, CONV_BF16),
                          lib.ainp_conv3x3_dy16_ok(*a), lib.ainp_conv3x3_io16_ok(*a),
                          lib.ainp_conv3x3_cl_ok(*a), lib.ainp_conv3x3_dgrad_cfnt_ok(*a),
                          lib.ainp_conv3x3_wgrad_workspace(*a),
                          lib.ainp_conv3x3_dgrad_bnr_workspace(*a)])
    return {"stat_parts": [lib.ainp_conv3x3_fwd_stat_parts(*s) for s in SHAPES], "table": table}


def run_env(extra):
    env = {k: v for k, v in os.environ.items() if k not in ROUTING_VARS}
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"], env=env,
                       capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def main():
    if "--emit" in sys.argv:
        json.dump(emit(), sys.stdout)
        return
    doc = {"pairs": PAIRS, "shapes": SHAPES, "columns": COLUMNS,
           "envs": {name: run_env(extra) for name, extra in ENVS.items()}}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, sum(len(e["table"]) * len(COLUMNS) + len(e["stat_parts"])
                   for e in doc["envs"].values()), "integers")


if __name__ == "__main__":
    main()
