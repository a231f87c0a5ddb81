"""Table of what the library and ainp.ops answer about the routing of the
GAN's general convolution (conv_gen) over a fixed grid of channel pairs,
kernels, strides, source sizes, shapes, statistics and routing environments.

    python tests/golden/gen_conv_gen_route_queries.py          # writes conv_gen_route_queries.json
    python tests/golden/gen_conv_gen_route_queries.py --emit   # this environment, to stdout

Per cell: ainp_conv_gen_stat_parts, ainp_conv_gen_workspace, "the
few-input-channel kernel serves the fp32 call" and "the bf16 call takes the
channel-last entry point".  The fixture was written by the library as it
stood before the routing moved into csrc/conv_gen_route.h, where the last two
were ops._direct_route and `Cout > 1 and ops._nhwc16_route` (as ops.conv_gen
combined them); since then they are read off ops.conv_gen_plan.
tests/test_cpu_conv_gen_route.py asserts that the answers are unchanged (the
environment is read once per process, so each environment is one child
process; ops imports without a GPU).
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "ml-audio-inpainting_amd")
LIB = os.path.join(PKG, "ainp", "libainp.so")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_gen_route_queries.json")

# (C0, C1, Cout)
PAIRS = [(1, 0, 16), (3, 0, 64), (4, 0, 64), (5, 0, 64), (2, 0, 64), (64, 0, 1), (33, 0, 1),
         (64, 1, 64), (32, 32, 48), (64, 0, 96), (128, 0, 70), (256, 0, 130), (512, 512, 512),
         (512, 0, 260)]
KERNELS = [3, 4, 5, 7]
STRIDES = [1, 2]
# output (N, Ho, Wo): one pixel; ragged tiles; the model's resolution; N * Ho * Wo * Cout
# past 2^31 for every Cout >= 8
SHAPES = [(1, 1, 1), (2, 9, 11), (8, 256, 256), (16, 4096, 4096)]
ENVS = {
    "default": {},
    "exact": {"AINP_CONV_EXACT": "1"},
    "split_wide0": {"AINP_CONV_SPLIT_WIDE": "0"},
    "split_wide3": {"AINP_CONV_SPLIT_WIDE": "3"},
    "splitk_tile0": {"AINP_SPLITK_TILE": "0"},
    "smallcin0": {"AINP_CONV_SMALLCIN": "0"},
    "nhwc16_0": {"AINP_CONV_NHWC16": "0"},
    "nhwc16_small0": {"AINP_CONV_NHWC16_SMALL": "0"},
    "nhwc16_small_all": {"AINP_CONV_NHWC16_SMALL": "all"},
}
ROUTING_VARS = ("AINP_CONV_SPLIT_WIDE", "AINP_SPLITK_TILE", "AINP_COUT1_B", "AINP_CONV_SMALLCIN",
                "AINP_SMALLCIN_LDS16", "AINP_CONV_EXACT", "AINP_CONV_GEN_BK",
                "AINP_CONV_GEN_B16_BK", "AINP_CONV16", "AINP_CONV16_RING", "AINP_CONV16_SMALLCO",
                "AINP_WIDE_PF", "AINP_CONV_NHWC16", "AINP_CONV_NHWC16_SMALL", "AINP_CONV_OUT16",
                "AINP_OUT16_DIRECT")
COLUMNS = ["stat_parts", "workspace", "direct", "nhwc16"]


def cells():
    """(C0, C1, Cout, k, stride, pad, up0, N, H0, W0, Hin, Win, Ho, Wo, stats)"""
    out = []
    for c0, c1, cout in PAIRS:
        for k in KERNELS:
            pad = (k - 1) // 2
            for s in STRIDES:
                for n, ho, wo in SHAPES:
                    hin, win = (ho - 1) * s + k - 2 * pad, (wo - 1) * s + k - 2 * pad
                    for up0 in (0, 1):
                        # source 0 at half size: the exact 2x upsample where
                        # the input size is even, nearest resampling otherwise
                        h0, w0 = (max(1, hin // 2), max(1, win // 2)) if up0 else (hin, win)
                        for stats in (0, 1):
                            out.append((c0, c1, cout, k, s, pad, up0, n, h0, w0, hin, win, ho, wo,
                                        stats))
    return out


def emit():
    lib = ctypes.CDLL(LIB)
    i64, ci = ctypes.c_int64, ctypes.c_int
    lib.ainp_conv_gen_stat_parts.restype = ci
    lib.ainp_conv_gen_workspace.restype = ctypes.c_size_t
    lib.ainp_conv_gen_stat_parts.argtypes = lib.ainp_conv_gen_workspace.argtypes = \
        [i64, ci, ci, ci, ci, i64, i64]
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ainp import ops
    table = []
    for c0, c1, cout, k, s, pad, up0, n, h0, w0, hin, win, ho, wo, stats in cells():
        q = (n, c0 + c1, k, k, cout, ho, wo)
        if hasattr(ops, "_direct_route"):    # before csrc/conv_gen_route.h
            a = (c0, c1, h0, w0, hin, win, k, k, cout, bool(stats))
            direct, nhwc16 = ops._direct_route(*a), cout > 1 and ops._nhwc16_route(*a)
        else:
            a = (n, c0, h0, w0, c1, hin, win, cout, hin, win, k, k, s, pad)
            direct = ops.conv_gen_plan(*a, want_stats=stats).kernel == "smallcin"
            nhwc16 = ops.conv_gen_plan(*a, want_stats=stats, bf16=True).entry == 1
        table.append([lib.ainp_conv_gen_stat_parts(*q), lib.ainp_conv_gen_workspace(*q),
                      int(bool(direct)), int(bool(nhwc16))])
    return table


def run_envs():
    """{environment name: table}, one child process each, side by side."""
    base = {k: v for k, v in os.environ.items() if k not in ROUTING_VARS}
    procs = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--emit"],
                                    env=dict(base, **extra), stdout=subprocess.PIPE, text=True)
             for name, extra in ENVS.items()}
    out = {}
    for name, p in procs.items():
        stdout, _ = p.communicate()
        if p.returncode:
            raise RuntimeError(f"{name}: exit status {p.returncode}")
        out[name] = json.loads(stdout)
    return out


def main():
    if "--emit" in sys.argv:
        json.dump(emit(), sys.stdout)
        return
    doc = {"pairs": PAIRS, "kernels": KERNELS, "strides": STRIDES, "shapes": SHAPES,
           "columns": COLUMNS, "envs": run_envs()}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, sum(len(t) * len(COLUMNS) for t in doc["envs"].values()), "integers")


if __name__ == "__main__":
    main()
