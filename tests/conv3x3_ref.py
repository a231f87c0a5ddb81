"""Plain torch restatement of the 3x3 convolution ABI (include/ainp.h:
ainp_conv3x3_fwd_ex / _dgrad_ex / _wgrad_ex over csrc/conv.hip,
csrc/conv_x6.hip and csrc/conv_route.h), for the tests only, in whatever dtype
it is asked for: float64 for the reference proper, float32 for the rounding
floor the GPU tests measure against it (gan_glue_ref.within_floor).

  y  = conv2d(pad(act(x)), w) + bias,   act(x) = relu(x * scale + shift)
  dx = conv_transpose(dy, w),  dw = sum dy * act(x) shifted,  db = sum dy
  BatchNorm partial sums: per channel sum y | sum y^2 of the stored y

in the layouts of the ABI ("nchw", "cl" = [N][H][W][C], "cfnt" = [C][H][N][W]).
The bf16 arithmetic follows test_gpu_kernels.py::test_conv3x3_bf16: act(x) is
one fp32 fmaf, then act(x), w and dy are rounded to bf16; a bf16-stored y is
the fp32 y rounded once.

The same module holds the planes, channel pairs, input builders and the list
of calls one (pair, precision) makes, so tests/test_cpu_conv3x3_ref.py (no
GPU: the reference against autograd, the exactness conditions of the integer
data, the kernel every call reaches) and tests/test_gpu_conv3x3_edges.py /
tests/conv3x3_edge_worker.py (the kernels) walk one table.  The builders are
cached: a case is built once and shared, and nobody writes into what they
return.
"""
import functools
import os
import re
import zlib

import torch
import torch.nn.functional as F

from gan_glue_ref import within_floor  # noqa: F401  (the GPU tests' element-wise rule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_H = os.path.join(ROOT, "ml-audio-inpainting_amd", "csrc", "conv_route.h")

# include/ainp.h
BF16, DY16, X16, Y16, XCL, YCL, GCL, YCFNT = 2, 4, 8, 16, 32, 64, 128, 256
BN_Y16 = 2

# ------------------------------------------------------------------ planes
# (H, W): lone pixel; tile - 1; one tile; one past; two tiles + 1, for every
# tiling of conv_route.h and the kernel sources
EDGE_PLANES = [
    (1, 1), (2, 3),
    # 8 x 48 (CV_FT x CV_TT); conv3x3_small_fwd's PX = 3 pixels per thread sit
    # 16 columns apart: 16, 17, 32, 33 columns
    (7, 47), (8, 48), (9, 49), (17, 97), (8, 16), (9, 17),
    # 16 x 32 and 8 x 32 (cx6, dg8, cxp, cxq, cdf, cdd)
    (7, 31), (8, 32), (9, 33), (15, 31), (16, 32), (17, 33), (17, 65), (33, 65),
    # 16 rows x 14 columns x 4 strips per workgroup (R1_*, R16_*)
    (16, 14), (17, 15), (15, 55), (16, 56), (16, 57), (17, 57), (33, 113),
    # 32 x 62 and 32 x 14 (SW_RS, SW_TW, SWC_TW); SW_RB = 8 rows per batch
    (31, 61), (32, 62), (33, 63), (65, 125), (31, 13), (32, 14), (33, 15), (65, 29),
    (24, 14), (25, 15),
    # 4 x 24 (wx6, wdm) and the 8 x 24 / 16 x 24 tile rows of x6s; their three
    # 8-column segments
    (3, 23), (4, 24), (5, 25), (9, 49), (7, 23), (8, 24), (9, 25), (17, 49), (15, 23), (16, 24),
    (17, 25), (33, 49),
    (4, 8), (5, 9), (4, 17),
    # 2 x 64 (WG_FT x WG_TT)
    (1, 63), (2, 64), (3, 65), (5, 129),
]
EDGE_PLANES = list(dict.fromkeys(EDGE_PLANES))
N3_PLANES = [(9, 33), (17, 15), (5, 25)]          # run with N = 3 as well
# more tiles than the largest default persistent grid, fewer than twice it;
# 9 rows are not a multiple of any tile, so a workgroup's walk crosses samples
WALK = (65, 9, 129)
WALK_TILES = {(8, 32): 650, (4, 24): 1170, (2, 64): 975}
# the real-valued checks: a lone pixel, one tile, one past, two tiles + 1
REAL_PLANES = [(1, 1), (8, 32), (9, 33), (16, 32), (17, 33), (33, 65), (8, 48), (9, 49), (17, 97),
               (16, 56), (17, 57), (33, 113), (32, 62), (33, 63), (4, 24), (5, 25), (9, 49),
               (2, 64), (3, 65), (5, 129)]
REAL_PLANES = list(dict.fromkeys(REAL_PLANES))


def shapes(planes=None, walk=True):
    """(N, H, W) of one pair's run."""
    planes = EDGE_PLANES if planes is None else planes
    out = [(1, h, w) for h, w in planes] + [(3, h, w) for h, w in N3_PLANES if (h, w) in planes]
    return out + ([WALK] if walk else [])


# ------------------------------------------------------------------ pairs
MODEL_PAIRS = [(1, 16), (16, 1), (2, 16), (16, 2), (16, 32), (32, 16), (32, 64), (64, 32)]
# the generic exact kernel: CT = 1 with predicated staging and a partial
# 8-channel chunk; a second chunk / second 16-channel tile of one channel;
# (20, 33); the `fast` staging with CT = 3 and 4; (64, 64)
EXACT_PAIRS = [(3, 5), (9, 17), (20, 33), (8, 48), (24, 64), (64, 64)]
# weight gradients whose 32-channel passes take different kernels / several passes
WGRAD_PAIRS = [(48, 16), (33, 64), (40, 32), (64, 16)]
# the persistent split-bf16 kernels with 18 of their 32 output channels (forward
# of (16, 18), data gradient of (18, 16)): NCHW only -- their channel-last
# stores write four channels at a time, so conv_route.h refuses such a Cout
PARTIAL_PAIRS = [(16, 18), (18, 16)]
PAIRS = MODEL_PAIRS + EXACT_PAIRS + WGRAD_PAIRS + PARTIAL_PAIRS
X6_MODEL_PAIRS = [(16, 32), (32, 16), (32, 64), (64, 32)]
PRECISIONS = ["fp32", "bf16", "st16"]     # st16: bf16 storage of x / y / dy


def small_pair(a, b):
    return (a in (1, 2) and b == 16) or (b in (1, 2) and a == 16)


def conv_is_x6(cin, cout):
    """A conv over `cin` source channels producing `cout` runs on a split-bf16
    kernel in the default environment (conv_route.h x6_route), so the bf16
    arithmetic rounds its operands.  The CPU test holds this against the
    routing table itself."""
    if small_pair(cin, cout) or not 16 <= cout <= 64:
        return False
    cop = 32 if cout <= 32 else 64
    return (cin, cop) in ((32, 64), (16, 32), (64, 32)) or (cin, cout) == (32, 16)


def wgrad_pass_is_x6(cp, cout):
    """One 32-channel pass of a weight gradient runs on a split-bf16 kernel."""
    return (cp == 32 and cout in (16, 64)) or (cp == 16 and cout == 32)


def wgrad_passes(cin):
    return [(c0, min(32, cin - c0)) for c0 in range(0, cin, 32)]


# ------------------------------------------------------------------ layouts
_TO = {"nchw": (0, 1, 2, 3), "cl": (0, 2, 3, 1), "cfnt": (1, 2, 0, 3)}
_FROM = {"nchw": (0, 1, 2, 3), "cl": (0, 3, 1, 2), "cfnt": (2, 0, 1, 3)}


def lay_of(flag, C):
    """The layout a set AINP_CONV_XCL / _YCL / _GCL flag means for a tensor of
    C channels: channel-last for more than two channels; the 1-2-channel side
    of the small pairs is planar with or without the flag (include/ainp.h)."""
    return "cl" if flag and C > 2 else "nchw"


def to_lay(t, lay):
    """NCHW tensor -> a contiguous tensor in `lay`."""
    return t.permute(*_TO[lay]).contiguous()


def from_lay(t, lay):
    """A tensor in `lay` -> its NCHW view."""
    return t.permute(*_FROM[lay])


# ------------------------------------------------------------------ reference
def bf(t):
    """t rounded to fp32, then to bf16 (nearest-even), in t's dtype."""
    return t.float().bfloat16().to(t.dtype)


def act(x, scale, shift, fp32_fma=False):
    """relu(x * scale + shift) per channel (identity without a scale), in x's
    dtype.  fp32_fma: the value one fp32 fmaf gives -- the product of two
    float32 values is exact in float64, the sum is rounded once there and once
    more to float32 -- as the bf16 kernels round it before the bf16 rounding."""
    if scale is None:
        return x
    C = x.shape[1]
    if fp32_fma:
        z = (x.double() * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)).float()
        return torch.relu(z).to(x.dtype)
    return torch.relu(x * scale.to(x.dtype).view(1, C, 1, 1) + shift.to(x.dtype).view(1, C, 1, 1))


def fwd_ref(x, w, bias, scale=None, shift=None, xlay="nchw", ylay="nchw", bf16=False, y16=False,
            dtype=torch.float64):
    """-> (y in ylay, sums [2 Cout] = sum y | sum y^2 of the stored y)."""
    a = act(from_lay(x, xlay).to(dtype), scale, shift, fp32_fma=bf16)
    w = w.to(dtype)
    if bf16:
        a, w = bf(a), bf(w)
    y = F.conv2d(a, w, None if bias is None else bias.to(dtype), padding=1)
    if y16:
        y = bf(y)
    return to_lay(y, ylay), torch.cat([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])


def dgrad_ref(dy, w, glay="nchw", dxlay="nchw", bf16=False, dtype=torch.float64):
    """-> dx in dxlay ("cfnt": [Cin][H][N][W])."""
    g, w = from_lay(dy, glay).to(dtype), w.to(dtype)
    if bf16:
        g, w = bf(g), bf(w)
    N, _, H, W = g.shape
    dx = torch.nn.grad.conv2d_input((N, w.shape[1], H, W), w, g.contiguous(), padding=1)
    return to_lay(dx, dxlay)


def wgrad_ref(x, dy, scale=None, shift=None, xlay="nchw", glay="nchw", bf16=False,
              dtype=torch.float64):
    """-> (dw [Cout, Cin, 3, 3], db [Cout]).  bf16: the passes of 32 input
    channels that run on a split-bf16 kernel round act(x) and dy; the others
    are fp32-accurate (wgrad_pass_is_x6).  db sums dy as it is stored."""
    a = act(from_lay(x, xlay).to(dtype), scale, shift, fp32_fma=bf16).contiguous()
    g = from_lay(dy, glay).to(dtype).contiguous()
    Cin, Cout = a.shape[1], g.shape[1]
    dw = torch.empty(Cout, Cin, 3, 3, dtype=dtype)
    for c0, cp in wgrad_passes(Cin):
        ap, gp = a[:, c0:c0 + cp].contiguous(), g
        if bf16 and wgrad_pass_is_x6(cp, Cout):
            ap, gp = bf(ap), bf(g)
        dw[:, c0:c0 + cp] = torch.nn.grad.conv2d_weight(ap, (Cout, cp, 3, 3), gp, padding=1)
    return dw, g.sum((0, 2, 3))


# ------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _cached(fn):
    """Small cases are kept for the session; the persistent-walk ones (tens of
    megabytes each) only while one pair runs."""
    small, big = functools.lru_cache(maxsize=None)(fn), functools.lru_cache(maxsize=4)(fn)

    @functools.wraps(fn)
    def get(cin, cout, N, H, W, *rest):
        return (big if N * H * W > 20000 else small)(cin, cout, N, H, W, *rest)
    return get


@_cached
def int_case(cin, cout, N, H, W, thin=False):
    """Integer data: x in [-3, 3] (even where its channel's scale is 0.5, so
    act(x) is an integer), dy in [-2, 2], w in [-2, 2], bias in [-3, 3], scale
    in {0.5, 1, 2}, shift an integer in [-2, 2].  Every product and every
    partial sum in any order is an integer below 2^24, exact in fp32, and a
    three-way bf16 split of such a value is the value, so the float64 result
    is the only correct fp32, split-bf16 and bf16 result.  thin: weights are
    zeroed (a fixed random half at a time) until max |y| <= 256, with and
    without the prologue, so y is exact in bf16 storage too.
    -> dict of float32 tensors (NCHW)."""
    g = _gen("int", cin, cout, N, H, W)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cin,), generator=g)]
    shift = _randint(g, -2, 2, (cin,))
    x = _randint(g, -3, 3, (N, cin, H, W))
    odd = (x.abs() % 2 == 1) & (scale == 0.5).view(1, cin, 1, 1)
    x = torch.where(odd, x - torch.sign(x), x)
    dy = _randint(g, -2, 2, (N, cout, H, W))
    w = _randint(g, -2, 2, (cout, cin, 3, 3))
    bias = _randint(g, -3, 3, (cout,))
    if thin:
        keep = torch.rand(w.shape, generator=g)
        level = 1.0
        while True:
            wt = torch.where(keep < level, w, torch.zeros(()))
            worst = max(float(F.conv2d(a.abs(), wt.abs(), bias.abs(), padding=1).max())
                        for a in (x, act(x, scale, shift)))
            if worst <= 256:
                break
            level *= 0.5
        w = wt
        assert float(w.abs().sum()) > 0
    return dict(x=x, dy=dy, w=w, bias=bias, scale=scale, shift=shift)


@_cached
def real_case(cin, cout, N, H, W):
    """The distributions of test_gpu_kernels.py::test_conv3x3_fwd_dgrad_wgrad
    (x, dy ~ N(0, 1), w ~ 0.2 N(0, 1), scale ~ U(0.5, 1.5)), with a bias, a
    shift and a per-channel offset of dy that keep each channel's sums of y
    and of dy away from cancellation (|sum| >= 0.1 sum |.|, asserted in
    test_cpu_conv3x3_ref.py): the bias gradient and the BatchNorm sums are
    checked per channel, relative to their own value."""
    g = _gen("real", cin, cout, N, H, W)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    sign = lambda n: torch.randint(0, 2, (n,), generator=g).float() * 2 - 1  # noqa: E731
    bias = sign(cout) * (1 + torch.rand(cout, generator=g)) * (1 + 0.4 * (9 * cin) ** 0.5)
    scale = torch.rand(cin, generator=g) + 0.5
    shift = torch.randn(cin, generator=g) * 0.3 + 0.5
    dy = torch.randn(N, cout, H, W, generator=g) + (sign(cout) * 1.5).view(1, cout, 1, 1)
    return dict(x=x, dy=dy, w=w, bias=bias, scale=scale, shift=shift)


@_cached
def int_refs(cin, cout, N, H, W, thin, pro):
    """float64 (y, sums, sum |y|, sum y^2, dx, dw, db) of an integer case, NCHW."""
    c = int_case(cin, cout, N, H, W, thin)
    sc, sh = (c["scale"], c["shift"]) if pro else (None, None)
    y, sums = fwd_ref(c["x"], c["w"], c["bias"], sc, sh)
    dw, db = wgrad_ref(c["x"], c["dy"], sc, sh)
    return dict(y=y, sums=sums, sabs=y.abs().sum((0, 2, 3)), dx=dgrad_ref(c["dy"], c["w"]),
                dw=dw, db=db)


# ------------------------------------------------------------------ calls
def layouts(op):
    """The layout flag sets of one entry point."""
    if op == "fwd":
        return [0, XCL, YCL, XCL | YCL]
    if op == "dgrad":
        return [0, XCL, YCL, XCL | YCL, YCFNT, XCL | YCFNT]
    if op == "bnr":
        return [YCL, XCL | YCL]
    return [0, XCL, GCL, XCL | GCL]


def storage_flags(op, prec):
    """The precision flag sets of one entry point."""
    if prec == "fp32":
        return [0]
    if prec == "bf16":
        return [BF16]
    if op == "fwd":
        return [BF16 | X16 | Y16]
    if op in ("dgrad", "bnr"):
        return [BF16 | DY16]
    return [BF16 | DY16 | X16, BF16 | DY16, BF16 | X16]


def calls(cin, cout, prec, shp=None):
    """Every launch of one (pair, precision): (op, N, H, W, flags, pro).  The
    data gradient has no prologue; conv3x3_dgrad_bnr takes dx of 16, 32 or 64
    channels."""
    out = []
    for N, H, W in (shapes() if shp is None else shp):
        for op in ("fwd", "dgrad", "bnr", "wgrad"):
            if op == "bnr" and cin not in (16, 32, 64):
                continue
            for st in storage_flags(op, prec):
                for lay in layouts(op):
                    for pro in ((True, False) if op in ("fwd", "wgrad") else (False,)):
                        out.append((op, N, H, W, st | lay, pro))
    return out


# ------------------------------------------------------------------ environments
# name -> (variable, value, env bits of tests/conv3x3_route_names.cpp, pairs, precisions):
# the routes only a fresh process can reach (conv_env() is read once)
ENV_BITS = dict(exact=1, x6_tiled=2, small_rows0=4, dgrad_bnr0=8, conv16_dma0=16, dgrad16_dma0=32,
                wgrad16_dma0=64, occ2=128, occ4=256, small_wgrad_tile=512)
SMALL_CL_PAIRS = [(1, 16), (16, 1), (2, 16), (16, 2)]
CHILD_SETTINGS = {
    "exact": ("AINP_CONV_EXACT", "1", ENV_BITS["exact"], MODEL_PAIRS, ["fp32", "bf16"]),
    "x6_tiled": ("AINP_CONV_X6_TILED", "1", ENV_BITS["x6_tiled"], X6_MODEL_PAIRS,
                 ["fp32", "bf16", "st16"]),
    "small_rows0": ("AINP_SMALL_ROWS", "0", ENV_BITS["small_rows0"], SMALL_CL_PAIRS, ["fp32"]),
    "dgrad_bnr0": ("AINP_DGRAD_BNR", "0", ENV_BITS["dgrad_bnr0"],
                   [(16, 1), (16, 2)] + X6_MODEL_PAIRS, ["fp32", "st16"]),
    "conv16_dma0": ("AINP_CONV16_DMA", "0", ENV_BITS["conv16_dma0"], [(16, 32), (32, 64)],
                    ["st16"]),
    "dgrad16_dma0": ("AINP_DGRAD16_DMA", "0", ENV_BITS["dgrad16_dma0"], [(32, 64)], ["st16"]),
    "wgrad16_dma0": ("AINP_WGRAD16_DMA", "0", ENV_BITS["wgrad16_dma0"], [(32, 64)], ["st16"]),
    "occ2": ("AINP_X6_OCC16", "2", ENV_BITS["occ2"], X6_MODEL_PAIRS, ["bf16", "st16"]),
    "occ4": ("AINP_X6_OCC16", "4", ENV_BITS["occ4"], X6_MODEL_PAIRS, ["bf16", "st16"]),
}
# the planes of a child: the tile edges of the kernels the switches select
CHILD_PLANES = [(1, 1), (2, 3), (7, 31), (8, 32), (9, 33), (16, 32), (17, 33), (33, 65), (8, 48),
                (9, 49), (17, 97), (9, 17), (16, 56), (16, 57), (4, 24), (5, 25), (9, 25),
                (33, 49), (2, 64), (3, 65)]


# ------------------------------------------------------------------ conv_route.h
def route_constants():
    """constexpr int NAME = value of conv_route.h."""
    src = open(ROUTE_H).read()
    return {m.group(1): int(m.group(2))
            for m in re.finditer(r"\b([A-Z][A-Z0-9_]*) = (\d+)\b", src)}


def refusal_texts():
    """ConvRefusal name -> its message (conv_refusal_text)."""
    src = open(ROUTE_H).read()
    out = {}
    for m in re.finditer(r'case (CR_\w+): return ((?:\s*"[^"]*")+);', src):
        out[m.group(1)] = "".join(re.findall(r'"([^"]*)"', m.group(2)))
    return out


def route_enum(name):
    """The enumerators of `enum name { ... }` in order, the _COUNT one dropped."""
    src = open(ROUTE_H).read()
    body = re.search(r"enum %s \{(.*?)\};" % name, src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = [t.split("=")[0].strip() for t in body.split(",") if t.strip()]
    return [n for n in names if not n.endswith("_COUNT")]
