"""tests/conv3x3_ref.py without a GPU: the float64 reference of the 3x3 conv
ABI against torch autograd in every layout, the conditions that make the
integer cases exact in fp32 / split-bf16 / bf16 (proved for every case of the
tables), the kernel every call of the GPU tests reaches according to
csrc/conv_route.h (tests/conv3x3_route_names.cpp, compiled here), and the tile
counts of the persistent-walk shape.
"""
import itertools
import subprocess

import pytest
import torch
import torch.nn.functional as F

import conv3x3_ref as R

D = torch.float64
TWO24 = float(2 ** 24)


# ------------------------------------------------------------------ reference
@pytest.mark.parametrize("cin,cout,N,H,W", [(1, 16, 2, 5, 7), (16, 2, 1, 4, 9), (3, 5, 3, 6, 4),
                                            (20, 33, 1, 3, 5), (40, 32, 2, 1, 1)])
@pytest.mark.parametrize("pro", [True, False])
def test_reference_matches_autograd(cin, cout, N, H, W, pro):
    c = R.real_case(cin, cout, N, H, W)
    sc, sh = (c["scale"], c["shift"]) if pro else (None, None)
    x = c["x"].double()
    a = x if not pro else torch.relu(x * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    a = a.clone().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    b = c["bias"].double().requires_grad_(True)
    y = F.conv2d(a, w, b, padding=1)
    dy = c["dy"].double()
    y.backward(dy)
    close = lambda p, q: float((p - q).abs().max()) <= 1e-12 * max(1.0, float(q.abs().max()))  # noqa: E731
    for xlay, ylay in itertools.product(("nchw", "cl"), ("nchw", "cl")):
        got, sums = R.fwd_ref(R.to_lay(c["x"], xlay), c["w"], c["bias"], sc, sh, xlay, ylay)
        assert got.dtype == D and close(R.from_lay(got, ylay), y.detach()), (xlay, ylay)
        assert close(sums[:cout], y.detach().sum((0, 2, 3)))
        assert close(sums[cout:], (y.detach() ** 2).sum((0, 2, 3)))
        dw, db = R.wgrad_ref(R.to_lay(c["x"], xlay), R.to_lay(c["dy"], ylay), sc, sh, xlay, ylay)
        assert close(dw, w.grad) and close(db, b.grad), (xlay, ylay)
    for glay, dxlay in itertools.product(("nchw", "cl"), ("nchw", "cl", "cfnt")):
        dx = R.dgrad_ref(R.to_lay(c["dy"], glay), c["w"], glay, dxlay)
        want = (cin, H, N, W) if dxlay == "cfnt" else (N, H, W, cin) if dxlay == "cl" else (N, cin, H, W)
        assert tuple(dx.shape) == want and dx.is_contiguous()
        assert close(R.from_lay(dx, dxlay), a.grad), (glay, dxlay)
    # the functional gradients the reference is built from are autograd's
    assert close(torch.nn.grad.conv2d_input(a.shape, w.detach(), dy, padding=1), a.grad)
    assert close(torch.nn.grad.conv2d_weight(a.detach(), w.shape, dy, padding=1), w.grad)


def test_reference_bf16_arithmetic():
    """As test_gpu_kernels.py::test_conv3x3_bf16: one fp32 fmaf, then bf16
    operands; a bf16-stored y is the fp32 y rounded once; only the passes of
    a weight gradient that run on a split-bf16 kernel round."""
    c = R.real_case(48, 16, 2, 6, 5)
    x, w, b, sc, sh, dy = (c[k] for k in ("x", "w", "bias", "scale", "shift", "dy"))
    a32 = torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1)))
    a = R.act(x.double(), sc, sh, fp32_fma=True)
    assert float((a - a32.double()).abs().max()) <= 2 ** -23 * float(a.abs().max())
    assert torch.equal(a, a.float().double())
    ab, wb, gb = a.float().bfloat16().double(), w.bfloat16().double(), dy.bfloat16().double()
    y, _ = R.fwd_ref(x, w, b, sc, sh, bf16=True)
    assert torch.equal(y, F.conv2d(ab, wb, b.double(), padding=1))
    y16, sums = R.fwd_ref(x, w, b, sc, sh, bf16=True, y16=True)
    assert torch.equal(y16, y.float().bfloat16().double())
    assert torch.equal(sums[:16], y16.sum((0, 2, 3)))
    assert torch.equal(R.dgrad_ref(dy, w, bf16=True),
                       torch.nn.grad.conv2d_input(x.shape, wb, gb, padding=1))
    dw, db = R.wgrad_ref(x, dy, sc, sh, bf16=True)     # (48, 16): x6s, then wgrad_t in fp32
    assert R.wgrad_passes(48) == [(0, 32), (32, 16)]
    assert R.wgrad_pass_is_x6(32, 16) and not R.wgrad_pass_is_x6(16, 16)
    assert torch.equal(dw[:, :32], torch.nn.grad.conv2d_weight(ab[:, :32].contiguous(),
                                                               (16, 32, 3, 3), gb, padding=1))
    assert torch.equal(dw[:, 32:], torch.nn.grad.conv2d_weight(a[:, 32:].contiguous(),
                                                               (16, 16, 3, 3), dy.double(),
                                                               padding=1))
    assert torch.equal(db, dy.double().sum((0, 2, 3)))


# ------------------------------------------------------------------ the planes
def test_planes_and_pairs_hold_what_the_tilings_need():
    need = [(1, 1), (2, 3), (7, 31), (8, 32), (9, 33), (7, 47), (8, 48), (9, 49), (16, 14),
            (17, 15), (16, 56), (16, 57), (4, 24), (5, 25), (2, 64), (3, 65), (32, 62), (33, 63),
            (33, 15), (17, 97), (33, 65)]
    assert set(need) <= set(R.EDGE_PLANES) and len(set(R.EDGE_PLANES)) == len(R.EDGE_PLANES)
    k = R.route_constants()
    tilings = [(k["CV_FT"], k["CV_TT"]), (16, 32), (8, 32), (k["R1_RS"], 4 * k["R1_TW"]),
               (k["R16_RS"], 4 * k["R16_TW"]), (k["SW_RS"], k["SW_TW"]), (k["SW_RS"], k["SWC_TW"]),
               (4, 24), (8, 24), (16, 24), (2, 64)]
    assert (k["TR"], k["TC"], k["TT"]) == (8, 32, 24)     # the last of cx6 / cdf / cdd; wdm
    for tr, tc in tilings:   # tile - 1, one tile, one past, two tiles + 1
        for h, w in ((tr - 1, tc - 1), (tr, tc), (tr + 1, tc + 1), (2 * tr + 1, 2 * tc + 1)):
            assert (h, w) in R.EDGE_PLANES, (tr, tc, h, w)
    assert len(R.N3_PLANES) == 3 and set(R.N3_PLANES) <= set(R.EDGE_PLANES)
    assert set(R.REAL_PLANES) <= set(R.EDGE_PLANES) and set(R.CHILD_PLANES) <= set(R.EDGE_PLANES)
    for pair in [(1, 16), (16, 1), (2, 16), (16, 2), (16, 32), (32, 16), (32, 64), (64, 32), (3, 5),
                 (9, 17), (20, 33), (8, 48), (24, 64), (64, 64), (48, 16), (33, 64), (40, 32),
                 (64, 16)]:
        assert pair in R.PAIRS
    assert len(set(R.PAIRS)) == len(R.PAIRS)


def test_persistent_walk_tile_counts():
    """(65, 9, 129): more tiles than any default persistent grid or slab count
    and fewer than twice the largest (the 4 x 24 tiles: fewer than three times
    WG_BLOCKS), a sample's tiles no divisor of a grid, so every workgroup's
    strided walk takes a second tile in another sample."""
    k = R.route_constants()
    N, H, W = R.WALK
    count = lambda tr, tc: N * -(-H // tr) * -(-W // tc)  # noqa: E731
    assert {t: count(*t) for t in R.WALK_TILES} == R.WALK_TILES
    assert R.WALK_TILES == {(8, 32): 650, (4, 24): 1170, (2, 64): 975}
    g1, g2, wg = k["X6P_GRID1"], k["X6P_GRID2"], k["WG_BLOCKS"]
    assert g1 < g2 < R.WALK_TILES[8, 32] < 2 * g2
    assert wg < R.WALK_TILES[2, 64] < 2 * wg
    assert 2 * wg < R.WALK_TILES[4, 24] < 3 * wg
    for (tr, tc), n in R.WALK_TILES.items():
        per_sample = n // N
        assert all(g % per_sample for g in (g1, g2, wg)), (tr, tc)
    # the bf16 grids at 2x and 4x hold more workgroups than tiles
    assert 2 * g2 > R.WALK_TILES[8, 32] and k["X6_OCC_MAX"] == 4


# ------------------------------------------------------------------ integer data
def _is_int(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("cin,cout", R.PAIRS, ids=lambda v: str(v))
def test_integer_cases_are_exact(cin, cout):
    """The conditions of conv3x3_ref.int_case, for every shape of the tables:
    integers (act(x) too, the prologue exact in fp32), every sum of |products|
    below 2^24 -- so every partial sum in any order is exact in fp32 --, all
    operands and (thin) every |y| <= 256 exact in bf16, and the float32 torch
    evaluation already equal to the float64 one."""
    for N, H, W in R.shapes():
        for thin in (False, True):
            c = R.int_case(cin, cout, N, H, W, thin)
            x, w, b, sc, sh, dy = (c[k] for k in ("x", "w", "bias", "scale", "shift", "dy"))
            tag = (N, H, W, thin)
            assert all(_is_int(t) for t in (x, w, b, sh, dy)), tag
            assert float(x.abs().max()) <= 3 and float(dy.abs().max()) <= 2, tag
            assert set(sc.tolist()) <= {0.5, 1.0, 2.0}, tag
            a32 = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))      # fp32
            a64 = R.act(x.double(), sc, sh)
            assert torch.equal(a32.double(), a64) and _is_int(a64), tag
            assert torch.equal(R.act(x.double(), sc, sh, fp32_fma=True), a64), tag
            for t in (x, a32, w, b, dy):                      # exact in bf16
                assert torch.equal(t.bfloat16().float(), t), tag
            bounds = [float(F.conv2d(a.abs(), w.double().abs(), b.double().abs(),
                                     padding=1).max()) for a in (x.double(), a64)]
            bounds.append(float(torch.nn.grad.conv2d_input(x.shape, w.double().abs(),
                                                           dy.double().abs(), padding=1).max()))
            bounds += [float(torch.nn.grad.conv2d_weight(a.abs(), w.shape, dy.double().abs(),
                                                         padding=1).max())
                       for a in (x.double(), a64)]
            bounds.append(float(dy.abs().sum((0, 2, 3)).max()))
            assert max(bounds) < TWO24, (tag, bounds)
            if thin:
                assert max(bounds[:2]) <= 256, (tag, bounds)
            for pro in (True, False):
                r = R.int_refs(cin, cout, N, H, W, thin, pro)
                s_, h_ = (sc, sh) if pro else (None, None)
                y32, _ = R.fwd_ref(x, w, b, s_, h_, dtype=torch.float32)
                dw32, db32 = R.wgrad_ref(x, dy, s_, h_, dtype=torch.float32)
                assert y32.dtype == torch.float32 and torch.equal(y32.double(), r["y"]), tag
                assert torch.equal(dw32.double(), r["dw"]) and torch.equal(db32.double(), r["db"]), tag
                if thin:
                    assert float(r["y"].abs().max()) <= 256, tag
            dx32 = R.dgrad_ref(dy, w, dtype=torch.float32)
            assert torch.equal(dx32.double(), R.int_refs(cin, cout, N, H, W, thin, True)["dx"]), tag


@pytest.mark.parametrize("cin,cout", R.PAIRS, ids=lambda v: str(v))
def test_real_cases_keep_their_sums_away_from_cancellation(cin, cout):
    """|sum y| >= 0.1 sum |y| per channel (and the same of dy): the BatchNorm
    sums and the bias gradient are checked relative to their own value."""
    for N, H, W in R.shapes(R.REAL_PLANES):
        c = R.real_case(cin, cout, N, H, W)
        dy = c["dy"].double()
        assert bool((dy.sum((0, 2, 3)).abs() >= 0.1 * dy.abs().sum((0, 2, 3))).all()), (N, H, W)
        for pro in (True, False):
            for b16 in ((False, True) if (cin, cout) in R.X6_MODEL_PAIRS else (False,)):
                s_, h_ = (c["scale"], c["shift"]) if pro else (None, None)
                y, sums = R.fwd_ref(c["x"], c["w"], c["bias"], s_, h_, bf16=b16)
                assert bool((sums[:cout].abs() >= 0.1 * y.abs().sum((0, 2, 3))).all()), (N, H, W, pro)


# ------------------------------------------------------------------ routes
@pytest.fixture(scope="module")
def route_names(tmp_path_factory):
    exe = tmp_path_factory.mktemp("route") / "conv3x3_route_names"
    src = R.os.path.join(R.ROOT, "tests", "conv3x3_route_names.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), src], check=True)

    def run(lines):
        text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
        rows = [ln.split() for ln in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return [dict(name=r[0], refuse=int(r[1]), fast=int(r[2]), dg8=int(r[3]), two_pass=int(r[4]),
                     grid=tuple(int(v) for v in r[5:8]), rows=int(r[8])) for r in rows]
    return run


def _lines(bits, cin, cout, prec, shp):
    out = []
    for op, N, H, W, flags, pro in R.calls(cin, cout, prec, shp):
        flags |= 1024 if pro else 0
        starts = [c0 for c0, _ in R.wgrad_passes(cin)] if op == "wgrad" else [0]
        out += [(bits, op, N, cin, cout, H, W, flags, c0) for c0 in starts]
    return out


def test_case_tables_reach_every_kernel(route_names):
    """The launches of test_gpu_conv3x3_edges.py -- the default environment,
    the per-call switch AINP_SMALL_WGRAD_TILE=1 and the child environments --
    run every forward / data-gradient kernel and every weight-gradient kernel
    of conv_route.h, the exact kernel with both stagings, the tiled split-bf16
    kernel with both tile heights, and the two-pass fused data gradient."""
    lines = []
    for cin, cout in R.PAIRS:
        for prec in R.PRECISIONS:
            lines += _lines(0, cin, cout, prec, R.shapes())
    for cin, cout in R.SMALL_CL_PAIRS:
        lines += [ln for ln in _lines(R.ENV_BITS["small_wgrad_tile"], cin, cout, "fp32", R.shapes())
                  if ln[1] == "wgrad"]
    default_n = len(lines)
    for var, val, bits, pairs, precs in R.CHILD_SETTINGS.values():
        for cin, cout in pairs:
            for prec in precs:
                lines += _lines(bits, cin, cout, prec, R.shapes(R.CHILD_PLANES))
    res = route_names(lines)
    served = [(ln, r) for ln, r in zip(lines, res) if r["refuse"] == 0]
    conv = [(ln, r) for ln, r in served if ln[1] != "wgrad"]
    wg = [(ln, r) for ln, r in served if ln[1] == "wgrad"]
    conv_names = {r["name"] for _, r in conv}
    wg_names = {r["name"] for _, r in wg}
    ck, wk = R.route_enum("ConvKernel"), R.route_enum("WgradKernel")
    assert len(ck) == 10 and len(wk) == 9
    assert conv_names == {"rows_16to1", "rows_1to16", "small_tile", "exact", "x6p", "x6q",
                          "x6_tiled", "fwd_b16dma", "dgrad_b16dma"} and len(conv_names) == len(ck) - 1
    assert wg_names == {"strip_cl", "strip", "small_tile", "x6s", "x6", "wgrad_b16dma", "wgrad_t",
                        "wgrad_mfma"} and len(wg_names) == len(wk) - 1
    assert {r["fast"] for _, r in conv if r["name"] == "exact"} == {0, 1}
    assert {r["dg8"] for _, r in conv if r["name"] == "x6_tiled"} == {0, 1}
    assert any(r["two_pass"] for _, r in conv)
    # the default environment alone reaches all but what the switches are for
    d_conv = {(r["name"], r["dg8"]) for ln, r in served[:] if ln[0] == 0 and ln[1] != "wgrad"}
    assert ("x6_tiled", 0) in d_conv and ("x6_tiled", 1) in d_conv
    assert default_n < len(lines)
    by_env = {}
    for ln, r in served:
        by_env.setdefault(ln[0], set()).add((ln[1] == "wgrad", ln[3], ln[4], r["name"]))
    B = R.ENV_BITS
    # AINP_CONV_EXACT=1: the model's pairs on the exact kernel and wgrad_t
    for pair in R.X6_MODEL_PAIRS:
        assert (False, *pair, "exact") in by_env[B["exact"]]
    for pair in ((16, 32), (32, 16), (32, 64)):
        assert (True, *pair, "wgrad_t") in by_env[B["exact"]]
    assert not any(n[3] in ("x6p", "x6q", "x6_tiled", "x6s", "x6") for n in by_env[B["exact"]])
    # AINP_CONV_X6_TILED: the 16-row forward of (32, 64)
    assert any(ln[0] == B["x6_tiled"] and ln[1] == "fwd" and (ln[3], ln[4]) == (32, 64) and
               r["name"] == "x6_tiled" and not r["dg8"] for ln, r in served)
    assert not any(n[3] in ("x6p", "x6q") for n in by_env[B["x6_tiled"]])
    # AINP_SMALL_ROWS=0: channel-last small pairs on the 8 x 48 tile kernel
    small = {ln[7] & (R.XCL | R.YCL) for ln, r in served if ln[0] == B["small_rows0"] and
             ln[1] in ("fwd", "dgrad") and r["name"] == "small_tile"}
    assert small == {0, R.XCL, R.YCL, R.XCL | R.YCL}
    assert not any(n[3].startswith("rows_") for n in by_env[B["small_rows0"]])
    # AINP_DGRAD_BNR=0: every fused call takes the two passes
    assert all(r["two_pass"] for ln, r in served if ln[0] == B["dgrad_bnr0"] and ln[1] == "bnr")
    # the register-staged bf16 channel-last kernels
    both = R.XCL | R.YCL
    assert all(r["name"] == "x6p" for ln, r in served if ln[0] == B["conv16_dma0"] and
               ln[1] == "fwd" and ln[7] & both == both)
    assert all(r["name"] == "x6_tiled" and r["dg8"] for ln, r in served
               if ln[0] == B["dgrad16_dma0"] and ln[1] in ("dgrad", "bnr") and ln[7] & both == both)
    assert all(r["name"] == "x6" for ln, r in served if ln[0] == B["wgrad16_dma0"] and
               ln[1] == "wgrad")
    # AINP_X6_OCC16: the bf16 persistent grids at 2x and 4x
    for key, mult in (("occ2", 2), ("occ4", 4)):
        grids = {r["grid"][0] for ln, r in served if ln[0] == B[key] and
                 r["name"] in ("x6p", "x6q", "fwd_b16dma", "x6s", "x6")}
        assert grids == {256 * mult, 512 * mult}, grids
    # the reference's own idea of which calls round to bf16 is the table's
    x6 = ("x6p", "x6q", "x6_tiled", "fwd_b16dma", "dgrad_b16dma")
    for ln, r in zip(lines[:default_n], res[:default_n]):
        if ln[0] or r["refuse"]:
            continue
        if ln[1] == "fwd":
            assert (r["name"] in x6) == R.conv_is_x6(ln[3], ln[4]), ln
        elif ln[1] == "dgrad":
            assert (r["name"] in x6) == R.conv_is_x6(ln[4], ln[3]), ln
        elif ln[1] == "wgrad" and not R.small_pair(ln[3], ln[4]):
            cp = min(32, ln[3] - ln[8])
            assert (r["name"] in ("x6s", "x6", "wgrad_b16dma")) == R.wgrad_pass_is_x6(cp, ln[4]), ln
    # the model's bf16 configuration: nothing is refused but [C][H][N][W] off 32 -> 16
    for ln, r in zip(lines[:default_n], res[:default_n]):
        if ln[0] == 0 and (ln[3], ln[4]) in ((16, 32), (32, 16), (32, 64)):
            cfnt_off = bool(ln[7] & R.YCFNT) and (ln[3], ln[4]) != (16, 32)
            assert (r["refuse"] != 0) == cfnt_off, ln
    # 18 of 32 output channels: x6p in NCHW; a channel-last output (four channels
    # per store) is refused, never routed to a split-bf16 kernel
    cl16 = R.route_enum("ConvRefusal").index("CR_CL16")
    seen = set()
    for ln, r in zip(lines[:default_n], res[:default_n]):
        conv = (ln[3], ln[4]) if ln[1] == "fwd" else (ln[4], ln[3]) if ln[1] == "dgrad" else None
        if ln[0] == 0 and conv == (16, 18):
            if ln[7] & R.YCL:
                assert r["refuse"] == cl16, ln
            elif not ln[7] & (R.YCFNT | R.X16 | R.DY16 | R.Y16):
                assert r["name"] == "x6p" and not r["refuse"], ln
                seen.add(ln[1])
    assert seen == {"fwd", "dgrad"}
    for ln, r in zip(lines, res):      # no split-bf16 kernel writes a channel-last Cout % 4 != 0
        if ln[1] in ("fwd", "dgrad", "bnr") and not r["refuse"] and ln[7] & R.YCL:
            cout = ln[4] if ln[1] == "fwd" else ln[3]
            assert cout % 4 == 0 or r["name"] in ("small_tile", "rows_16to1"), ln
    # mixed-kernel and multi-pass weight gradients (default environment, fp32)
    passes = {}
    for ln, r in zip(lines[:default_n], res[:default_n]):
        if ln[1] == "wgrad" and ln[7] == 1024 and ln[0] == 0 and (ln[2], ln[5], ln[6]) == (1, 9, 33):
            passes.setdefault((ln[3], ln[4]), []).append(r["name"])
    assert passes[48, 16] == ["x6s", "wgrad_t"] and passes[33, 64] == ["x6", "wgrad_mfma"]
    assert passes[64, 16] == ["x6s", "x6s"] and passes[64, 64] == ["x6", "x6"]
    assert passes[40, 32] == ["wgrad_t", "wgrad_mfma"]


def test_refusal_texts_parse():
    t = R.refusal_texts()
    assert set(t) == set(R.route_enum("ConvRefusal")) - {"CR_OK"}
    assert all(t.values()) and "AINP_CONV_YCFNT" in t["CR_CFNT"]
