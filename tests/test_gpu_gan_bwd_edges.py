"""Direct tests of the generator-backward kernels (csrc/gan_bwd.hip through
their ainp.ops wrappers) that test_gpu_gan_glue.py does not cover:
bn_act_bwd_reduce / bn_act_bwd_apply, gen_act_bwd, pconv_src_materialize /
pconv_src_grad, maxpool2_bwd, absdiff_grad, gram_sign_sym and gan_recon_bwd,
each against the float64 restatement of its contract in tests/gan_bwd_ref.py
(pinned to torch autograd, with the conditions on the inputs, in
test_cpu_gan_bwd_ref.py), element by element, at the shapes where the tiling
changes and in every mode of the wrappers.

Bounds, as in test_gpu_gan_glue.py.  Copies, selections and pure sign outputs:
torch.equal with the float32 torch evaluation.  Everything else: the
element-wise rule gan_glue_ref.within_floor (the largest deviation from
float64 at most 4 x that of the float32 torch evaluation of the same
reference plus 4e-7 of the reference's largest magnitude).  dgamma / dbeta:
1e-6 relative per element.  The padding [P, ldo) of a row: exactly 0; the
wrappers allocate gc themselves, so every padded element is looked at, and
buffers a caller passes in start from NaN.  Each check of the floor rule
prints what it measured; DESIGN.md ("Edge-shape tests") keeps the largest.
"""
import pytest
import torch

import gan_bwd_ref as B
import gan_glue_ref as R

pytestmark = pytest.mark.gpu

D = torch.float64


@pytest.fixture(scope="module")
def ops():
    from ainp import ops as _ops
    return _ops


def dv(t):
    return None if t is None else t.float().cuda().contiguous()


def each_ok(got, ref, tol=1e-6):
    """Every element within tol of its own reference value."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= tol * ref.abs()).all())


def floor_ok(tag, got, ref64, ref32):
    dev, floor, ok = R.within_floor(got.cpu(), ref64, ref32)
    scale = float(ref64.abs().max())
    print(f"{tag}: dev {dev:.3e} floor {floor:.3e} max|ref| {scale:.3e}")
    return ok and bool(torch.isfinite(got).all())


def all_zero(t):
    return torch.equal(t.cpu(), torch.zeros(t.shape))


def nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda")


def test_ld4_is_the_models(ops):
    from ainp.gan import _ld4
    assert all(B.ld4(p) == _ld4(p) for p in range(1, 70))


# ------------------------------------------------ BatchNorm2d + LeakyReLU backward
def _bn_call(ops, shape, mode, with_gamma, with_ratio, ldo, count):
    """reduce + apply as ainp.gan runs them -> (sums, gc, dgamma, dbeta)."""
    c = B.bn_inputs(shape, mode, with_gamma)
    N, C, H, W = shape
    a = [dv(c[k]) for k in ("ga", "y", "scale", "shift", "save")]
    sums = ops.bn_act_bwd_reduce(*a, B.SLOPE, count=N * H * W if count == 0 else None)
    assert sums.dtype == D and sums.numel() == 2 * C + (1 if count == 0 else 0)
    gc, dgamma, dbeta = ops.bn_act_bwd_apply(*a, dv(c["gamma"]), sums, count, B.SLOPE,
                                             dv(c["ratio"]) if with_ratio else None, ldo)
    return sums, gc, dgamma, dbeta


def _bn_check(tag, out, shape, mode, with_gamma, with_ratio, ldo):
    N, C, H, W = shape
    P = H * W
    sums, gc, dgamma, dbeta = out
    (gc64, dg64, db64), (gc32, _, _) = B.bn_refs(shape, mode, with_gamma, with_ratio, ldo)
    assert gc.shape == (N, C, ldo)
    gc = gc.cpu()
    assert all_zero(gc[:, :, P:]), tag                               # the padding: exactly 0
    assert floor_ok(tag, gc[:, :, :P], gc64[:, :, :P], gc32[:, :, :P]), tag
    rel = lambda got, ref: float(((got.double().cpu() - ref).abs() / ref.abs()).max())  # noqa: E731
    print(f"{tag}: dbeta rel {rel(dbeta, db64):.3e} dgamma rel "
          f"{rel(sums[C:2 * C] if dgamma is None else dgamma, dg64):.3e}")
    assert each_ok(dbeta, db64) and each_ok(sums[:C], db64), tag
    assert each_ok(sums[C:2 * C], dg64), tag
    if with_gamma:
        assert each_ok(dgamma, dg64), tag
    else:
        assert dgamma is None


def _same_bits(x, y):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("shape", B.BN_PLANES, ids=str)
def test_bn_act_bwd_train(ops, shape):
    N, C, H, W = shape
    P = H * W
    for ldo in B.bn_ldos(P):
        out = _bn_call(ops, shape, "train", True, True, ldo, N * P)
        _bn_check(f"bn_act_bwd train {shape} ldo={ldo}", out, shape, "train", True, True, ldo)
        # fixed-order partial sums: a second call gives the same bits
        assert _same_bits(out, _bn_call(ops, shape, "train", True, True, ldo, N * P))


@pytest.mark.parametrize("shape", B.BN_MODE_PLANES, ids=str)
def test_bn_act_bwd_count_from_sums(ops, shape):
    """count = 0: the element count is sums[2C], as the SyncBN path leaves it."""
    N, C, H, W = shape
    P = H * W
    for ldo in B.bn_ldos(P):
        out = _bn_call(ops, shape, "train", True, True, ldo, 0)
        assert float(out[0][2 * C]) == N * P
        _bn_check(f"bn_act_bwd count=0 {shape} ldo={ldo}", out, shape, "train", True, True, ldo)
        given = _bn_call(ops, shape, "train", True, True, ldo, N * P)
        assert torch.equal(out[0][:2 * C], given[0]) and _same_bits(out[1:], given[1:])


@pytest.mark.parametrize("shape", B.BN_MODE_PLANES, ids=str)
def test_bn_act_bwd_eval(ops, shape):
    """count = -1: running statistics, save = [running_mean | rsqrt(running_var + eps)]."""
    P = shape[2] * shape[3]
    for ldo in B.bn_ldos(P):
        out = _bn_call(ops, shape, "eval", True, True, ldo, -1)
        _bn_check(f"bn_act_bwd eval {shape} ldo={ldo}", out, shape, "eval", True, True, ldo)
        assert _same_bits(out, _bn_call(ops, shape, "eval", True, True, ldo, -1))


@pytest.mark.parametrize("with_gamma,with_ratio", [(False, True), (True, False), (False, False)],
                         ids=["gamma=None", "ratio=None", "both=None"])
def test_bn_act_bwd_without_gamma_or_ratio(ops, with_gamma, with_ratio):
    shape = B.BN_OPTION_PLANE
    N, C, H, W = shape
    P = H * W
    for ldo in B.bn_ldos(P):
        for mode, count in (("train", N * P), ("eval", -1)):
            out = _bn_call(ops, shape, mode, with_gamma, with_ratio, ldo, count)
            _bn_check(f"bn_act_bwd {mode} gamma={with_gamma} ratio={with_ratio} ldo={ldo}", out,
                      shape, mode, with_gamma, with_ratio, ldo)


# ------------------------------------------------------ activation + crop backward
@pytest.mark.parametrize("grid", B.ACT_GRIDS, ids=str)
@pytest.mark.parametrize("act", B.ACTS)
def test_gen_act_bwd(ops, act, grid):
    N, C, H, W, gH, gW = grid
    P = H * W
    c = B.act_inputs(act, grid)
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY, ops.ACT_TANH) == (0, 1, 2, 3)
    g, a, ratio = dv(c["g"]), dv(c["a"]), dv(c["ratio"])
    outside = torch.ones(H, W, dtype=torch.bool)
    outside[:gH, :gW] = False
    selection = act in (0, 1)                          # gz is g or 0, nothing is computed
    for ldo in (P, P + 3):
        for with_ratio in (True, False):
            (gz64, gc64), (gz32, gc32) = B.act_refs(act, grid, with_ratio, ldo)
            for want_gz in (True, False):
                tag = f"gen_act_bwd act={act} {grid} ldo={ldo} ratio={with_ratio} gz={want_gz}"
                gz, gc = ops.gen_act_bwd(g, a, act, B.SLOPE, ratio if with_ratio else None, H, W,
                                         ldo, want_gz=want_gz)
                assert gc.shape == (N, C, ldo)
                gc = gc.cpu()
                assert all_zero(gc[:, :, P:]), tag                       # the padding
                assert all_zero(gc[:, :, :P].reshape(N, C, H, W)[:, :, outside]), tag
                if selection and not with_ratio:
                    assert torch.equal(gc, gc32), tag
                else:
                    assert floor_ok(tag + " gc", gc, gc64, gc32), tag
                if not want_gz:
                    assert gz is None
                    continue
                assert gz.shape == (N, C, P)
                gz = gz.cpu()
                assert all_zero(gz.reshape(N, C, H, W)[:, :, outside]), tag   # outside the crop
                if selection:
                    assert torch.equal(gz, gz32), tag
                else:
                    assert floor_ok(tag + " gz", gz, gz64, gz32), tag
                if act in (1, 2):                      # a == 0 exactly: the <= 0 branch
                    at = gz.reshape(N, C, H, W)[:, :, :gH, :gW][c["planted"]]
                    gp = c["g"][c["planted"]]
                    assert torch.equal(at, gp * 0 if act == 1 else gp * B.SLOPE), tag


# --------------------------------------------------------- PartialConv sources
@pytest.mark.parametrize("factor", B.PCONV_FACTORS, ids=str)
@pytest.mark.parametrize("shape", B.PCONV_SHAPES, ids=str)
def test_pconv_src_materialize(ops, shape, factor):
    """A copy times a 0 / 1 mask: the bits of the float32 torch evaluation."""
    fy, fx = factor
    c = B.pconv_inputs(shape, factor)
    x0, m0, x1, m1 = c["x0"], c["m0"], c["x1"], c["m1"]
    Hin, Win = c["Hin"], c["Win"]
    for s0, s1 in (((x0, m0), (x1, m1)),          # two masked sources
                   ((x0, m0), None),              # no second source
                   ((x0, None), (x1, None)),      # no masks
                   ((x0, None), (x1, m1)), ((x0, m0), (x1, None)), ((x0, None), None)):
        got = ops.pconv_src_materialize(tuple(dv(t) for t in s0),
                                        None if s1 is None else tuple(dv(t) for t in s1), Hin, Win)
        want = B.pconv_src_materialize(s0[0], s0[1], *(s1 or (None, None)), fy, fx)
        assert got.shape == want.shape
        assert torch.equal(got.cpu(), want), (s0[1] is None, s1 is None)


@pytest.mark.parametrize("factor", B.PCONV_FACTORS, ids=str)
@pytest.mark.parametrize("shape", B.PCONV_SHAPES, ids=str)
def test_pconv_src_grad(ops, shape, factor):
    N, C0, C1, Hs, Ws = shape
    fy, fx = factor
    c = B.pconv_inputs(shape, factor)
    Hin, Win = c["Hin"], c["Win"]
    dxin = dv(c["dxin"])
    c_off, C = B.PCONV_MID[shape]
    one = fy * fx == 1                              # no sum: a copy times the mask
    # (c_off, C, mask, fy, fx, what the buffer held: None = NaN and accumulate False)
    runs = [(0, C0, c["m0"], fy, fx, c["prev0"]),              # the upsampled source, accumulated
            (0, C0, c["m0"], fy, fx, None),
            (0, C0, None, fy, fx, None),                       # no mask
            (C0, C1, c["m1"], 1, 1, None),                     # the second source: c_off = C0
            (c_off, C, None, fy, fx, None),                    # a slice from the middle of Cin
            (c_off, C, c["m0"], fy, fx, c["prev_mid"])]
    for off, Cs, ms, ry, rx, prev in runs:
        hs, ws = Hin // ry, Win // rx
        tag = f"pconv_src_grad {shape} x{factor} c_off={off} C={Cs} mask={ms is not None} " \
              f"accumulate={prev is not None}"
        buf = nan_like((N, Cs, hs, ws)) if prev is None else dv(prev)
        out = ops.pconv_src_grad(dxin, off, dv(ms), buf, prev is not None)
        assert out is buf
        cast = lambda t, dt: None if t is None else t.to(dt)  # noqa: E731
        ref = {dt: B.pconv_src_grad(c["dxin"].to(dt), off, Cs, cast(ms, dt), ry, rx, cast(prev, dt))
               for dt in (D, torch.float32)}
        if prev is None and (one or (ry, rx) == (1, 1)):
            assert torch.equal(buf.cpu(), ref[torch.float32]), tag
        else:
            assert floor_ok(tag, buf, ref[D], ref[torch.float32]), tag


# --------------------------------------------------------- MaxPool2d(2, 2) backward
@pytest.mark.parametrize("shape", B.MAXPOOL_SHAPES, ids=str)
def test_maxpool2_bwd(ops, shape):
    """torch's CPU rule: the first maximum of a window, the last NaN if it has any."""
    N, C, H, W = shape
    if shape == (1, 1, 2, 2):                       # one window: each planted one in turn
        g = torch.tensor([[[[7.0]]]])
        for w, idx in B.MAXPOOL_WINDOWS:
            x = B.window_tensor(w).reshape(1, 1, 2, 2)
            got = ops.maxpool2_bwd(dv(g), dv(x)).cpu()
            assert torch.equal(got, B.maxpool2_autograd(g, x)), (w, got.reshape(4).tolist())
            assert float(got.reshape(4)[idx]) == 7.0
    c = B.maxpool_inputs(shape)
    got = ops.maxpool2_bwd(dv(c["g"]), dv(c["x"])).cpu()
    want = B.maxpool2_autograd(c["g"], c["x"])
    for n, ch, oy, ox, idx in c["planted"]:
        win = (slice(n, n + 1), slice(ch, ch + 1), slice(2 * oy, 2 * oy + 2), slice(2 * ox, 2 * ox + 2))
        assert torch.equal(got[win], want[win]), (B.MAXPOOL_WINDOWS[c["planted"].index(
            (n, ch, oy, ox, idx))], got[win].reshape(4).tolist())
    assert torch.equal(got, want)
    assert all_zero(got[:, :, 2 * (H // 2):]) and all_zero(got[:, :, :, 2 * (W // 2):])   # odd H, W


# ----------------------------------------------------------------- sign gradients
@pytest.mark.parametrize("n", B.ABSDIFF_NS)
def test_absdiff_grad(ops, n):
    forms = [B.absdiff_inputs(n)] + ([B.absdiff_inputs(1, True)] if n == 1 else [])
    for c in forms:
        a, b, ties, scale = c["a"], c["b"], c["ties"], c["scale"]
        for gs in (None, c["gs"]):
            tag = f"absdiff_grad n={n} gscale={gs is not None} ties={int(ties.sum())}"
            # accumulate=False: sign * scale * gs in the kernel's order, exactly
            want = B.absdiff_grad(a, b, gs, scale)
            out = nan_like((n,))
            got = ops.absdiff_grad(dv(a), dv(b), dv(gs), scale, out=out, accumulate=False)
            assert got is out and torch.equal(out.cpu(), want), tag
            assert torch.equal(ops.absdiff_grad(dv(a), dv(b), dv(gs), scale).cpu(), want), tag
            assert all_zero(out[ties.cuda()]), tag
            # accumulate=True onto random contents
            prev = c["prev"]
            out = dv(prev)
            ops.absdiff_grad(dv(a), dv(b), dv(gs), scale, out=out, accumulate=True)
            g64 = None if gs is None else gs.double()
            assert floor_ok(tag + " accumulate", out, B.absdiff_grad(a.double(), b.double(), g64, scale,
                                                                   prev.double()),
                            B.absdiff_grad(a, b, gs, scale, prev)), tag
            assert torch.equal(out.cpu()[ties], prev[ties]), tag         # a tie adds nothing


@pytest.mark.parametrize("shape", B.GRAM_SHAPES, ids=str)
def test_gram_sign_sym(ops, shape):
    Bn, C = shape
    c = B.gram_inputs(Bn, C)
    Ga, Gb, scale = c["Ga"], c["Gb"], c["scale"]
    diag = torch.eye(C, dtype=torch.bool).expand(Bn, C, C)
    for gs in (None, c["gs"]):
        got = ops.gram_sign_sym(dv(Ga), dv(Gb), dv(gs), scale).cpu()
        want = B.gram_sign_sym(Ga, Gb, gs, scale)                       # float32, the kernel's order
        assert got.shape == (Bn, C, C)
        assert torch.equal(got, want), (shape, gs)
        assert torch.equal(got, got.transpose(1, 2))                    # its own transpose
        d = torch.sign(Ga - Gb) * 2 * scale
        assert torch.equal(got[diag], (d if gs is None else d * gs)[diag])
        assert all_zero(got[c["zeros"] & diag])


@pytest.mark.parametrize("mask", B.RECON_MASKS)
@pytest.mark.parametrize("n", B.RECON_NS)
def test_gan_recon_bwd(ops, n, mask):
    forms = [B.recon_inputs(n, mask)] + ([B.recon_inputs(1, mask + "+tie")] if n == 1 else [])
    for c in forms:
        g, o, m, gout, ties = c["g"], c["o"], c["m"], c["gout"], c["ties"]
        dev_sums = ops.gan_recon_sums(dv(g), dv(o), dv(m))
        ref_sums = B.recon_sums(g.double(), o.double(), m.double())
        assert dev_sums.dtype == D and each_ok(dev_sums, ref_sums)
        # the forward's own sums, then once the float64 reference's: the two
        # kernels apart.  n_total = 3 n: a data-parallel rank's share
        for sums, n_total in ((dev_sums, n), (dev_sums, 3 * n), (ref_sums.cuda(), n)):
            tag = f"gan_recon_bwd n={n} {mask} n_total={n_total} ties={int(ties.sum())}" \
                  f"{' ref sums' if sums is not dev_sums else ''}"
            got = ops.gan_recon_bwd(dv(g), dv(o), dv(m), sums, dv(gout), n_total)
            s = sums.cpu()
            r64 = B.gan_recon_bwd(g.double(), o.double(), m.double(), s, gout.double(), float(n_total))
            r32 = B.gan_recon_bwd(g, o, m, s, gout, float(n_total))
            assert got.shape == g.shape
            assert floor_ok(tag, got, r64, r32), tag
            assert all_zero(got[ties.cuda()]), tag                       # g == o: no gradient
