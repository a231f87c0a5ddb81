"""Direct tests of the GAN's small kernels (csrc/gan.hip, gan_bwd.hip, bn.hip,
loss.hip through their ainp.ops wrappers), which the Discriminator / VGGLoss /
GanTrainer goldens reach only at the fixture shapes: each op against a plain
float64 torch evaluation (tests/gan_glue_ref.py for the spectral norm, pinned
to torch.nn.utils.spectral_norm in test_cpu_gan_glue_ref.py; oracle/gan_ref.py
for the VGG input), at the smallest shapes that reach every tail.  Of
gan_bwd.hip this file holds vgg_prep_bwd, conv_weight_flip_t and
affine_leaky_out; that file's remaining ops (BatchNorm + LeakyReLU backward,
activation + crop backward, the PartialConv sources, maxpool2_bwd and the sign
gradients) are in tests/test_gpu_gan_bwd_edges.py, under the same bounds.

Bounds.  Copies, selections and maxima: torch.equal with the float32 torch
result.  Reduced scalars: 1e-6 relative (as test_l1_pow10_loss,
test_absdiff_mean_matches_fp64).  Tensors: 1e-5 relative L2, and where one
wrong element could hide in a norm the element-wise rule of
test_gpu_lstm_edges.py (gan_glue_ref.within_floor): the largest deviation from
float64 may be 4 x that of the float32 torch evaluation of the same reference
plus 4e-7 of the reference's largest magnitude.  Tests of that kind print what
they measured; DESIGN.md ("Edge-shape tests") keeps the largest.
"""
import pytest
import torch
import torch.nn.functional as F

import gan_glue_ref as R
from oracle import gan_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from ainp import ops as _ops
    return _ops


def dv(t):
    return t.float().cuda().contiguous()


def rel_l2(got, ref):
    ref = ref.double().cpu()
    return float(torch.linalg.vector_norm(got.double().cpu() - ref)
                 / torch.linalg.vector_norm(ref).clamp_min(1e-300))


def scalar_ok(got, ref, tol=1e-6):
    """|got - ref| <= tol |ref|; a reference of exactly 0 must come out 0."""
    got, ref = float(got), float(ref)
    return got == got and abs(got - ref) <= tol * abs(ref)


def each_ok(got, ref, tol=1e-6):
    """Every element within tol of its own reference value."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= tol * ref.abs()).all())


def floor_ok(tag, got, ref64, ref32):
    dev, floor, ok = R.within_floor(got.cpu(), ref64, ref32)
    scale = float(ref64.abs().max())
    print(f"{tag}: dev {dev:.3e} floor {floor:.3e} max|ref| {scale:.3e}")
    return ok


# ------------------------------------------------------------ spectral norm
# (h, wd): h = 1, 3, 5, 13 mod 16 for the row remainder loop; h = 16, where
# the 16-row unrolled loop runs exactly once in wave 0 and not at all in the
# others; h = 17; wd below, at, just above and far above the 64-column tile
SN_LAYERS = [(1, 1024), (3, 5), (5, 3), (13, 70), (16, 64), (17, 65), (33, 129), (64, 513)]


def _sn_layers(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    Ws, us, vs = [], [], []
    for h, wd in shapes:
        Ws.append(torch.randn(h, wd, generator=g))
        us.append(R.normalize(torch.randn(h, generator=g)))
        vs.append(R.normalize(torch.randn(wd, generator=g)))
    return Ws, us, vs


def _sn_stage(ops, tag, Wd, ud, vd, Ws, update):
    """One ops.sn_power call against the reference started from the vectors
    the call itself started from (what the previous call left on the device)."""
    u_in = [u.cpu().clone() for u in ud]
    v_in = [v.cpu().clone() for v in vd]
    inv = ops.sn_power(Wd, ud, vd, update=update).cpu()
    bad = []
    for l, W in enumerate(Ws):
        u64, v64, s64 = R.sn_power(W.double(), u_in[l].double(), v_in[l].double(), update)
        u32, v32, _ = R.sn_power(W, u_in[l], v_in[l], update)
        u, v = ud[l].cpu(), vd[l].cpu()
        name = f"sn_power {tag} layer {tuple(W.shape)}"
        if update:
            ok = floor_ok(name + " u", u, u64, u32) and floor_ok(name + " v", v, v64, v32)
            ok = ok and rel_l2(u, u64) <= 1e-5 and rel_l2(v, v64) <= 1e-5
        else:
            ok = torch.equal(u, u_in[l]) and torch.equal(v, v_in[l])      # untouched
        e = abs(float(inv[l]) * float(s64) - 1.0)
        print(f"{name} inv_sigma rel {e:.3e}")
        if not (ok and e <= 1e-6):
            bad.append((name, e))
    assert not bad, bad


def test_sn_power_eight_layers(ops):
    Ws, us, vs = _sn_layers(SN_LAYERS, seed=1)
    Wd = [dv(W) for W in Ws]
    Wd[4] = Wd[4].view(16, 4, 4, 4)         # conv weights as the discriminator passes them
    Wd[7] = Wd[7].view(64, 57, 3, 3)
    ud, vd = [dv(u) for u in us], [dv(v) for v in vs]
    _sn_stage(ops, "update 1", Wd, ud, vd, Ws, True)
    _sn_stage(ops, "update 2", Wd, ud, vd, Ws, True)
    _sn_stage(ops, "eval", Wd, ud, vd, Ws, False)


@pytest.mark.parametrize("shape", [(17, 65), (1, 1024)])
def test_sn_power_one_layer(ops, shape):
    Ws, us, vs = _sn_layers([shape], seed=2)
    Wd, ud, vd = [dv(Ws[0])], [dv(us[0])], [dv(vs[0])]
    _sn_stage(ops, "nl=1 update", Wd, ud, vd, Ws, True)
    _sn_stage(ops, "nl=1 eval", Wd, ud, vd, Ws, False)


@pytest.mark.parametrize("extra", [0, 1, 4], ids=["ld=wd", "ld=wd+1,bias", "ld=wd+4"])
@pytest.mark.parametrize("h,wd", [(1, 1024), (13, 70), (64, 513), (3, 5)])
def test_sn_weight_grad(ops, h, wd, extra):
    """G [h, ld] with ld = wd, wd + 1 (the bias column: dbias = G[:, wd]
    exactly) and wd + 4.  The wrapper wants a contiguous G and takes ld from
    its row length, so the last is the whole wider buffer, its four extra
    columns at 1e30: a read past wd shows."""
    g = torch.Generator().manual_seed(h * wd + extra)
    W = torch.randn(h, wd, generator=g)
    G = torch.randn(h, wd + extra, generator=g)
    if extra == 4:
        G[:, wd:] = 1e30
    # u, v as two power iterations leave them (sigma near the largest singular value)
    u = R.normalize(torch.randn(h, generator=g).double())
    v = R.normalize(torch.randn(wd, generator=g).double())
    for _ in range(2):
        u, v, _ = R.sn_power(W.double(), u, v, True)
    u, v = u.float(), v.float()
    sigma = torch.dot(u.double(), W.double() @ v.double())
    inv = (1.0 / sigma).float().reshape(1)
    out, db = ops.sn_weight_grad(dv(G), dv(W), dv(u), dv(v), inv.cuda(), with_bias=(extra == 1))
    out = out.cpu()
    ref64 = R.sn_weight_grad(G[:, :wd].double(), W.double(), u.double(), v.double())
    ref32 = R.sn_weight_grad(G[:, :wd].contiguous(), W, u, v)
    assert out.shape == W.shape and torch.isfinite(out).all()
    assert floor_ok(f"sn_weight_grad ({h},{wd}) ld=wd+{extra}", out, ref64, ref32)
    assert rel_l2(out, ref64) <= 1e-5
    if extra == 1:
        assert torch.equal(db.cpu(), G[:, wd])
    else:
        assert db is None


# ------------------------------------------------------------------- losses
# kRedBlocks = 512 blocks of 256 threads (csrc/gan.hip): 131072 elements per
# pass of the grid-stride loop; 131589 gives every block a second pass, partly
BCE_NS = [1, 63, 257, 4097, 131589]
PLANTED = [0.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0]


@pytest.mark.parametrize("target", [1.0, 0.0, 0.9])
@pytest.mark.parametrize("n", BCE_NS)
def test_bce_logits(ops, n, target):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3
    if n >= 63:
        x[torch.randperm(n, generator=g)[:len(PLANTED)]] = torch.tensor(PLANTED)
    xd = dv(x)
    x64 = x.double()
    ref = F.binary_cross_entropy_with_logits(x64, torch.full_like(x64, target))
    for gs in (None, 0.37):
        loss, grad = ops.bce_logits(xd, target, want_grad=True, grad_scale=gs)
        assert loss.dtype == torch.float64 and loss.dim() == 0
        e = abs(float(loss) - float(ref)) / float(ref)
        print(f"bce_logits n={n} target={target}: mean {float(loss):.9e} ref {float(ref):.9e} rel {e:.3e}")
        assert scalar_ok(loss, ref)
        scale = 1.0 / n if gs is None else gs
        g64 = scale * (torch.sigmoid(x64) - target)
        g32 = torch.tensor(scale, dtype=torch.float32) * (torch.sigmoid(x) - target)
        assert torch.isfinite(grad).all()
        assert floor_ok(f"bce_logits grad n={n} target={target} scale={gs}", grad, g64, g32)
        assert rel_l2(grad, g64) <= 1e-5
        only, none = ops.bce_logits(xd, target, want_grad=False, grad_scale=gs)
        assert none is None and torch.equal(only, loss)


def _recon_ref(g, o, m):
    """calculate_losses' reconstruction terms and the five sums behind them, fp64."""
    g, o, m = g.double(), o.double(), m.double()
    h = 1 - m
    sums = torch.stack([(g * m - o * m).abs().sum(), m.sum(), (g * h - o * h).abs().sum(), h.sum(),
                        ((g - o).abs() * o.abs()).sum()])
    lv = sums[0] / (sums[1] + 1e-8)
    lh = sums[2] / (sums[3] + 1e-8)
    lw = torch.mean((g - o).abs() * o.abs())
    return torch.stack([lv, lh, lw]), sums


@pytest.mark.parametrize("mask", ["random", "ones", "zeros"])
@pytest.mark.parametrize("n", [1, 1003, 70001])
def test_gan_recon_losses_and_sums(ops, n, mask):
    gen = torch.Generator().manual_seed(n)
    g = torch.tanh(torch.randn(n, generator=gen))
    o = torch.rand(n, generator=gen) * 3
    m = {"random": (torch.rand(n, generator=gen) > 0.4).float(), "ones": torch.ones(n),
         "zeros": torch.zeros(n)}[mask]
    ref, ref_sums = _recon_ref(g, o, m)
    got = ops.gan_recon_losses(dv(g), dv(o), dv(m)).cpu()
    sums = ops.gan_recon_sums(dv(g), dv(o), dv(m))
    from_sums = ops.gan_recon_from_sums(sums, n).cpu()
    print(f"gan_recon n={n} {mask}: got {got.tolist()} ref {ref.tolist()}")
    assert got.dtype == torch.float64 and torch.isfinite(got).all()     # no hole: 0, not NaN
    for q in range(3):
        assert scalar_ok(got[q], ref[q]), (q, float(got[q]), float(ref[q]))
        assert scalar_ok(from_sums[q], got[q]), (q, float(from_sums[q]), float(got[q]))
        assert scalar_ok(from_sums[q], ref[q])
    for q in range(5):
        assert scalar_ok(sums[q], ref_sums[q]), (q, float(sums[q]), float(ref_sums[q]))
    if mask == "ones":
        assert float(got[1]) == 0.0 and float(from_sums[1]) == 0.0
    if mask == "zeros":
        assert float(got[0]) == 0.0 and float(from_sums[0]) == 0.0


# ---------------------------------------------------------------- VGG input
def _tables(ops, H, W, S=224, short=256):
    """The separable resize tables as VGGLoss._prep_tables builds them."""
    nh, nw = gan_ref.resized_size(H, W, short)
    top, left = int(round((nh - S) / 2.0)), int(round((nw - S) / 2.0))
    t = ops.aa_bilinear_weights(H, nh, top, S) + ops.aa_bilinear_weights(W, nw, left, S)
    return tuple(torch.from_numpy(a).cuda() for a in t)


# upsampling (one or two taps per output pixel), the crop's own size, and a
# non-integer downsampling in both axes.  The reference is the oracle in
# float32, as in test_vgg_prepare_matches_oracle: torch computes the resize
# weights in float32, the kernel's tables repeat that arithmetic, and at
# (300, 233) those weights alone put the float32 oracle 5e-5 from its float64
# evaluation.  Against float64 the element-wise floor rule holds instead.
@pytest.mark.parametrize("H,W", [(37, 50), (224, 224), (300, 233)])
def test_vgg_prep_forward(ops, H, W):
    N = 3
    g = torch.Generator().manual_seed(H + W)
    gen = torch.rand(N, 1, H, W, generator=g) * 3 - 1.5         # both clamps of (x + 1) / 2 active
    tgt = torch.rand(N, 1, H, W, generator=g) * 4 - 0.5
    tables = _tables(ops, H, W)
    for x, is_gen in ((gen, True), (tgt, False)):
        got = ops.vgg_prep(dv(x), is_gen, tables).cpu()
        ref32 = gan_ref.vgg_prepare(x, is_gen)
        ref64 = gan_ref.vgg_prepare(x.double(), is_gen)
        d32 = float((got - ref32).abs().max())
        print(f"vgg_prep ({H},{W}) generated={is_gen}: vs the fp32 oracle {d32:.3e}")
        assert got.shape == (N, 3, 224, 224) and d32 < 2e-5
        assert floor_ok(f"vgg_prep ({H},{W}) generated={is_gen} vs fp64", got, ref64, ref32)


def test_vgg_prep_target_modes(ops):
    N, H, W = 3, 37, 50
    g = torch.Generator().manual_seed(21)
    tables = _tables(ops, H, W)
    # no positive sample: the batch maximum is 0, nothing is divided, every
    # pixel is (0 - mean_c) / std_c
    neg = -torch.rand(N, 1, H, W, generator=g) - 0.01
    got = ops.vgg_prep(dv(neg), False, tables).cpu()
    ref = gan_ref.vgg_prepare(neg, False)
    for c in range(3):
        mean, std = torch.tensor(gan_ref.IMAGENET_MEAN[c]), torch.tensor(gan_ref.IMAGENET_STD[c])
        want = (torch.tensor(0.0) - mean) / std
        assert torch.equal(got[:, c], want.expand(N, 224, 224)), c
    assert float((got - ref).abs().max()) < 2e-5
    # the maximum in the last element of the last image
    x = torch.rand(N, 1, H, W, generator=g) * 4 - 0.5
    x[-1, 0, -1, -1] = 9.0
    got = ops.vgg_prep(dv(x), False, tables)
    ref = gan_ref.vgg_prepare(x, False)
    assert float((got.cpu() - ref).abs().max()) < 2e-5
    # generated = 2: the precomputed (all-reduced) maximum
    mx = ops.vgg_target_max(dv(x))
    assert torch.equal(ops.vgg_prep(dv(x), False, tables, target_max=mx), got)


@pytest.mark.parametrize("n", [1, 65, 100003])
def test_vgg_target_max(ops, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 2
    cases = [x, -x.abs() - 0.5]
    if n > 1:
        last = x.clone()
        last[-1] = 7.5                       # the maximum in the last element
        cases.append(last)
    for t in cases:
        mx = ops.vgg_target_max(dv(t)).cpu()
        want = torch.clamp(t, min=0).max().reshape(1).view(torch.int32)
        assert mx.dtype == torch.int32 and torch.equal(mx, want)
    assert int(ops.vgg_target_max(dv(cases[1])).cpu()) == 0             # all negative


@pytest.mark.parametrize("H,W", [(37, 50), (129, 100)])
def test_vgg_prep_bwd(ops, H, W):
    N = 2
    g = torch.Generator().manual_seed(H * W)
    x = torch.rand(N, 1, H, W, generator=g) * 3 - 1.5
    # keep clear of the clamp edges x = -1, 1, so that fp32 and fp64 agree on
    # the side of every sample (a condition on the inputs, not a tolerance)
    x[(x.abs() - 1).abs() < 1e-4] = 0.5
    gout = torch.randn(N, 3, 224, 224, generator=g)
    got = ops.vgg_prep_bwd(dv(gout), dv(x), _tables(ops, H, W)).cpu()
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaf = x.to(dt).requires_grad_(True)
        gan_ref.vgg_prepare(leaf, True).backward(gout.to(dt))
        ref[dt] = leaf.grad
    out = x.abs() > 1
    assert int(out.sum()) > 100 and not ref[torch.float64][out].any()
    assert torch.equal(got[out], torch.zeros(int(out.sum())))           # clamped: exactly 0
    e = rel_l2(got, ref[torch.float64])
    print(f"vgg_prep_bwd ({H},{W}): rel L2 {e:.3e}")
    assert floor_ok(f"vgg_prep_bwd ({H},{W})", got, ref[torch.float64], ref[torch.float32])
    assert e <= 1e-5


# ------------------------------------------------------- element-wise glue
@pytest.mark.parametrize("n", [1, 1003])
def test_leaky_bwd_plain(ops, n):
    g = torch.Generator().manual_seed(n)
    gr, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n == 1:
        y[0] = 0.0
    else:
        y[3], y[4], y[n - 1] = 0.0, -0.0, 0.0
    want = torch.where(y > 0, gr, gr * 0.2)                   # y > 0 ? 1 : slope
    assert torch.equal(ops.leaky_bwd(dv(gr), dv(y), 0.2).cpu(), want)


@pytest.mark.parametrize("ldo", [36, 40])
def test_leaky_bwd_row_padded(ops, ldo):
    N, C, H, W = 2, 3, 5, 7
    g = torch.Generator().manual_seed(ldo)
    gr, y = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    y[0, 0, 0, 0], y[1, 2, 4, 6] = 0.0, -0.0
    got = ops.leaky_bwd(dv(gr), dv(y), 0.2, ldo=ldo).cpu()
    want = torch.where(y > 0, gr, gr * 0.2).view(N, C, H * W)
    assert got.shape == (N, C, ldo)
    assert torch.equal(got[:, :, :H * W], want)
    assert torch.equal(got[:, :, H * W:], torch.zeros(N, C, ldo - H * W))


@pytest.mark.parametrize("shape", [(2, 1, 3, 5), (2, 7, 3, 5), (1, 64, 9, 131)])
def test_channel_sum(ops, shape):
    """Mask planes: 0 / 1 and eighths in between, so that the sum over up to 64
    channels is exact in any order (a sequential fp32 sum of 64 arbitrary
    floats is itself only good to about 4e-6)."""
    g = torch.Generator().manual_seed(sum(shape))
    m = torch.randint(0, 9, shape, generator=g).float() / 8
    got = ops.channel_sum(dv(m)).cpu()
    assert got.shape == (shape[0], shape[2], shape[3])
    assert each_ok(got, m.double().sum(1))


@pytest.mark.parametrize("n", [1, 1003])
def test_mul_and_scale_by_scalar(ops, n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    assert torch.equal(ops.mul(dv(a), dv(b)).cpu(), a * b)
    s = torch.tensor(-1.7)
    assert torch.equal(ops.scale_by_scalar(dv(a), s.cuda()).cpu(), a * s)


# (H, W) -> (Hp, Wp): no padding, the largest reflect pad (H - 1, W - 1), a model-like one
@pytest.mark.parametrize("H,W,Hp,Wp", [(5, 7, 5, 7), (5, 7, 9, 13), (129, 100, 144, 112)])
def test_gan_pad_input(ops, H, W, Hp, Wp):
    N = 2
    g = torch.Generator().manual_seed(H + Wp)
    x = torch.randn(N, 1, H, W, generator=g)
    m = (torch.rand(N, 1, H, W, generator=g) > 0.3).float()
    xp, mp = ops.gan_pad_input(dv(x), dv(m), Hp, Wp)
    pad = (0, Wp - W, 0, Hp - H)
    assert torch.equal(xp.cpu(), F.pad(x, pad, mode="reflect")[:, 0])
    assert torch.equal(mp.cpu(), F.pad(m, pad, value=1.0)[:, 0])


AFFINE_SHAPES = [(2, 1, 1, 1), (2, 5, 3, 7), (1, 64, 9, 131)]


def _act64(v, act):
    return {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.2), 3: torch.tanh}[act](v)


@pytest.mark.parametrize("shape", AFFINE_SHAPES)
def test_affine_act_and_leaky_out(ops, shape):
    C = shape[1]
    g = torch.Generator().manual_seed(sum(shape))
    y = torch.randn(shape, generator=g)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    v64 = y.double() * sc.double().view(1, C, 1, 1) + sh.double().view(1, C, 1, 1)
    codes = (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY, ops.ACT_TANH)
    assert codes == (0, 1, 2, 3)
    for act in codes:
        yd = dv(y)
        out = ops.affine_act_(yd, dv(sc), dv(sh), act, 0.2)
        assert out is yd                                            # in place
        assert each_ok(yd, _act64(v64, act)), act
    yd = dv(y)
    out = ops.affine_leaky_out(yd, dv(sc), dv(sh), 0.2)
    assert torch.equal(yd.cpu(), y)                                 # the input is kept
    assert each_ok(out, _act64(v64, 2))


@pytest.mark.parametrize("C", [1, 5, 512])
def test_bn_eval_affine(ops, C):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale.  beta takes
    the sign opposite to mean * gamma, so that no channel's shift is a
    difference of nearly equal terms (whose relative error no fp32 evaluation
    bounds); the signs of gamma and mean themselves are random."""
    g = torch.Generator().manual_seed(C)
    eps = 1e-5
    gamma, mean = torch.randn(C, generator=g), torch.randn(C, generator=g)
    var = torch.rand(C, generator=g) + 0.1
    var[0] = 0.0
    beta = -torch.sign(mean * gamma) * (torch.rand(C, generator=g) + 0.1)
    for gm, bt in ((gamma, beta), (None, None)):
        scale, shift = ops.bn_eval_affine(None if gm is None else dv(gm), None if bt is None else dv(bt),
                                          dv(mean), dv(var), eps)
        g64 = gamma.double() if gm is not None else torch.ones(C, dtype=torch.float64)
        b64 = beta.double() if bt is not None else torch.zeros(C, dtype=torch.float64)
        s64 = g64 / torch.sqrt(var.double() + eps)
        assert each_ok(scale, s64) and each_ok(shift, b64 - mean.double() * s64)


@pytest.mark.parametrize("shape", [(2, 3, 8, 10), (1, 5, 7, 9), (1, 1, 2, 2)])
def test_maxpool2_plain(ops, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    got = ops.maxpool2(dv(x)).cpu()
    assert got.shape == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)     # odd sizes floor
    assert torch.equal(got, F.max_pool2d(x, 2, 2))


@pytest.mark.parametrize("Cout,Cin,K", [(3, 5, 3), (64, 3, 3), (1, 1, 1)])
def test_conv_weight_flip_t(ops, Cout, Cin, K):
    g = torch.Generator().manual_seed(Cout + Cin)
    w = torch.randn(Cout, Cin, K, K, generator=g)
    got = ops.conv_weight_flip_t(dv(w)).cpu()
    assert got.shape == (Cin, Cout, K, K)
    assert torch.equal(got, w.flip(2, 3).transpose(0, 1))


@pytest.mark.parametrize("nb,rows,cols", [(1, 1, 1), (3, 5, 37), (1, 130, 1003), (2, 64, 4099)])
def test_rowsum_batched(ops, nb, rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.rand(nb, rows, cols, generator=g) - 0.25
    xd = dv(x)
    got = ops.rowsum_batched(xd)
    assert got.shape == (rows,)
    assert each_ok(got, x.double().sum((0, 2)))
    assert torch.equal(ops.rowsum_batched(xd), got)                 # fixed order: the same bits
