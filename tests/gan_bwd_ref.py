"""Plain torch restatements of the generator-backward kernels' contracts
(csrc/gan_bwd.hip behind ainp.ops), for the tests only, in whatever dtype the
inputs have: float64 for the reference proper, float32 for the rounding floor
the GPU tests measure against it (gan_glue_ref.within_floor).  Every function
takes the very tensors the kernel gets (float32 values, cast up for the
reference), so both sides start from identical numbers.

tests/test_cpu_gan_bwd_ref.py pins each formula to torch autograd and proves
the conditions on the inputs built here (branch margins, planted ties, the
maxpool tie / NaN windows); tests/test_gpu_gan_bwd_edges.py runs the kernels
on the same cases.  The builders are cached: a case is built once and shared,
and nobody writes into what they return.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

SLOPE = 0.2
EPS = 1e-5
MARGIN = 1e-4          # min |z| >= MARGIN * max |z| at every activation kink


def ld4(P):
    """Pixel rows padded to a multiple of 4, as ainp.gan._ld4."""
    return P + (-P) % 4


def fmaf32(y, a, b):
    """fmaf(y, a, b) of float32 operands.  The product of two float32 values
    is exact in float64; the sum is rounded once to float64 and once more to
    float32.  That second rounding can move the last bit, never the sign, and
    the sign is all the kernels' branch reads."""
    return (y.double() * a.double() + b.double()).float()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _chan(t, C):
    return t.reshape(1, C, 1, 1)


# ------------------------------------------------ BatchNorm2d + LeakyReLU backward
def bn_act_bwd(ga, y, scale, shift, save, gamma, ratio, ldo, eval_mode, slope=SLOPE):
    """-> (gc [N, C, ldo], dgamma [C], dbeta [C]).  g' = ga * leaky'(z) with
    the branch on z = y * scale[c] + shift[c]; xhat = (y - save[c]) * save[C + c];
    dbeta = sum g', dgamma = sum g' xhat over (n, pixel);
    dy = gamma rstd (g' - dbeta / M - xhat dgamma / M), the two mean terms
    dropped in eval mode (save = running mean | rstd); gamma None is 1; then
    dy * ratio[n][p] in rows of ldo, the padding 0."""
    N, C, H, W = y.shape
    P, M = H * W, N * H * W
    z = y * _chan(scale, C) + _chan(shift, C)
    gp = torch.where(z > 0, ga, ga * slope)
    xhat = (y - _chan(save[:C], C)) * _chan(save[C:], C)
    dbeta = gp.sum((0, 2, 3))
    dgamma = (gp * xhat).sum((0, 2, 3))
    k = save[C:] if gamma is None else gamma * save[C:]
    if eval_mode:
        dy = _chan(k, C) * gp
    else:
        dy = _chan(k, C) * (gp - _chan(dbeta, C) / M - xhat * _chan(dgamma, C) / M)
    if ratio is not None:
        dy = dy * ratio.unsqueeze(1)
    gc = torch.zeros(N, C, ldo, dtype=y.dtype)
    gc[:, :, :P] = dy.reshape(N, C, P)
    return gc, dgamma, dbeta


# (N, C, H, W): planes around BA_CHUNK = 4096 and the 256-lane loop
BN_PLANES = [
    (2, 3, 5, 7),          # P = 35: fewer elements than lanes
    (1, 2, 64, 64),        # P = 4096: exactly one full chunk
    (2, 5, 17, 241),       # P = 4097: the second chunk holds one element
    (1, 3, 68, 125),       # P = 8500: three chunks, the last 308 (two rounds for some lanes)
    (130, 1, 17, 241),     # N * chunks = 260 > 256: bn_act_bwd_sum_kernel's second round
]
BN_MODE_PLANES = [BN_PLANES[0], BN_PLANES[2], BN_PLANES[3]]     # also count = 0 and eval
BN_OPTION_PLANE = BN_PLANES[0]                                  # gamma None, ratio None
# every (plane, mode, with_gamma) the GPU file builds
BN_CASES = ([(s, "train", True) for s in BN_PLANES] + [(s, "eval", True) for s in BN_MODE_PLANES]
            + [(BN_OPTION_PLANE, "train", False), (BN_OPTION_PLANE, "eval", False)])


def bn_ldos(P):
    return sorted({P, P + 1, ld4(P)})


def bn_affine(y, gamma, beta, mode, rm=None, rv=None):
    """(scale, shift, save) in float64 from y's batch statistics (train) or the
    running ones (eval); gamma None is 1, beta None 0."""
    y = y.double()
    C = y.shape[1]
    if mode == "train":
        mean = y.mean((0, 2, 3))
        var = y.var((0, 2, 3), unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    rstd = 1.0 / torch.sqrt(var + EPS)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    scale = g * rstd
    return scale, b - mean * scale, torch.cat([mean, rstd])


def kink_margin(z):
    """min |z| / max |z|."""
    z = z.double().abs()
    return float(z.min() / z.max())


@functools.lru_cache(maxsize=None)
def bn_inputs(shape, mode, with_gamma):
    """float32 inputs of one BN case: ga, y, gamma, beta, scale, shift, save,
    ratio (+ rm, rv in eval mode).  ga has mean 1 and |gamma| >= 0.5, so that
    dbeta and dgamma are sums of mostly like-signed terms (1e-6 relative is a
    fair bound for them; test_cpu_gan_bwd_ref.py checks the conditioning).
    y is repaired until no z = y * scale + shift lies within MARGIN * max |z|
    of the LeakyReLU kink: an offending y moves away from it by 1e-3 max |z|,
    and the batch statistics (train mode) are taken again."""
    N, C, H, W = shape
    g = _gen("bn", shape, mode, with_gamma)
    std, off = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    y = torch.randn(shape, generator=g) * _chan(std, C) + _chan(off, C)
    ga = torch.randn(shape, generator=g) * 0.5 + 1.0
    sign = torch.where(torch.rand(C, generator=g) > 0.5, 1.0, -1.0)
    gamma = sign * (torch.rand(C, generator=g) + 0.5) if with_gamma else None
    beta = torch.randn(C, generator=g) * 0.1 if with_gamma else None
    # running statistics near the batch's own, as training leaves them
    rm = off + torch.randn(C, generator=g) * 0.1
    rv = std * std * (torch.rand(C, generator=g) * 0.4 + 0.8)
    ratio = torch.rand(N, H, W, generator=g) * 3
    for _ in range(20):
        scale, shift, save = (t.float() for t in bn_affine(y, gamma, beta, mode, rm, rv))
        z = y.double() * _chan(scale.double(), C) + _chan(shift.double(), C)
        zmax = float(z.abs().max())
        bad = z.abs() < 2 * MARGIN * zmax           # twice the margin: the statistics move on
        if not bad.any():
            break
        away = torch.sign(z) * torch.sign(_chan(scale.double(), C)) * 1e-3 * zmax
        y = torch.where(bad, y.double() + away / _chan(scale.double().abs(), C), y.double()).float()
    else:
        raise AssertionError("bn_inputs: the kink repair did not settle")
    out = dict(ga=ga, y=y, gamma=gamma, beta=beta, scale=scale, shift=shift, save=save,
               ratio=ratio)
    if mode == "eval":
        out.update(rm=rm, rv=rv)
    return out


@functools.lru_cache(maxsize=None)
def bn_refs(shape, mode, with_gamma, with_ratio, ldo):
    """((gc, dgamma, dbeta) in float64, the same in float32) for one case."""
    c = bn_inputs(shape, mode, with_gamma)
    out = []
    for dt in (torch.float64, torch.float32):
        cast = lambda t: None if t is None else t.to(dt)  # noqa: E731
        out.append(bn_act_bwd(cast(c["ga"]), cast(c["y"]), cast(c["scale"]), cast(c["shift"]),
                              cast(c["save"]), cast(c["gamma"]),
                              cast(c["ratio"]) if with_ratio else None, ldo, mode == "eval"))
    return tuple(out)


# ------------------------------------------------------ activation + crop backward
def act_deriv(a, act, slope=SLOPE):
    """act'(.) from the activation's output a (ainp's ACT_* codes 0 none,
    1 ReLU, 2 LeakyReLU, 3 Tanh); a == 0 takes the <= 0 branch."""
    if act == 0:
        return None
    if act == 1:
        return torch.where(a > 0, torch.ones_like(a), torch.zeros_like(a))
    if act == 2:
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    return 1 - a * a


def gen_act_bwd(g, a, act, ratio, H, W, ldo, slope=SLOPE):
    """g, a [N, C, gH, gW] (the crop's top-left corner is the grid's) ->
    (gz [N, C, H*W] = g * act'(a), 0 outside the crop;
     gc [N, C, ldo] = gz * ratio[n][p], 0 in the padding)."""
    N, C, gH, gW = g.shape
    if act == 2:
        v = torch.where(a > 0, g, g * slope)         # the kernel's one product
    else:
        d = act_deriv(a, act, slope)
        v = g if d is None else g * d
    gz = torch.zeros(N, C, H, W, dtype=g.dtype)
    gz[:, :, :gH, :gW] = v
    gr = gz if ratio is None else gz * ratio.unsqueeze(1)
    gc = torch.zeros(N, C, ldo, dtype=g.dtype)
    gc[:, :, :H * W] = gr.reshape(N, C, H * W)
    return gz.reshape(N, C, H * W), gc


# (N, C, H, W, gH, gW).  N * C * ldo is above 256 and no multiple of it for
# ldo = P and P + 3, but for the two 16 x 16 grids: one workgroup exactly
# (C = 1, where every row is its own image) and two exactly (C = 2).  With
# C = 1 the ratio index row / C is row itself, so that grid says nothing
# about the division; every other grid has C > 1 and does.
ACT_GRIDS = [
    (2, 3, 9, 31, 9, 31),
    (2, 3, 9, 31, 7, 28),
    (2, 3, 9, 31, 1, 1),
    (1, 1, 16, 16, 16, 16),
    (1, 2, 16, 16, 16, 16),
]
ACTS = [0, 1, 2, 3]


def _apply_act(z, act):
    return {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, SLOPE), 3: torch.tanh}[act](z)


@functools.lru_cache(maxsize=None)
def act_inputs(act, grid):
    """g, a (None for act 0), ratio in float32, and `planted`, the mask of the
    a == 0 planted for ReLU / LeakyReLU.  a is the activation's own float32
    output over the conv grid, cropped; every non-zero a of act 1, 2 is at
    least MARGIN * max |a| (smaller ones are set to +-0.5)."""
    N, C, H, W, gH, gW = grid
    gen = _gen("act", act, grid)
    g = torch.randn(N, C, gH, gW, generator=gen)
    z = torch.randn(N, C, H, W, generator=gen)
    ratio = torch.rand(N, H, W, generator=gen) * 3
    a = _apply_act(z, act)[:, :, :gH, :gW].contiguous()
    planted = torch.zeros_like(a, dtype=torch.bool)
    if act in (1, 2):
        small = (a != 0) & (a.abs() < MARGIN * a.abs().max())
        a = torch.where(small, torch.where(a > 0, 0.5, -0.5), a)
        flat = planted.view(-1)
        flat[0] = flat[-1] = flat[flat.numel() // 2] = True
        a = torch.where(planted, torch.zeros_like(a), a)
    return dict(g=g, a=None if act == 0 else a, ratio=ratio, planted=planted)


@functools.lru_cache(maxsize=None)
def act_refs(act, grid, with_ratio, ldo):
    c = act_inputs(act, grid)
    H, W = grid[2], grid[3]
    out = []
    for dt in (torch.float64, torch.float32):
        cast = lambda t: None if t is None else t.to(dt)  # noqa: E731
        out.append(gen_act_bwd(cast(c["g"]), cast(c["a"]), act,
                               cast(c["ratio"]) if with_ratio else None, H, W, ldo))
    return tuple(out)


# --------------------------------------------------------- PartialConv sources
def nearest_up(x, fy, fx):
    """Nearest upsample by integer factors: output (y, x) reads (y // fy, x // fx)."""
    return x.repeat_interleave(fy, -2).repeat_interleave(fx, -1)


def pconv_src_materialize(x0, m0, x1, m1, fy, fx):
    """cat(nearest(x0 * m0), x1 * m1) over channels; a mask None is 1, x1 None
    no second source.  x0 [N, C0, Hs, Ws], m0 [N, Hs, Ws]; x1 [N, C1, Hin, Win]."""
    s0 = x0 if m0 is None else x0 * m0.unsqueeze(1)
    out = nearest_up(s0, fy, fx)
    if x1 is not None:
        out = torch.cat([out, x1 if m1 is None else x1 * m1.unsqueeze(1)], 1)
    return out


def block_sum(x, fy, fx):
    """[.., Hs * fy, Ws * fx] -> [.., Hs, Ws]: the sum over each fy x fx block
    (the nearest upsample's backward)."""
    *lead, Hin, Win = x.shape
    return x.reshape(*lead, Hin // fy, fy, Win // fx, fx).sum((-3, -1))


def pconv_src_grad(dxin, c_off, C, ms, fy, fx, prev=None):
    """prev + ms * block_sum(dxin[:, c_off : c_off + C]) (prev None: 0)."""
    s = block_sum(dxin[:, c_off:c_off + C], fy, fx)
    if ms is not None:
        s = s * ms.unsqueeze(1)
    return s if prev is None else s + prev


PCONV_FACTORS = [(1, 1), (2, 2), (2, 1), (3, 2)]
# (N, C0, C1, Hs, Ws); mid = (c_off, C) of a slice from the middle of Cin
PCONV_SHAPES = [(2, 3, 2, 5, 7), (1, 65, 1, 9, 13)]
PCONV_MID = {(2, 3, 2, 5, 7): (1, 2), (1, 65, 1, 9, 13): (7, 50)}


@functools.lru_cache(maxsize=None)
def pconv_inputs(shape, factor):
    N, C0, C1, Hs, Ws = shape
    fy, fx = factor
    Hin, Win = Hs * fy, Ws * fx
    g = _gen("pconv", shape, factor)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    mask = lambda *s: (torch.rand(*s, generator=g) > 0.3).float()  # noqa: E731
    c_off, C = PCONV_MID[shape]
    return dict(x0=r(N, C0, Hs, Ws), m0=mask(N, Hs, Ws), x1=r(N, C1, Hin, Win),
                m1=mask(N, Hin, Win), dxin=r(N, C0 + C1, Hin, Win), prev0=r(N, C0, Hs, Ws),
                prev_mid=r(N, C, Hs, Ws), Hin=Hin, Win=Win)


# --------------------------------------------------------- MaxPool2d(2, 2) backward
def maxpool2_bwd(g, x):
    """The rule torch's CPU max_pool2d follows, restated: scan the window in
    row-major order and move on to a candidate that is larger or NaN.  So the
    first maximum takes the gradient, and where the window holds NaNs, the
    last NaN.  An odd last row / column belongs to no window: 0."""
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    w = x[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5)
    w = w.reshape(N, C, Ho, Wo, 4)
    mx = w[..., 0].clone()
    best = torch.zeros(N, C, Ho, Wo, dtype=torch.int64)
    for k in range(1, 4):
        c = w[..., k]
        take = (c > mx) | torch.isnan(c)
        mx = torch.where(take, c, mx)
        best = torch.where(take, torch.full_like(best, k), best)
    hit = F.one_hot(best, 4).to(g.dtype) * g.unsqueeze(-1)
    hit = hit.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    gx = torch.zeros(N, C, H, W, dtype=g.dtype)
    gx[:, :, :2 * Ho, :2 * Wo] = hit
    return gx


def maxpool2_autograd(g, x):
    """The gradient torch's own CPU kernels route."""
    leaf = x.clone().requires_grad_(True)
    F.max_pool2d(leaf, 2, 2).backward(g)
    return leaf.grad


_NAN, _INF = float("nan"), float("inf")
# (window in row-major order [[w0, w1], [w2, w3]], the index torch's CPU pooling routes to)
MAXPOOL_WINDOWS = [
    # a tie of the maximum at every pair of positions: the first one
    (tuple(5.0 if k in pair else -1.0 - k for k in range(4)), pair[0])
    for pair in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
] + [
    ((2.5, 2.5, 2.5, 2.5), 0),                       # all equal
    ((0.5, -_INF, -_INF, -_INF), 0),                 # -inf in three positions
    ((-_INF, 0.5, -_INF, -_INF), 1),
    ((-_INF, -_INF, 0.5, -_INF), 2),
    ((-_INF, -_INF, -_INF, 0.5), 3),
    ((-_INF, -_INF, -_INF, -_INF), 0),               # and in all four: nothing beats the first
    ((_NAN, 1.0, 2.0, 3.0), 0),                      # one NaN at each position
    ((1.0, _NAN, 2.0, 3.0), 1),
    ((1.0, 2.0, _NAN, 3.0), 2),
    ((3.0, 2.0, 1.0, _NAN), 3),
    ((1.0, _NAN, 3.0, _NAN), 3),                     # two NaNs: the last one
    ((0.0, 1.0, _NAN, _NAN), 3),
    ((_NAN, _NAN, 0.0, 1.0), 1),
]
MAXPOOL_SHAPES = [(1, 1, 2, 2), (2, 3, 8, 10), (1, 5, 7, 9), (1, 2, 33, 35)]


def window_tensor(w):
    return torch.tensor(w, dtype=torch.float32).reshape(2, 2)


@functools.lru_cache(maxsize=None)
def maxpool_inputs(shape):
    """x with every MAXPOOL_WINDOWS entry planted (half of them in the first
    windows of the tensor, half in the last, the final window included), g,
    and `planted` [(n, c, oy, ox, index)].  (1, 1, 2, 2) holds one window:
    the GPU test runs that shape once per planted window instead."""
    N, C, H, W = shape
    Ho, Wo = H // 2, W // 2
    gen = _gen("maxpool", shape)
    x = torch.randn(shape, generator=gen)
    g = torch.randn(N, C, Ho, Wo, generator=gen)
    planted = []
    total = N * C * Ho * Wo
    if total >= len(MAXPOOL_WINDOWS):
        half = len(MAXPOOL_WINDOWS) // 2
        for i, (w, idx) in enumerate(MAXPOOL_WINDOWS):
            f = i if i < half else total - len(MAXPOOL_WINDOWS) + i
            ox, oy, c, n = f % Wo, (f // Wo) % Ho, (f // (Wo * Ho)) % C, f // (Wo * Ho * C)
            x[n, c, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2] = window_tensor(w)
            planted.append((n, c, oy, ox, idx))
    return dict(x=x, g=g, planted=planted)


# ----------------------------------------------------------------- sign gradients
def absdiff_grad(a, b, gs, scale, prev=None):
    """prev + sign(a - b) * scale * gs (nn.L1Loss backward; sign(0) = 0)."""
    v = torch.sign(a - b) * scale
    if gs is not None:
        v = v * gs
    return v if prev is None else v + prev


ABSDIFF_NS = [1, 255, 256, 257, 100003]


def f32(v):
    """A Python float that float32 holds exactly (what the kernel receives)."""
    return float(torch.tensor(v, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def absdiff_inputs(n, tie_only=False):
    """a, b, prev, gs (a 1-element tensor), scale, ties (mask of the planted
    a == b).  n = 1 comes in two forms: its element a tie, or not."""
    g = _gen("absdiff", n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ties = torch.zeros(n, dtype=torch.bool)
    if n > 1:
        ties[[0, n // 2, n - 1]] = True
    elif tie_only:
        ties[0] = True
    b = torch.where(ties, a, b)
    assert not ((a == b) & ~ties).any()
    return dict(a=a, b=b, prev=torch.randn(n, generator=g), gs=torch.tensor([1.7]),
                scale=f32(1.0 / n), ties=ties)


def gram_sign_sym(Ga, Gb, gs, scale):
    """(sign(Ga - Gb) + sign(Ga - Gb)^T) * scale * gs per batch."""
    s = torch.sign(Ga - Gb)
    v = (s + s.transpose(1, 2)) * scale
    return v if gs is None else v * gs


GRAM_SHAPES = [(1, 1), (2, 3), (1, 17), (2, 64)]


@functools.lru_cache(maxsize=None)
def gram_inputs(B, C):
    """Non-symmetric Ga, Gb with Ga == Gb planted on the diagonal and, for
    C > 1, at off-diagonal places whose mirror image differs (`zeros` mask)."""
    g = _gen("gram", B, C)
    Ga, Gb = torch.randn(B, C, C, generator=g), torch.randn(B, C, C, generator=g)
    zeros = torch.zeros(B, C, C, dtype=torch.bool)
    zeros[B - 1, C - 1, C - 1] = True
    if C > 1:
        zeros[0, 0, 0] = True
        zeros[0, 0, C - 1] = True                     # [C - 1, 0] stays non-zero
        zeros[B - 1, C - 1, C // 2 - 1 if C > 2 else 0] = True
    Gb = torch.where(zeros, Ga, Gb)
    assert not ((Ga == Gb) & ~zeros).any()
    return dict(Ga=Ga, Gb=Gb, zeros=zeros, gs=torch.tensor([3.0]), scale=f32(1.0 / (B * C * C)))


def recon_sums(g, o, m):
    """calculate_losses' five sums: sum |gm - om|, sum m, sum |gh - oh|,
    sum h, sum |g - o| |o|, with h = 1 - m."""
    h = 1 - m
    return torch.stack([(g * m - o * m).abs().sum(), m.sum(), (g * h - o * h).abs().sum(), h.sum(),
                        ((g - o).abs() * o.abs()).sum()])


def gan_recon_bwd(g, o, m, sums, gout, n_total, norm32=True):
    """d (gout . (Lv, Lh, Lw)) / d g =
         gout0 sign(gm - om) m / (sum m + 1e-8) + gout1 sign(gh - oh) h / (sum h + 1e-8)
         + gout2 sign(g - o) |o| / n_total.
    norm32: the normalisers as the kernel forms them, (float)sum + 1e-8f in
    float32 (an input both sides share: with an all-0 or all-1 mask the 1e-8
    is the whole normaliser); False: in g's dtype, as autograd of the float64
    loss has them."""
    h = 1 - m
    if norm32:
        nv = (sums[1].float() + torch.tensor(1e-8, dtype=torch.float32)).to(g.dtype)
        nh = (sums[3].float() + torch.tensor(1e-8, dtype=torch.float32)).to(g.dtype)
    else:
        nv, nh = sums[1].to(g.dtype) + 1e-8, sums[3].to(g.dtype) + 1e-8
    r = gout[0] * (torch.sign(g * m - o * m) * m / nv)
    r = r + gout[1] * (torch.sign(g * h - o * h) * h / nh)
    return r + gout[2] * (torch.sign(g - o) * o.abs() / n_total)


RECON_NS = [1, 257, 70001]
RECON_MASKS = ["random", "ones", "zeros"]


@functools.lru_cache(maxsize=None)
def recon_inputs(n, mask):
    """g, o, m, gout, ties (mask of the planted g == o; n = 1 has none, its
    tie form is recon_inputs(1, mask + "+tie"))."""
    tie1 = mask.endswith("+tie")
    mask = mask.replace("+tie", "")
    gen = _gen("recon", n, mask)
    g = torch.tanh(torch.randn(n, generator=gen))
    o = torch.rand(n, generator=gen) * 3
    m = {"random": (torch.rand(n, generator=gen) > 0.4).float(), "ones": torch.ones(n),
         "zeros": torch.zeros(n)}[mask]
    ties = torch.zeros(n, dtype=torch.bool)
    if n > 1:
        ties[[0, n // 3, n - 1]] = True
    elif tie1:
        ties[0] = True
    o = torch.where(ties, g, o)
    assert not ((g == o) & ~ties).any()
    return dict(g=g, o=o, m=m, gout=torch.tensor([1.0, 2.0, 0.2]), ties=ties)
