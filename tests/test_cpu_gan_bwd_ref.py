"""CPU-only checks of tests/gan_bwd_ref.py, the float64 references that
tests/test_gpu_gan_bwd_edges.py holds csrc/gan_bwd.hip's kernels to.

Two things are settled here, without a GPU.  The formulas: each restatement
equals torch autograd of the operation it stands for, to 1e-12
(gan_glue_ref.max_rel).  The inputs: every case the GPU file runs keeps its
activation kinks clear (min |z| >= 1e-4 max |z| in float64, and the float32
fmaf takes the float64 branch everywhere; the fused multiply-add rounds z to
within 2^-24 |z|, so 1e-4 leaves three orders of room), holds its planted
exact ties, whose reference gradient is 0, and the maxpool tie / NaN windows
route under F.max_pool2d on the CPU to the indices the case list states.
"""
import pytest
import torch
import torch.nn.functional as F

import gan_bwd_ref as B
import gan_glue_ref as R

D = torch.float64


def _chan(t):
    return t.reshape(1, -1, 1, 1)


# ------------------------------------------------ BatchNorm2d + LeakyReLU backward
@pytest.mark.parametrize("with_gamma", [True, False])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 5, 17, 241)])
def test_bn_formulas_match_autograd(shape, mode, with_gamma):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(N + C + H)
    y = (torch.randn(shape, generator=g, dtype=D) * 1.3 + 0.2).requires_grad_(True)
    ga = torch.randn(shape, generator=g, dtype=D)
    ratio = torch.rand(N, H, W, generator=g, dtype=D) * 3
    gamma = (torch.rand(C, generator=g, dtype=D) - 0.5).requires_grad_(True) if with_gamma else None
    beta = torch.randn(C, generator=g, dtype=D).requires_grad_(True) if with_gamma else None
    rm, rv = torch.randn(C, generator=g, dtype=D), torch.rand(C, generator=g, dtype=D) + 0.5
    if mode == "train":
        z = F.batch_norm(y, None, None, gamma, beta, True, 0.1, B.EPS)
    else:
        z = F.batch_norm(y, rm, rv, gamma, beta, False, 0.1, B.EPS)
    F.leaky_relu(z, B.SLOPE).backward(ga)
    det = lambda t: None if t is None else t.detach()  # noqa: E731
    scale, shift, save = B.bn_affine(y.detach(), det(gamma), det(beta), mode, rm, rv)
    assert R.max_rel(y.detach() * _chan(scale) + _chan(shift), z.detach()) <= 1e-12
    P, ldo = H * W, H * W + 3
    for rt in (ratio, None):
        gc, dgamma, dbeta = B.bn_act_bwd(ga, y.detach(), scale, shift, save, det(gamma), rt, ldo,
                                         mode == "eval")
        want = y.grad if rt is None else y.grad * rt.unsqueeze(1)
        assert R.max_rel(gc[:, :, :P], want.reshape(N, C, P)) <= 1e-12
        assert not gc[:, :, P:].any()
        if with_gamma:
            assert R.max_rel(dgamma, gamma.grad) <= 1e-12 and R.max_rel(dbeta, beta.grad) <= 1e-12
    if mode == "train":      # the two mean terms are there: eval's form is another gradient
        ev = B.bn_act_bwd(ga, y.detach(), scale, shift, save, det(gamma), None, P, True)[0]
        assert R.max_rel(ev, y.grad.reshape(N, C, P)) > 1e-3


@pytest.mark.parametrize("case", B.BN_CASES, ids=str)
def test_bn_cases_keep_clear_of_the_kink(case):
    shape, mode, with_gamma = case
    c = B.bn_inputs(*case)
    N, C, H, W = shape
    y, sc, sh = c["y"], c["scale"], c["shift"]
    assert all(c[k].dtype == torch.float32 for k in ("ga", "y", "scale", "shift", "save", "ratio"))
    # scale / shift / save are the float32 roundings of this y's own statistics
    want = B.bn_affine(y, c["gamma"], c["beta"], mode, c.get("rm"), c.get("rv"))
    for got, w in zip((sc, sh, c["save"]), want):
        assert torch.equal(got, w.float())
    z64 = y.double() * _chan(sc.double()) + _chan(sh.double())
    margin = B.kink_margin(z64)
    print(f"bn {case}: min|z| / max|z| = {margin:.3e}")
    assert margin >= B.MARGIN
    assert torch.equal(B.fmaf32(y, _chan(sc), _chan(sh)) > 0, z64 > 0)
    assert torch.equal(y * _chan(sc) + _chan(sh) > 0, z64 > 0)       # the float32 torch floor too
    assert 0 < int((z64 > 0).sum()) < z64.numel()                    # both branches are taken
    # dbeta / dgamma are no differences of nearly equal sums: 1e-6 relative is fair
    gp = torch.where(z64 > 0, c["ga"].double(), c["ga"].double() * B.SLOPE)
    xhat = (y.double() - _chan(c["save"][:C].double())) * _chan(c["save"][C:].double())
    for terms in (gp, gp * xhat):
        assert (terms.abs().sum((0, 2, 3)) <= 4 * terms.sum((0, 2, 3)).abs()).all()


def test_bn_case_lists():
    assert [s[2] * s[3] for s in B.BN_PLANES] == [35, 4096, 4097, 8500, 4097]
    assert [B.bn_ldos(p) for p in (35, 4096, 4097, 8500)] == [
        [35, 36], [4096, 4097], [4097, 4098, 4100], [8500, 8501]]
    assert B.BN_PLANES[4][0] * 2 > 256                                # N * chunks
    for s in B.BN_PLANES + B.BN_MODE_PLANES:
        for mode in ("train", "eval"):
            assert (s, mode, True) in B.BN_CASES or (mode == "eval" and s not in B.BN_MODE_PLANES)


# ------------------------------------------------------ activation + crop backward
@pytest.mark.parametrize("grid", B.ACT_GRIDS, ids=str)
@pytest.mark.parametrize("act", B.ACTS)
def test_act_crop_matches_autograd(act, grid):
    N, C, H, W, gH, gW = grid
    g = torch.Generator().manual_seed(act + H + gW)
    z = torch.randn(N, C, H, W, generator=g, dtype=D)
    z[0, 0, 0, 0] = 0.0                               # on the kink: torch takes the <= 0 branch
    z.requires_grad_(True)
    a = B._apply_act(z, act)[:, :, :gH, :gW]
    go = torch.randn(a.shape, generator=g, dtype=D)
    ratio = torch.rand(N, H, W, generator=g, dtype=D) * 3
    a.backward(go)
    ldo = H * W + 3
    gz, gc = B.gen_act_bwd(go, None if act == 0 else a.detach(), act, ratio, H, W, ldo)
    assert R.max_rel(gz, z.grad.reshape(N, C, H * W)) <= 1e-12
    assert R.max_rel(gc[:, :, :H * W], (z.grad * ratio.unsqueeze(1)).reshape(N, C, H * W)) <= 1e-12
    assert not gc[:, :, H * W:].any()
    outside = torch.ones(H, W, dtype=torch.bool)
    outside[:gH, :gW] = False
    assert not gz.reshape(N, C, H, W)[:, :, outside].any()
    if act in (1, 2):
        assert float(gz[0, 0, 0]) == float(go[0, 0, 0, 0]) * (0.0 if act == 1 else B.SLOPE)
    _, plain = B.gen_act_bwd(go, None if act == 0 else a.detach(), act, None, H, W, H * W)
    assert torch.equal(plain, gz)


@pytest.mark.parametrize("grid", B.ACT_GRIDS, ids=str)
@pytest.mark.parametrize("act", B.ACTS)
def test_act_cases(act, grid):
    N, C, H, W, gH, gW = grid
    c = B.act_inputs(act, grid)
    for ldo in (H * W, H * W + 3):
        rows = N * C * ldo
        assert rows >= 256 and (rows % 256 != 0 or (H, W) == (16, 16))
    if act == 0:
        assert c["a"] is None
        return
    a = c["a"]
    assert a.dtype == torch.float32 and a.shape == c["g"].shape
    if act in (1, 2):
        # the branch reads the float32 input a itself, so both precisions see
        # the same comparison; a == 0 is planted, every other a keeps the margin
        assert c["planted"].any() and not a[c["planted"]].any()
        nz = a[a != 0]
        if nz.numel():
            assert float(nz.abs().min()) >= B.MARGIN * float(a.abs().max())
        d = B.act_deriv(a.double(), act)
        assert torch.equal(d[c["planted"]],
                           torch.full((int(c["planted"].sum()),), 0.0 if act == 1 else B.SLOPE, dtype=D))
        assert torch.equal(a > 0, a.double() > 0)


# --------------------------------------------------------- PartialConv sources
@pytest.mark.parametrize("factor", B.PCONV_FACTORS, ids=str)
@pytest.mark.parametrize("shape", B.PCONV_SHAPES, ids=str)
def test_pconv_sources_match_autograd(shape, factor):
    N, C0, C1, Hs, Ws = shape
    fy, fx = factor
    c = B.pconv_inputs(shape, factor)
    Hin, Win = c["Hin"], c["Win"]
    assert (Hin, Win) == (Hs * fy, Ws * fx)
    x0 = c["x0"].double().requires_grad_(True)
    x1 = c["x1"].double().requires_grad_(True)
    m0, m1, dxin = c["m0"].double(), c["m1"].double(), c["dxin"].double()
    up = F.interpolate(x0 * m0.unsqueeze(1), size=(Hin, Win), mode="nearest")
    xin = torch.cat([up, x1 * m1.unsqueeze(1)], 1)
    got = B.pconv_src_materialize(x0.detach(), m0, x1.detach(), m1, fy, fx)
    assert torch.equal(got, xin.detach())
    xin.backward(dxin)
    assert R.max_rel(B.pconv_src_grad(dxin, 0, C0, m0, fy, fx), x0.grad) <= 1e-12
    assert R.max_rel(B.pconv_src_grad(dxin, C0, C1, m1, 1, 1), x1.grad) <= 1e-12
    prev = c["prev0"].double()
    assert R.max_rel(B.pconv_src_grad(dxin, 0, C0, m0, fy, fx, prev), x0.grad + prev) <= 1e-12
    # no masks, no second source
    x0n = c["x0"].double().requires_grad_(True)
    upn = F.interpolate(x0n, size=(Hin, Win), mode="nearest")
    assert torch.equal(B.pconv_src_materialize(x0n.detach(), None, None, None, fy, fx), upn.detach())
    upn.backward(dxin[:, :C0])
    assert R.max_rel(B.pconv_src_grad(dxin, 0, C0, None, fy, fx), x0n.grad) <= 1e-12
    # a slice from the middle
    c_off, C = B.PCONV_MID[shape]
    assert 0 < c_off and c_off + C < C0 + C1
    assert torch.equal(B.pconv_src_grad(dxin, c_off, C, None, fy, fx),
                       B.block_sum(dxin, fy, fx)[:, c_off:c_off + C])
    assert (c["m0"] == 0).any() and (c["m0"] == 1).any() and c["prev0"].abs().min() > 0


# ----------------------------------------------------------------- sign gradients
@pytest.mark.parametrize("n", B.ABSDIFF_NS)
def test_absdiff_grad_matches_l1loss(n):
    forms = [B.absdiff_inputs(n)] + ([B.absdiff_inputs(1, True)] if n == 1 else [])
    for c in forms:
        a = c["a"].double().requires_grad_(True)
        b, gs = c["b"].double(), c["gs"].double()
        (gs[0] * torch.nn.L1Loss()(a, b)).backward()
        ref = B.absdiff_grad(a.detach(), b, gs, 1.0 / n)
        assert R.max_rel(ref, a.grad) <= 1e-12 or not a.grad.any()
        assert torch.equal(ref == 0, c["ties"]) and torch.equal(a.grad == 0, c["ties"])
        # float32 operands: the float32 difference has the exact sign
        assert torch.equal(torch.sign(c["a"] - c["b"]).double(), torch.sign(a.detach() - b))
        assert c["scale"] == float(torch.tensor(c["scale"], dtype=torch.float32))
        prev = c["prev"].double()
        assert torch.equal(B.absdiff_grad(a.detach(), b, None, c["scale"], prev),
                           prev + torch.sign(a.detach() - b) * c["scale"])
    assert n == 1 or forms[0]["ties"].sum() == 3
    assert n > 1 or (forms[1]["ties"].all() and not forms[0]["ties"].any())


@pytest.mark.parametrize("shape", B.GRAM_SHAPES, ids=str)
def test_gram_sign_sym_matches_autograd(shape):
    Bn, C = shape
    c = B.gram_inputs(Bn, C)
    Ga, Gb, zeros = c["Ga"], c["Gb"], c["zeros"]
    # the inputs: not symmetric, exact zeros of Ga - Gb on and off the diagonal
    diag = torch.eye(C, dtype=torch.bool).expand(Bn, C, C)
    assert torch.equal(Ga - Gb == 0, zeros) and (zeros & diag).any()
    d = torch.sign(Ga - Gb)
    if C > 1:
        assert (zeros & ~diag).any() and not torch.equal(d, d.transpose(1, 2))
        assert (zeros & ~zeros.transpose(1, 2) & ~diag).any()      # a zero whose mirror is none
    assert torch.equal(d.double(), torch.sign(Ga.double() - Gb.double()))
    ref = B.gram_sign_sym(Ga.double(), Gb.double(), c["gs"].double(), c["scale"])
    assert torch.equal(ref, ref.transpose(1, 2))
    assert torch.equal(ref[diag], (2 * d.double() * c["scale"] * 3.0)[diag])
    assert not ref[zeros & diag].any()
    # autograd: the gradient of gs * scale * sum |F F^T - T| w.r.t. F is (dG + dG^T) F
    g = torch.Generator().manual_seed(Bn * C)
    Fm = torch.randn(Bn, C, 7, generator=g, dtype=D).requires_grad_(True)
    T = torch.randn(Bn, C, C, generator=g, dtype=D)
    gram = torch.bmm(Fm, Fm.transpose(1, 2))
    (3.0 * c["scale"] * (gram - T).abs().sum()).backward()
    want = torch.bmm(B.gram_sign_sym(gram.detach(), T, c["gs"].double(), c["scale"]), Fm.detach())
    assert R.max_rel(want, Fm.grad) <= 1e-12


@pytest.mark.parametrize("mask", B.RECON_MASKS)
@pytest.mark.parametrize("n", B.RECON_NS)
def test_gan_recon_bwd_matches_autograd(n, mask):
    forms = [B.recon_inputs(n, mask)] + ([B.recon_inputs(1, mask + "+tie")] if n == 1 else [])
    for c in forms:
        g = c["g"].double().requires_grad_(True)
        o, m, gout = c["o"].double(), c["m"].double(), c["gout"].double()
        lv = torch.sum(torch.abs(g * m - o * m)) / (m.sum() + 1e-8)
        lh = torch.sum(torch.abs(g * (1 - m) - o * (1 - m))) / ((1 - m).sum() + 1e-8)
        lw = torch.mean(torch.abs(g - o) * torch.abs(o))
        (gout[0] * lv + gout[1] * lh + gout[2] * lw).backward()
        sums = B.recon_sums(g.detach(), o, m)
        ref = B.gan_recon_bwd(g.detach(), o, m, sums, gout, float(n), norm32=False)
        assert R.max_rel(ref, g.grad) <= 1e-12 or not g.grad.any()
        # the kernel's float32 normalisers are the same numbers to float32 rounding
        k = B.gan_recon_bwd(g.detach(), o, m, sums, gout, float(n))
        assert R.max_rel(k, ref) <= 2e-7 or not ref.any()
        assert not k[c["ties"]].any() and not g.grad[c["ties"]].any()
        assert torch.equal(c["g"] == c["o"], c["ties"])
        assert torch.equal(torch.sign(c["g"] - c["o"]).double(), torch.sign(g.detach() - o))
        # data parallel: only the Lw term knows the global count
        k3 = B.gan_recon_bwd(g.detach(), o, m, sums, gout, 3.0 * n)
        lw_term = gout[2] * torch.sign(g.detach() - o) * o.abs() / n
        assert R.max_rel(k - k3, lw_term * (2.0 / 3.0)) <= 1e-9 or not lw_term.any()
    assert n == 1 or forms[0]["ties"].sum() == 3
    assert n > 1 or (forms[1]["ties"].all() and not forms[0]["ties"].any())


# --------------------------------------------------------- MaxPool2d(2, 2) backward
@pytest.mark.parametrize("k", range(len(B.MAXPOOL_WINDOWS)))
def test_maxpool_windows_route_as_stated(k):
    w, idx = B.MAXPOOL_WINDOWS[k]
    x = B.window_tensor(w).reshape(1, 1, 2, 2)
    _, ind = F.max_pool2d(x, 2, 2, return_indices=True)
    assert int(ind) == idx
    g = torch.tensor([[[[7.0]]]])
    want = torch.zeros(4)
    want[idx] = 7.0
    assert torch.equal(B.maxpool2_autograd(g, x).reshape(4), want)
    assert torch.equal(B.maxpool2_bwd(g, x).reshape(4), want)


def test_maxpool_window_list():
    ws = dict(B.MAXPOOL_WINDOWS)
    nan = float("nan")
    key = lambda *v: next(w for w in ws if repr(w) == repr(tuple(float(t) for t in v)))  # noqa: E731
    assert ws[key(1, nan, 3, nan)] == 3 and ws[key(0, 1, nan, nan)] == 3
    assert ws[key(nan, nan, 0, 1)] == 1
    ties = [w for w in ws if w.count(5.0) == 2]
    assert sorted((w.index(5.0), 3 - w[::-1].index(5.0)) for w in ties) == [
        (0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert all(ws[w] == w.index(5.0) for w in ties)
    assert sum(1 for w in ws if sum(t != t for t in w) == 1) == 4
    assert sum(1 for w in ws if w.count(-float("inf")) == 3) == 4


@pytest.mark.parametrize("shape", B.MAXPOOL_SHAPES, ids=str)
def test_maxpool_rule_matches_torch(shape):
    c = B.maxpool_inputs(shape)
    x, g = c["x"], c["g"]
    N, C, H, W = shape
    want = B.maxpool2_autograd(g, x)
    assert torch.equal(B.maxpool2_bwd(g, x), want)
    assert torch.equal(B.maxpool2_bwd(g.double(), x.double()), want.double())
    assert not want[:, :, 2 * (H // 2):].any() and not want[:, :, :, 2 * (W // 2):].any()
    assert len(c["planted"]) == (len(B.MAXPOOL_WINDOWS) if H > 2 else 0)
    for n, ch, oy, ox, idx in c["planted"]:
        win = want[n, ch, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2].reshape(4)
        expect = torch.zeros(4)
        expect[idx] = g[n, ch, oy, ox]
        assert torch.equal(win, expect), (n, ch, oy, ox)
    if c["planted"]:
        last = c["planted"][-1]
        assert last[:4] == (N - 1, C - 1, H // 2 - 1, W // 2 - 1)        # the final window too
