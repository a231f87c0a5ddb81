"""CPU-only checks of tests/lstm_ref.py, the float64 reference the GPU tests of
csrc/lstm.hip compare against (tests/test_gpu_lstm_edges.py): it must agree
with torch.nn.LSTM(bidirectional=True) in float64 to 1e-12, in the hidden
states and in the gradient, and its layouts must be the kernel's."""
import pytest
import torch

import lstm_ref as R


def _lstm_case(H, T, N=3, I=24):
    g = torch.Generator().manual_seed(100 * H + T)
    lstm = torch.nn.LSTM(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
    x = torch.randn(N, T, I, generator=g, dtype=torch.float64, requires_grad=True)
    out, _ = lstm(x)
    dh = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dh)
    xd = x.detach()
    # zx = x W_ih^T + b_ih + b_hh for both directions, as test_lstm_recurrence forms it
    zf = xd @ lstm.weight_ih_l0.detach().t() + lstm.bias_ih_l0.detach() + lstm.bias_hh_l0.detach()
    zr = (xd @ lstm.weight_ih_l0_reverse.detach().t() + lstm.bias_ih_l0_reverse.detach()
          + lstm.bias_hh_l0_reverse.detach())
    zx = torch.cat([zf, zr], dim=2)
    return lstm, x, out.detach(), dh, zx


@pytest.mark.parametrize("T", [1, 17])
def test_reference_matches_nn_lstm(T):
    H = 32
    lstm, x, out, dh, zx = _lstm_case(H, T)
    wf, wr = lstm.weight_hh_l0.detach(), lstm.weight_hh_l0_reverse.detach()
    h, cell, gates, dg = R.recurrence(zx, wf, wr, dh)
    assert h.shape == out.shape and cell.shape == out.shape
    assert gates.shape == zx.shape and dg.shape == zx.shape
    eh = R.max_rel(h, out)
    # the gradient with respect to the input, through W_ih
    dx = dg[..., :4 * H] @ lstm.weight_ih_l0.detach() + dg[..., 4 * H:] @ lstm.weight_ih_l0_reverse.detach()
    ex = R.max_rel(dx, x.grad)
    # the bias and recurrent-weight gradients pin dgates per direction and hprev
    eb = R.max_rel(dg[..., :4 * H].sum((0, 1)), lstm.bias_ih_l0.grad)
    ebr = R.max_rel(dg[..., 4 * H:].sum((0, 1)), lstm.bias_hh_l0_reverse.grad)
    hp = R.hprev(h, H)
    dwf = dg[..., :4 * H].reshape(-1, 4 * H).t() @ hp[..., :H].reshape(-1, H)
    dwr = dg[..., 4 * H:].reshape(-1, 4 * H).t() @ hp[..., H:].reshape(-1, H)
    print(f"lstm_ref vs nn.LSTM T={T}: h {eh:.2e} dx {ex:.2e} db {eb:.2e}/{ebr:.2e}")
    assert eh <= 1e-12 and ex <= 1e-12 and eb <= 1e-12 and ebr <= 1e-12
    if T > 1:           # at T = 1 every step starts from zero: the gradient is exactly 0
        assert R.max_rel(dwf, lstm.weight_hh_l0.grad) <= 1e-12
        assert R.max_rel(dwr, lstm.weight_hh_l0_reverse.grad) <= 1e-12
    else:
        assert not hp.any() and not lstm.weight_hh_l0.grad.any()


def test_reference_layouts():
    """gates / cell are what h is made of, at dir*4H + q*H + u: h = o * tanh(c),
    and c_t = f c_{t-1} + i g with c_{t-1} taken along each direction's walk."""
    H, T, N = 32, 5, 2
    g = torch.Generator().manual_seed(7)
    zx = torch.randn(N, T, 8 * H, generator=g, dtype=torch.float64)
    wf = torch.randn(4 * H, H, generator=g, dtype=torch.float64) * 0.3
    wr = torch.randn(4 * H, H, generator=g, dtype=torch.float64) * 0.3
    h, cell, gates, dg = R.recurrence(zx, wf, wr)
    assert dg is None
    for d in range(2):
        i, f, gg, o = gates[..., d * 4 * H:(d + 1) * 4 * H].split(H, dim=2)
        c = cell[..., d * H:(d + 1) * H]
        assert torch.allclose(h[..., d * H:(d + 1) * H], o * torch.tanh(c), rtol=0, atol=1e-15)
        cprev = torch.zeros_like(c)
        if d == 0:
            cprev[:, 1:] = c[:, :-1]
        else:
            cprev[:, :-1] = c[:, 1:]
        assert torch.allclose(c, f * cprev + i * gg, rtol=0, atol=1e-15)
        assert 0 < float(i.min()) and float(i.max()) < 1 and float(gg.min()) < 0   # sigmoid / tanh
    # the first step of each direction sees only zx
    assert torch.equal(gates[:, 0, :H], torch.sigmoid(zx[:, 0, :H]))
    assert torch.equal(gates[:, T - 1, 6 * H:7 * H], torch.tanh(zx[:, T - 1, 6 * H:7 * H]))


def test_hprev_hand_case():
    H = 2
    h = torch.arange(1.0, 13.0, dtype=torch.float64).view(1, 3, 4)   # rows [1..4], [5..8], [9..12]
    want = torch.tensor([[[0, 0, 7, 8], [1, 2, 11, 12], [5, 6, 0, 0]]], dtype=torch.float64)
    assert torch.equal(R.hprev(h, H), want)
    assert not R.hprev(h[:, :1], H).any()


def test_float32_evaluation_is_a_rounding_floor():
    """The same reference in float32 stays within fp32 rounding of the float64
    result (what the GPU tests use as the floor of their bounds)."""
    H, T, N = 32, 17, 2
    g = torch.Generator().manual_seed(11)
    zx = torch.randn(N, T, 8 * H, generator=g)
    wf = torch.randn(4 * H, H, generator=g) * 0.3
    wr = torch.randn(4 * H, H, generator=g) * 0.3
    dh = torch.randn(N, T, 2 * H, generator=g)
    r64 = R.recurrence(zx.double(), wf.double(), wr.double(), dh.double())
    r32 = R.recurrence(zx, wf, wr, dh)
    for a, b in zip(r32, r64):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert 0 < R.max_rel(a, b) < 1e-5
