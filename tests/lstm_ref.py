"""Step-by-step reference of the bidirectional LSTM recurrence that
csrc/lstm.hip computes, for the tests only: plain differentiable torch ops in
whatever dtype the inputs have (float64 for the reference proper, float32 for
the rounding floor the GPU tests measure against it).

Layouts are the kernel's:
  zx    [N, T, 8H]  gate pre-activations x W_ih^T + b of both directions, the
                    forward direction's 4H first, gate order i, f, g, o
  whh_* [4H, H]     recurrent weights (rows in the same gate order)
  h     [N, T, 2H]  hidden state, forward direction's H first
  cell  [N, T, 2H]  cell state c_t
  gates [N, T, 8H]  post-activation gates at dir*4H + q*H + u
The reverse direction walks t = T-1 .. 0.  It shares no structure with the
kernel: no chunks, no staging, torch.sigmoid / torch.tanh.
"""
import torch


def recurrence(zx, whh_f, whh_r, dh=None):
    """-> (h, cell, gates, dgates); dgates = d<h, dh>/d zx (None without dh).
    zx is used as the autograd leaf, so dgates is exactly zx.grad."""
    N, T, G = zx.shape
    H = G // 8
    assert G == 8 * H and whh_f.shape == (4 * H, H) and whh_r.shape == (4 * H, H)
    zx = zx.detach().clone().requires_grad_(dh is not None)
    hs, cs, gs = [], [], []
    for d, whh in enumerate((whh_f, whh_r)):
        h = zx.new_zeros(N, H)
        c = zx.new_zeros(N, H)
        hd, cd, gd = [None] * T, [None] * T, [None] * T
        for s in range(T):
            t = T - 1 - s if d else s
            pre = zx[:, t, d * 4 * H:(d + 1) * 4 * H] + h @ whh.t()
            i, f, g, o = pre.split(H, dim=1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c = f * c + i * g
            h = o * torch.tanh(c)
            hd[t], cd[t], gd[t] = h, c, torch.cat([i, f, g, o], dim=1)
        hs.append(torch.stack(hd, dim=1))
        cs.append(torch.stack(cd, dim=1))
        gs.append(torch.stack(gd, dim=1))
    h = torch.cat(hs, dim=2)
    cell = torch.cat(cs, dim=2)
    gates = torch.cat(gs, dim=2)
    dgates = None
    if dh is not None:
        dgates, = torch.autograd.grad(h, zx, dh.to(h.dtype))
    return h.detach(), cell.detach(), gates.detach(), dgates


def hprev(h, H):
    """The hidden state each step started from, in h's layout: the forward half
    shifted one step later, the reverse half one step earlier, zero at the
    open end."""
    out = torch.zeros_like(h)
    out[:, 1:, :H] = h[:, :-1, :H]
    out[:, :-1, H:] = h[:, 1:, H:]
    return out


def max_rel(got, ref):
    """max |got - ref| / max |ref|: one wrong element is not averaged away."""
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
