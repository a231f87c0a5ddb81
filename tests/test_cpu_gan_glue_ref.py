"""CPU-only checks of tests/gan_glue_ref.py, the float64 spectral-norm
reference the GPU tests of csrc/gan.hip's sn_* kernels compare against
(tests/test_gpu_gan_glue.py): it must reproduce
torch.nn.utils.spectral_norm on a float64 Conv2d."""
import pytest
import torch

import gan_glue_ref as R


def _sn_conv(cout, cin, k, seed):
    torch.manual_seed(seed)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, cout, k).double())
    assert conv.weight_u.dtype == torch.float64
    return conv


@pytest.mark.parametrize("cout,cin,k", [(8, 3, 4), (1, 16, 4), (5, 1, 1)])
def test_power_iteration_matches_torch(cout, cin, k):
    conv = _sn_conv(cout, cin, k, seed=cout + cin)
    W = conv.weight_orig.detach().flatten(1).clone()
    u0, v0 = conv.weight_u.clone(), conv.weight_v.clone()
    x = torch.randn(2, cin, 9, 9, dtype=torch.float64)
    conv.train()
    conv(x)                                  # one power iteration, in place on u / v
    u, v, sigma = R.sn_power(W, u0, v0, update=True)
    assert not (torch.equal(conv.weight_u, u0) and torch.equal(conv.weight_v, v0))
    assert R.max_rel(u, conv.weight_u) <= 1e-12
    assert R.max_rel(v, conv.weight_v) <= 1e-12
    assert R.max_rel((W / sigma).view_as(conv.weight), conv.weight.detach()) <= 1e-12
    # a second train-mode forward iterates from the updated vectors
    conv(x)
    u2, v2, sigma2 = R.sn_power(W, u, v, update=True)
    assert R.max_rel(u2, conv.weight_u) <= 1e-12 and R.max_rel(v2, conv.weight_v) <= 1e-12
    assert R.max_rel((W / sigma2).view_as(conv.weight), conv.weight.detach()) <= 1e-12
    # eval: no update, sigma from the stored vectors
    conv.eval()
    ue, ve = conv.weight_u.clone(), conv.weight_v.clone()
    conv(x)
    assert torch.equal(conv.weight_u, ue) and torch.equal(conv.weight_v, ve)
    u3, v3, sigma3 = R.sn_power(W, ue, ve, update=False)
    assert torch.equal(u3, ue) and torch.equal(v3, ve)
    assert R.max_rel((W / sigma3).view_as(conv.weight), conv.weight.detach()) <= 1e-12


def test_weight_grad_matches_torch():
    conv = _sn_conv(6, 3, 4, seed=5)
    x = torch.randn(2, 3, 9, 9, dtype=torch.float64)
    conv.train()
    conv(x)                                  # conv.weight = W / sigma with the updated u, v
    G = torch.randn(conv.weight.shape, dtype=torch.float64)
    (G * conv.weight).sum().backward()
    got = R.sn_weight_grad(G.flatten(1), conv.weight_orig.detach().flatten(1),
                           conv.weight_u.clone(), conv.weight_v.clone())
    assert R.max_rel(got.view_as(G), conv.weight_orig.grad) <= 1e-12
    # the correction term is there: the gradient is not just G / sigma
    sigma = torch.dot(conv.weight_u, conv.weight_orig.detach().flatten(1) @ conv.weight_v)
    assert R.max_rel(G / sigma, conv.weight_orig.grad) > 1e-3


def test_normalize_eps_and_floor_rule():
    z = torch.zeros(4, dtype=torch.float64)
    assert torch.equal(R.normalize(z), z)                    # 0 / max(0, eps), not NaN
    x = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert torch.equal(R.normalize(x), x / 5.0)
    ref = torch.tensor([1.0, -2.0], dtype=torch.float64)
    r32 = ref + torch.tensor([1e-7, 0.0], dtype=torch.float64)
    dev, floor, ok = R.within_floor(ref + 1.1e-6, ref, r32)
    assert floor == pytest.approx(1e-7) and dev == pytest.approx(1.1e-6) and ok   # 4e-7 + 8e-7
    assert not R.within_floor(ref + 1.3e-6, ref, r32)[2]
