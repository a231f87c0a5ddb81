"""Plain restatements of the GAN's spectral-norm arithmetic (csrc/gan.hip's
sn_* kernels), for the tests only, in whatever dtype the inputs have: float64
for the reference proper, float32 for the rounding floor the GPU tests measure
against it.  tests/test_cpu_gan_glue_ref.py pins them to
torch.nn.utils.spectral_norm itself.

W is the weight as a matrix [h, wd] (Conv2d: weight.flatten(1)).
"""
import torch


def normalize(x, eps=1e-12):
    """F.normalize(x, dim=0, eps): x / max(||x||, eps)."""
    return x / torch.clamp(torch.linalg.vector_norm(x), min=eps)


def sn_power(W, u, v, update=True, eps=1e-12):
    """One train-mode forward of torch.nn.utils.spectral_norm
    (n_power_iterations = 1): v = normalize(W^T u), u = normalize(W v),
    sigma = u . W v.  update=False is the eval form: sigma from the stored
    u, v.  -> (u, v, sigma)."""
    if update:
        v = normalize(W.t() @ u, eps)
        u = normalize(W @ v, eps)
    return u, v, torch.dot(u, W @ v)


def sn_weight_grad(G, W, u, v):
    """d <G, W / sigma(W)> / dW with sigma = u . W v and u, v held constant
    (torch detaches them), by autograd of that expression."""
    W = W.detach().clone().requires_grad_(True)
    sigma = torch.dot(u, W @ v)
    (G * (W / sigma)).sum().backward()
    return W.grad


def max_rel(got, ref):
    """max |got - ref| / max |ref|."""
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def within_floor(got, ref64, ref32):
    """The element-wise rule of the kernel tests: the kernel's largest
    deviation from the float64 reference may be 4 x that of the float32
    evaluation of the same reference plus 4e-7 of the reference's largest
    magnitude (a few fp32 roundings of it: another operation order).
    -> (deviation, floor, ok)."""
    ref64 = ref64.double()
    dev = float((got.double() - ref64).abs().max())
    floor = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    return dev, floor, dev <= 4.0 * floor + 4e-7 * scale
