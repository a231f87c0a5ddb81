"""Edge shapes of the BLSTM recurrence (csrc/lstm.hip through ops.lstm_rec_fwd,
ops.lstm_rec_bwd and ops.lstm_hprev) against the float64 step-by-step
reference tests/lstm_ref.py (pinned to torch.nn.LSTM in test_cpu_lstm_ref.py).

The kernels stage LCH = 16 time steps at a time through double-buffered LDS,
so T runs over 1, 15, 16, 17, 32, 33 and 48 for each instantiated H: less
than a chunk, exactly one, one step more, exactly two (the last chunk full and
nothing to prefetch after it), two and one step, three.

Bound.  Every output (h, cell, gates, dgates) is compared element-wise: the
largest |kernel - fp64| may be 4 x the largest |fp32 - fp64| of the same
reference evaluated in float32 on the CPU (the floor, computed in the test)
plus 4e-7 of the reference's largest magnitude.  The additive term and the 4
cover the hardware exp2 / rcp gates (about 1 ulp each) and tanh formed as
2 sigmoid(2x) - 1, which lstm.hip's header puts within about 1.5e-7 absolute
of tanhf and which the backward evaluates once more on the saved cell.  The
same bound holds on the single time steps next to the chunk seams, so that one
bad step is not averaged away.  Each test prints what it measured.
Measured on an MI355X: see DESIGN.md, "BLSTM recurrence".
"""
import functools

import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

HS = (32, 64, 128)
TS = (1, 15, 16, 17, 32, 33, 48)
CASES = [(H, T) for H in HS for T in TS]
SEAMS = (15, 16, 17, 31, 32)          # forward steps next to a chunk boundary
NAMES = ("h", "cell", "gates", "dgates")


@pytest.fixture(scope="module")
def ops():
    from ainp import ops as _ops
    return _ops


def _inputs(H, T, N, zscale=1.0, seed=None):
    """float32 CPU tensors: zx, whh_f, whh_r (x 0.3, as test_lstm_recurrence), dh."""
    g = torch.Generator().manual_seed(1000 * H + 10 * T + N if seed is None else seed)
    wf = torch.randn(4 * H, H, generator=g) * 0.3
    wr = torch.randn(4 * H, H, generator=g) * 0.3
    zx = torch.randn(N, T, 8 * H, generator=g) * zscale
    dh = torch.randn(N, T, 2 * H, generator=g)
    return zx, wf, wr, dh


def _references(zx, wf, wr, dh):
    """(fp64 reference, its fp32 evaluation), each (h, cell, gates, dgates)."""
    r64 = R.recurrence(zx.double(), wf.double(), wr.double(), dh.double())
    r32 = R.recurrence(zx, wf, wr, dh)
    return r64, r32


def _kernel(ops, zx, wf, wr, dh, save=True):
    """The kernels' (h, cell, gates, dgates) on the CPU; the backward reads the
    forward's own saved gates / cell, as the model does."""
    H = wf.shape[1]
    d = [t.cuda().contiguous() for t in (zx, wf, wr, dh)]
    h, gates, cell = ops.lstm_rec_fwd(d[0], d[1], d[2], H, save=save)
    if not save:
        assert gates is None and cell is None
        torch.cuda.synchronize()
        return h.cpu()
    dg = ops.lstm_rec_bwd(d[3], gates, cell, d[1], d[2], H)
    torch.cuda.synchronize()
    return h.cpu(), cell.cpu(), gates.cpu(), dg.cpu()


@functools.lru_cache(maxsize=None)
def _case(H, T, N=3):
    """Inputs, references and kernel outputs of one shape, computed once and
    shared (read-only) by the tests below."""
    from ainp import ops
    inp = _inputs(H, T, N)
    r64, r32 = _references(*inp)
    return inp, r64, r32, _kernel(ops, *inp)


def _measure(got, r64, r32):
    dev = float((got.double() - r64).abs().max())
    floor = float((r32.double() - r64).abs().max())
    scale = float(r64.abs().max())
    return dev, floor, scale


def _check_all(tag, out, r64, r32):
    bad = []
    for name, got, a, b in zip(NAMES, out, r64, r32):
        assert got.shape == a.shape and torch.isfinite(got).all(), name
        dev, floor, scale = _measure(got, a, b)
        print(f"lstm {tag} {name}: dev {dev:.3e} floor {floor:.3e} max|ref| {scale:.3e} "
              f"(dev/max {dev / scale:.2e}, floor/max {floor / scale:.2e})")
        if not dev <= 4.0 * floor + 4e-7 * scale:
            bad.append((name, dev, floor, scale))
    assert not bad, bad


def _dir_slice(x, t, d):
    """Direction d's part of time step t of an [N, T, 2H | 8H] tensor."""
    w = x.shape[2] // 2
    return x[:, t, d * w:(d + 1) * w]


@pytest.mark.parametrize("H,T", CASES)
def test_every_output_elementwise(H, T):
    _, r64, r32, out = _case(H, T)
    _check_all(f"H={H} T={T}", out, r64, r32)


@pytest.mark.parametrize("H,T", [c for c in CASES if c[1] > SEAMS[0]])
def test_chunk_seams(H, T):
    """The bound on the single steps t = 15, 16, 17, 31, 32 of the forward
    direction and T-1-t of the reverse one (the same positions of its walk)."""
    _, r64, r32, out = _case(H, T)
    bad = []
    for t in (t for t in SEAMS if t < T):
        for d in range(2):
            tt = T - 1 - t if d else t
            for name, got, a, b in zip(NAMES, out, r64, r32):
                dev, floor, scale = _measure(_dir_slice(got, tt, d), _dir_slice(a, tt, d),
                                             _dir_slice(b, tt, d))
                print(f"lstm seam H={H} T={T} step {t} dir {d} {name}: dev {dev:.3e} "
                      f"floor {floor:.3e} max|ref| {scale:.3e}")
                if not dev <= 4.0 * floor + 4e-7 * scale:
                    bad.append((t, d, name, dev, floor, scale))
    assert not bad, bad


def _assert_batch_independent(ops, inp, out):
    zx, wf, wr, dh = inp
    for n in range(zx.shape[0]):
        alone = _kernel(ops, zx[n:n + 1], wf, wr, dh[n:n + 1])
        for name, a, b in zip(NAMES, alone, out):
            assert torch.equal(a[0], b[n]), (name, n)


@pytest.mark.parametrize("H,T", CASES)
def test_batch_independence(ops, H, T):
    """Each sequence run alone (N = 1) gives the batch's bits."""
    inp, _, _, out = _case(H, T)
    _assert_batch_independent(ops, inp, out)


def test_batch_independence_66_workgroups(ops):
    """N = 33: 66 workgroups (sequence x direction), T = 17, H = 32."""
    inp = _inputs(32, 17, 33)
    out = _kernel(ops, *inp)
    _assert_batch_independent(ops, inp, out)
    r64, r32 = _references(*inp)
    _check_all("H=32 T=17 N=33", out, r64, r32)


@pytest.mark.parametrize("H,T", CASES)
def test_save_false_and_repeatability(ops, H, T):
    inp, _, _, out = _case(H, T)
    assert torch.equal(_kernel(ops, *inp, save=False), out[0])     # null gates / cell
    again = _kernel(ops, *inp)
    for name, a, b in zip(NAMES, again, out):
        assert torch.equal(a, b), name


def test_saturated_gates(ops):
    """zx x 8 (many pre-activations beyond +-20) with entries at +-90, where
    exp2 overflows to inf inside the kernel's sigmoid: everything stays finite
    and within the same bound (the floor from the fp32 reference at the same
    inputs)."""
    H, T, N = 64, 33, 3
    zx, wf, wr, dh = _inputs(H, T, N, zscale=8.0)
    assert int((zx.abs() > 20).sum()) > 300
    g = torch.Generator().manual_seed(5)
    flat = zx.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:16]
    flat[idx[:8]] = 90.0
    flat[idx[8:]] = -90.0
    # one of each in the g gate (argument doubled in the kernel) at a chunk seam
    zx[0, 16, 2 * H + 3] = 90.0
    zx[1, 16, 4 * H + 2 * H + 5] = -90.0
    out = _kernel(ops, zx, wf, wr, dh)
    r64, r32 = _references(zx, wf, wr, dh)
    for a in r64:
        assert torch.isfinite(a).all()
    _check_all("saturated H=64 T=33", out, r64, r32)


@pytest.mark.parametrize("N,T,H", [(2, 1, 32), (2, 3, 32), (3, 17, 64)])
def test_hprev_exact(ops, N, T, H):
    g = torch.Generator().manual_seed(N * T * H)
    h = torch.randn(N, T, 2 * H, generator=g)
    assert (N * T * 2 * H) % 256 != 0          # a partial last block of the 256-thread grid
    got = ops.lstm_hprev(h.cuda(), H).cpu()
    assert torch.equal(got, R.hprev(h, H))
    if T == 1:
        assert not got.any()


def test_unsupported_h_raises(ops):
    """Only H = 32, 64 and 128 are instantiated; anything else is an error,
    not a silent no-op, from both entry points."""
    H, N, T = 48, 2, 5
    zx, wf, wr, dh = (t.cuda() for t in _inputs(H, T, N))
    with pytest.raises(RuntimeError, match="H must be 32, 64 or 128"):
        ops.lstm_rec_fwd(zx, wf, wr, H)
    gates = torch.zeros(N, T, 8 * H, device="cuda")
    cell = torch.zeros(N, T, 2 * H, device="cuda")
    with pytest.raises(RuntimeError, match="H must be 32, 64 or 128"):
        ops.lstm_rec_bwd(dh, gates, cell, wf, wr, H)
