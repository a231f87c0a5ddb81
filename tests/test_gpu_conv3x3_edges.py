"""Element-wise tests of every 3x3 conv route (csrc/conv.hip, csrc/conv_x6.hip
behind csrc/conv_route.h) against the float64 reference of
tests/conv3x3_ref.py, at the planes where the tilings change, for the model's
channel pairs, the generic exact kernel's stagings and the mixed-kernel /
multi-pass weight gradients, in fp32, the bf16 arithmetic and bf16 storage,
in every layout the entry points take.  test_cpu_conv3x3_ref.py pins the
reference to autograd, proves the conditions of the integer data and checks
on the host which kernel every launch here reaches.

Integer cases (conv3x3_edge_worker.run_int): y, dx, dw, db torch.equal to the
float64 result, launched into NaN-filled buffers; the BatchNorm partial rows
of exactly ainp_conv3x3_fwd_stat_rows_ex rows start from NaN, none is left,
their sums are within 1e-6 sum |y| (sum y^2) of the reference per channel and
a second call gives the same bits; conv3x3_dgrad_bnr's dx is the plain data
gradient.  A call the host queries (cl_ok, io16_ok, dy16_ok, dgrad_cfnt_ok) do
not promise may refuse, with a message of conv_refusal_text; a served one is
checked all the same.

Real cases: gan_glue_ref.within_floor on every tensor (the largest deviation
from float64 at most 4 x that of the float32 torch evaluation of the same
reference plus 4e-7 of the reference's largest magnitude); for the bf16
arithmetic both references take the bf16-rounded operands.  db and the summed
statistics: 1e-6 relative per channel.  Each check prints what it measured;
DESIGN.md ("Edge-shape tests") keeps the largest.

The routes that conv_env() selects once per process run the integer cases in a
fresh child each (conv3x3_edge_worker.py as a script), one after the other.
"""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import conv3x3_edge_worker as Wk
import conv3x3_ref as R

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv3x3_edge_worker.py")
# a clean child takes 3-7 s on the MI355X, Python's and torch's start-up
# included; 5 x the slowest is 35 s, and 60 s is the least a child gets
CHILD_TIMEOUT = 60


@pytest.fixture(scope="module")
def ops():
    from ainp import ops as _ops
    return _ops


def _run(*args, **kw):
    """run_int; a HIP error ends the session: nothing more runs on that GPU."""
    try:
        return Wk.run_int(*args, **kw)
    except RuntimeError as e:
        pytest.exit(f"GPU error, the session ends here: {str(e)[:300]}", returncode=3)


def _report(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails)


# ------------------------------------------------------------------ integer cases
@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_integer_cases_every_element(ops, pair, prec):
    tally = {}
    fails = _run(ops, *pair, prec, R.shapes(), tally=tally)
    print(f"{pair} {prec}: {tally}")
    assert tally.get("served", 0) > 0 or prec == "st16"
    _report(fails)


@pytest.mark.parametrize("pair", R.SMALL_CL_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_integer_cases_small_wgrad_tile_kernel(ops, monkeypatch, pair):
    """AINP_SMALL_WGRAD_TILE=1 (read per call): the 8 x 48-tile weight gradient."""
    monkeypatch.setenv("AINP_SMALL_WGRAD_TILE", "1")
    _report(_run(ops, *pair, "fp32", R.shapes(), only=("wgrad",)))


@pytest.mark.parametrize("var,val,prec", [("AINP_X6S_FT3", "4", "fp32"), ("AINP_X6S_FT3", "8", "fp32"),
                                          ("AINP_X6S_FT1", "4", "st16"), ("AINP_X6S_FT1", "8", "st16"),
                                          ("AINP_X6S_FT1", "16", "st16"),
                                          ("AINP_X6S_FT1", "16", "bf16")])
def test_integer_cases_x6s_tile_rows(ops, monkeypatch, var, val, prec):
    """The 4-, 8- and 16-row tiles of conv3x3_wgrad_x6s (read per launch), on
    the model's pairs and, in fp32, as one pass of a mixed weight gradient."""
    monkeypatch.setenv(var, val)
    fails = []
    for pair in [(16, 32), (32, 16)] + ([(48, 16), (64, 16)] if prec == "fp32" else []):
        fails += _run(ops, *pair, prec, R.shapes(), only=("wgrad",))
    _report(fails)


# ------------------------------------------------------------------ real cases
# split-bf16 routes that need the analytic bound instead of the floor rule
# (none: DESIGN.md, "Edge-shape tests", has the measured figures)
ANALYTIC = set()


def _dev(t):
    return None if t is None else t.to("cuda")


def _floor(tag, got, ref64, ref32, worst, key, bound):
    """within_floor, printed with the share of the analytic first-order bound
    `bound` that the worst element uses; a route in ANALYTIC passes on that
    bound where the floor rule does not hold."""
    got = got.float().cpu()
    dev, floor, ok = R.within_floor(got, ref64, ref32)
    scale = float(ref64.abs().max())
    allowed = 4.0 * floor + 4e-7 * scale
    share = dev / allowed if allowed > 0 else 0.0
    line = f"{tag}: dev {dev:.3e} floor {floor:.3e} max|ref| {scale:.3e} share {share:.2f}"
    ashare = float(((got.double() - ref64).abs() / bound.clamp_min(1e-300)).max())
    worst[key + ".analytic"] = max(worst.get(key + ".analytic", 0.0), ashare)
    print(line + f" analytic share {ashare:.2f}")
    w = worst.setdefault(key, [0.0, 0.0, 0.0])
    if scale > 0:
        w[0], w[1], w[2] = max(w[0], dev / scale), max(w[1], floor / scale), max(w[2], share)
    if not bool(torch.isfinite(got).all()):
        return False
    return ok or (key in ANALYTIC and ashare <= 1.0)


def _each(tag, got, ref, tol=1e-6):
    got, ref = got.double().cpu(), ref.double()
    rel = float(((got - ref).abs() / ref.abs()).max())
    print(f"{tag}: rel {rel:.3e}")
    return bool(torch.isfinite(got).all()) and rel <= tol


REAL = [(p, "fp32") for p in R.PAIRS] + [(p, "bf16") for p in R.X6_MODEL_PAIRS]


@pytest.mark.parametrize("pair,prec", REAL, ids=lambda v: str(v).replace(" ", ""))
def test_real_cases_within_floor(ops, pair, prec):
    cin, cout = pair
    b16 = prec == "bf16"
    fails, worst = [], {}
    u = 2.0 ** -24
    for N, H, W in R.shapes(R.REAL_PLANES):
        c = R.real_case(cin, cout, N, H, W)
        x, w, b, dy = c["x"], c["w"], c["bias"], c["dy"]
        xd, wd, bd, dyd = _dev(x), _dev(w), _dev(b), _dev(dy)
        dx64 = R.dgrad_ref(dy, w, bf16=b16 and R.conv_is_x6(cout, cin))
        dx32 = R.dgrad_ref(dy, w, bf16=b16 and R.conv_is_x6(cout, cin), dtype=torch.float32)
        dxb = (9 * cout + 8) * u * torch.nn.grad.conv2d_input(x.shape, w.double().abs(),
                                                              dy.double().abs(), padding=1)
        tag = f"({cin},{cout}) {prec} N={N} {H}x{W}"
        dx = ops.conv3x3_dgrad(dyd, wd, bf16=b16)
        kx = f"{'x6' if R.conv_is_x6(cout, cin) else 'f32'}-dgrad"
        if not _floor(f"{tag} dx", dx, dx64, dx32, worst, f"{cout}>{cin}:{kx}", dxb):
            fails.append(f"{tag} dx")
        for pro in (True, False):
            sc, sh = (c["scale"], c["shift"]) if pro else (None, None)
            t = f"{tag} pro={int(pro)}"
            fb = b16 and R.conv_is_x6(cin, cout)
            y64, s64 = R.fwd_ref(x, w, b, sc, sh, bf16=fb)
            y32, _ = R.fwd_ref(x, w, b, sc, sh, bf16=fb, dtype=torch.float32)
            a = R.act(x.double(), sc, sh)
            yb = (9 * cin + 8) * u * torch.nn.functional.conv2d(a.abs(), w.double().abs(),
                                                                b.double().abs(), padding=1)
            y, stats = ops.conv3x3_fwd(xd, wd, bd, _dev(sc), _dev(sh), want_stats=True, bf16=b16)
            kf = f"{'x6' if R.conv_is_x6(cin, cout) else 'f32'}-fwd"
            if not _floor(f"{t} y", y, y64, y32, worst, f"{cin}>{cout}:{kf}", yb):
                fails.append(f"{t} y")
            if not _each(f"{t} sum y / sum y^2", stats.sum(0), s64):
                fails.append(f"{t} stats")
            dw64, db64 = R.wgrad_ref(x, dy, sc, sh, bf16=b16)
            dw32, _ = R.wgrad_ref(x, dy, sc, sh, bf16=b16, dtype=torch.float32)
            dwb = (N * H * W + 8) * u * torch.nn.grad.conv2d_weight(a.abs(), w.shape,
                                                                    dy.double().abs(), padding=1)
            dw, db = ops.conv3x3_wgrad(xd, dyd, _dev(sc), _dev(sh), bf16=b16)
            x6w = any(R.wgrad_pass_is_x6(cp, cout) for _, cp in R.wgrad_passes(cin))
            if not _floor(f"{t} dw", dw, dw64, dw32, worst, f"{cin}>{cout}:{'x6' if x6w else 'f32'}-wgrad",
                          dwb):
                fails.append(f"{t} dw")
            if not _each(f"{t} db", db, db64):
                fails.append(f"{t} db")
    for k, v in worst.items():
        print(f"WORST ({cin},{cout}) {prec} {k}: {v}")
    _report(fails)


# ------------------------------------------------------------------ child processes
_ended_badly = []


@pytest.mark.parametrize("name", list(R.CHILD_SETTINGS))
def test_env_switched_routes_in_a_fresh_process(name, tmp_path):
    """One child per setting, one after the other; the inherited environment
    plus the one variable.  A child that ends by signal, abort or time limit
    fails, and no later child is started on that GPU."""
    if _ended_badly:
        pytest.skip(f"an earlier child ended badly ({_ended_badly[0]}): nothing more is started "
                    "on a GPU that has just faulted")
    var, val, _, pairs, precs = R.CHILD_SETTINGS[name]
    specs = [f"{a}x{b}:{p}" for a, b in pairs for p in precs]
    out = tmp_path / "failures.json"
    t0 = time.time()
    try:
        proc = subprocess.run([sys.executable, WORKER, str(out), "child", *specs],
                              env=dict(os.environ, **{var: val}), timeout=CHILD_TIMEOUT,
                              capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _ended_badly.append(f"{var}={val}: time limit of {CHILD_TIMEOUT} s")
        pytest.fail(_ended_badly[0])
    print(f"{var}={val}: {time.time() - t0:.1f} s; {proc.stdout.strip().splitlines()[-1:]}")
    if proc.returncode not in (0, 1) or not out.exists():
        _ended_badly.append(f"{var}={val}: exit status {proc.returncode}")
        pytest.fail(_ended_badly[0] + "\n" + proc.stderr[-2000:])
    fails = json.loads(out.read_text())
    assert isinstance(fails, list) and (proc.returncode == 0) == (not fails)
    _report(fails)
