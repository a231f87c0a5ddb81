"""Host-side tests of S-SPAIN with the OMP coefficient update: the test-only
reference tests/spain_omp_ref.py, the refusals and the clipped default maxit of
ainp.spain, and the argument checks of ainp_spain_omp.  No GPU.

OMP takes discrete decisions: which atom, whether the residual is under its
target, whether a pivot is too small, and the loop around it whether the
objective is under epsilon.  Round-off flips one only where two magnitudes, a
residual and its target, a pivot and its floor, or an objective and epsilon
nearly meet.  test_parity_inputs_are_well_conditioned asserts, on the reference
alone, that no input the GPU parity tests use comes near any of them;
test_two_formulations_bound_the_parity_bound that the bound 1e-9 * max|clean
gap| lies at least 10x above what two float64 least-squares solvers differ by
and at least 10x below what float32 input moves.  DESIGN §14.3 records the
figures both print.  Measured: smallest margin 1.0e-5, residual-stop distance
1.27, epsilon distance 4.1e-3, relative squared pivot 1.9e-3, largest condition
number 2.0e2; the two solvers differ by at most 4.9e-15, float32 input moves at
least 3.7e-8, pass counts unchanged by both.
"""
import ctypes
import inspect

import numpy as np
import pytest

import janssen_ref as R
import spain_omp_ref as O
import spain_ref as S


def _runs():
    """Every (tag, reference dict, epsilon) the GPU parity tests compare with."""
    for (case, eps, errdb, kw), tag in zip(O.PARITY, O.PARITY_IDS):
        yield tag, O.case_reference(case, eps, errdb, kw), eps
    yield "largest", O.big_reference(), 0.1
    yield "wide row", O.wide_reference(), O.WIDE["epsilon"]


# ---------------------------------------------------------- the reference
def test_parity_inputs_are_well_conditioned():
    """At every inner step of every pass of every window of every GPU parity
    run: selection margin >= 1e-8, residual-stop distance >= 1e-6, relative
    squared pivot >= 1e-6, and per pass |obj - epsilon| / epsilon >= 1e-6."""
    worst = dict(margin=np.inf, resid=np.inf, pivot=np.inf, eps=np.inf, cond=0.0)
    for tag, ref, eps in _runs():
        c = O.conditions(ref["stats"], eps)
        print(f"{tag}: margin {c['margin']:.2e}, residual stop {c['resid']:.2e}, pivot "
              f"{c['pivot']:.2e}, epsilon {c['eps']:.2e}, condition {c['cond']:.2e}, stops "
              f"{sorted(c['stops'])}, passes {ref.get('iters', len(ref['obj']))}")
        assert c["margin"] >= 1e-8, tag
        assert c["resid"] >= 1e-6, tag
        assert c["pivot"] >= 1e-6, tag
        assert c["eps"] >= 1e-6, tag
        for key in ("margin", "resid", "pivot", "eps"):
            worst[key] = min(worst[key], c[key])
        worst["cond"] = max(worst["cond"], c["cond"])
    print("worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_two_formulations_bound_the_parity_bound():
    lo, hi = 0.0, np.inf
    for (case, eps, errdb, kw), tag in zip(O.PARITY, O.PARITY_IDS):
        s0, e0 = case[2], case[3]
        scale = np.max(np.abs(S.case_signal(case)[s0:e0]))
        one = O.case_reference(case, eps, errdb, kw)
        two = O.case_reference(case, eps, errdb, kw, solver="normal")
        f32 = O.case_reference(case, eps, errdb, kw, float32=True)
        d2 = np.max(np.abs(one["out"][s0:e0] - two["out"][s0:e0])) / scale
        d32 = np.max(np.abs(one["out"][s0:e0] - f32["out"][s0:e0])) / scale
        print(f"{tag}: lstsq against normal equations {d2:.2e}, float32 input {d32:.2e}, passes "
              f"{one['iters']}")
        assert two["iters"] == one["iters"] and np.array_equal(two["atoms"], one["atoms"]), tag
        assert f32["iters"] == one["iters"], tag
        assert 10.0 * d2 <= 1e-9 <= d32 / 10.0, tag
        lo, hi = max(lo, d2), min(hi, d32)
    print(f"two formulations at most {lo:.2e}, float32 input at least {hi:.2e}")
    # the row with 260 unknowns: the recorded row relative to its peak
    one, two = O.wide_reference(), O.wide_reference("normal")
    d2 = np.max(np.abs(one["rec"] - two["rec"])) / np.max(np.abs(one["rec"]))
    print(f"wide row: lstsq against normal equations {d2:.2e}, atoms {one['atoms']}")
    assert two["atoms"] == one["atoms"] == [130, 130] and 10.0 * d2 <= 1e-9


def test_w64_small_epsilon_fills_the_block():
    """(64, 16, [301, 321)) at epsilon 1e-3 goes on until 32 atoms bring w = 64
    real unknowns.  No call goes past w: 32 two-column atoms fit a block exactly
    (the residual rule ends the call), and with DC among them the 63 unknowns
    leave no room for another pair (the dimension rule does)."""
    ref = O.case_reference(S.CASES[0], 1e-3, -120.0)
    assert ref["atoms"].max() == 32
    for seed, stop, dc in ((1, "residual", False), (0, "dimension", True)):
        st = []
        v = np.random.default_rng(seed).standard_normal(64)
        zb, chosen = O.omp(v, 128, 40, -200.0, stats=st)
        assert st[0]["stop"] == stop and len(chosen) == 32 and (0 in chosen) == dc
        assert 64 not in chosen


def test_orthonormal_atoms_return_the_analysis_coefficients():
    """red = 1: the atoms are orthonormal, so the least squares returns A v on
    the chosen support."""
    rng = np.random.default_rng(2)
    for w, k in ((64, 5), (64, 20), (128, 33)):
        v = rng.standard_normal(w)
        zb, chosen = O.omp(v, w, k, -300.0)
        av = S.analysis(v, w)
        d = np.max(np.abs(zb[chosen] - av[chosen]))
        print(f"w {w}, k {k}: {d:.2e}")
        assert len(chosen) == k and d <= 1e-13
        off = np.ones(w, bool)
        off[chosen] = False
        off[[(-m) % w for m in chosen]] = False
        assert np.all(zb[off] == 0.0)


def test_a_sparse_block_stops_on_the_residual_with_its_atoms():
    w, M = 64, 128
    for bins, k in (([5, 40], 6), ([0, 17, 64], 5), ([3, 9, 33, 50], 5)):
        z = np.zeros(M // 2 + 1, complex)
        for j, m in enumerate(bins):
            z[m] = (1.0 + 0.3 * j) * (1.0 if m in (0, M // 2) else np.exp(0.7j * (j + 1)))
        v = np.real(S.synthesis(np.concatenate((z, np.conj(z[-2:0:-1]))), w))
        st = []
        zb, chosen = O.omp(v, M, k, -200.0, stats=st)
        assert st[0]["stop"] == "residual" and sorted(chosen) == bins and len(bins) < k
        assert np.max(np.abs(zb[:M // 2 + 1] - z)) <= 1e-12
    st = []
    zb, chosen = O.omp(np.zeros(w), M, 3, stats=st)
    assert st[0]["stop"] == "residual" and chosen == [] and not zb.any()


def test_plain_magnitudes_and_ties_to_the_lower_bin():
    """Neither DC nor Nyquist is rescaled: on the flat spectrum of a unit
    impulse the first atom is m = 0 (H_k, which halves DC, takes m = 1)."""
    row, obs, g0, h = S.tie_row(64)
    st = []
    zb, chosen = O.omp(row, 128, 1, stats=st)
    assert chosen == [0] and st[0]["margin"][0] == 0.0
    assert np.flatnonzero(S.hard_threshold(S.analysis(row, 128), 1)).tolist() == [1, 127]


# ------------------------------------------------------------ the host layer
def test_refusals_and_the_clipped_default():
    from ainp.spain import (check_omp_args, default_maxit, f_update_id, omp_default_maxit, omp_k,
                            spain_inpaint)
    x = R.sinusoid_mix(2000)
    m = np.ones(2000, bool)
    m[900:980] = False
    with pytest.raises(ValueError, match="algorithm='sspain'"):
        spain_inpaint(x, m, algorithm="aspain", w=256, a=64, f_update="OMP")
    with pytest.raises(ValueError, match="algorithm='sspain'"):
        spain_inpaint(x, m, w=256, a=64, f_update="omp")          # the default is A-SPAIN
    with pytest.raises(ValueError, match="f_update"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="mp")
    with pytest.raises(ValueError, match="f_update"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update=None)
    with pytest.raises(ValueError, match="omp_errdb"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="OMP", omp_errdb=1.0)
    with pytest.raises(ValueError, match="omp_errdb"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="OMP", omp_errdb=-301.0)
    with pytest.raises(ValueError, match="omp_errdb"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="OMP",
                      omp_errdb=float("nan"))
    with pytest.raises(ValueError, match="512 real unknowns"):
        spain_inpaint(x, m, algorithm="SSPAIN", w=1024, a=256, f_update="OMP", maxit=257)
    with pytest.raises(ValueError, match="maxit"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="OMP", maxit=258)
    with pytest.raises(ValueError, match="red"):
        spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="OMP", red=3)
    assert f_update_id("h") == "H" and f_update_id("Omp") == "OMP"
    assert f_update_id("H", "aspain") == "H"
    # k(cnt) = s (1 + cnt // r - 1 // r)
    assert [omp_k(c) for c in (1, 2, 7)] == [1, 2, 7]
    assert [omp_k(c, 2, 3) for c in (1, 2, 3, 5, 6)] == [2, 2, 4, 4, 6]
    assert all(omp_k(c, s, r) == O.omp_k(c, s, r) for c in range(1, 40) for s in (1, 3)
               for r in (1, 2, 5))
    # every w <= 512 is free of the cap; above, the default stops where k = 256
    for w, red in ((64, 2), (256, 4), (512, 2)):
        assert omp_default_maxit(w, red) == default_maxit(w, red)
        assert check_omp_args(w, red) == default_maxit(w, red)
    assert omp_default_maxit(1024) == 256 and omp_default_maxit(4096, 2) == 256
    assert omp_default_maxit(4096, 2, 2, 1) == 128 and omp_default_maxit(4096, 2, 1, 2) == 511
    assert omp_default_maxit(4096, 2, 3, 4) == 339         # k(339) = 3 * 85 = 255, k(340) = 258
    for w, s, r in ((1024, 1, 1), (4096, 2, 1), (4096, 1, 2), (4096, 3, 4), (2048, 256, 3)):
        mx = check_omp_args(w, 2, s, r)
        assert mx == omp_default_maxit(w, 2, s, r) >= 1
        assert 2 * omp_k(mx, s, r) <= 512 < 2 * omp_k(mx + 1, s, r) or mx == default_maxit(w, 2, s, r)
    with pytest.raises(ValueError, match="leaves no pass"):
        check_omp_args(4096, 2, 257, 1)
    assert check_omp_args(1024, 2, 1, 1, 0.1, 256) == 256


def test_the_options_are_keyword_only_and_h_is_the_default():
    """spain_inpaint keeps its parameter list; f_update and omp_errdb come after
    it, by keyword only.  Each refusal below is raised before any device work."""
    import ainp.spain as sp
    from models import model_eval
    import models.AudioReg as AR
    assert AR.spain_inpaint is sp.spain_inpaint
    assert list(inspect.signature(sp.spain_inpaint).parameters)[-1] == "device"
    x = R.sinusoid_mix(2000)
    m = np.ones(2000, bool)
    m[900:980] = False
    seen = []
    orig = sp._spain_inpaint
    sp._spain_inpaint = lambda *a, **kw: seen.append(kw)
    try:
        sp.spain_inpaint(x, m, "sspain", 256, 64)
        sp.spain_inpaint(x, m, algorithm="sspain", w=256, a=64, f_update="omp", omp_errdb=-60.0)
        with pytest.raises(TypeError):        # 13 positional parameters, no more
            sp.spain_inpaint(x, m, "sspain", 256, 64, "hann", 2, 1, 1, 0.1, None, False, "cuda",
                             "OMP")
        with pytest.raises(TypeError):
            sp.spain_inpaint(x, m, f_updat="OMP")
    finally:
        sp._spain_inpaint = orig
    assert [(k["f_update"], k["omp_errdb"]) for k in seen] == [("H", -40.0), ("omp", -60.0)]
    assert seen[0]["algorithm"] == "sspain" and seen[0]["w"] == 256 and seen[0]["maxit"] is None
    assert seen[1]["device"] == "cuda" and seen[1]["return_history"] is False
    assert model_eval.SPAIN_ALGORITHMS == ("aspain", "sspain")
    assert not any("omp" in name.lower() for name in AR.__all__)


def test_ops_spain_omp_refuses_cpu_tensors():
    import torch
    from ainp import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.spain_omp(torch.zeros(2, 64, dtype=torch.float64), [3, 4], [5, 6])


# ---------------------------------------------------------------- the C ABI
ONE = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced


def test_spain_omp_bad_arguments_fail_without_launching():
    from ainp import _lib
    assert {"ainp_spain_omp", "ainp_spain_omp_workspace"} <= set(_lib.EXPORTED)
    order = ["sol", "n_rows", "stride", "gap_start", "gap_len", "w", "red", "s", "r", "epsilon",
             "maxit", "errdb", "iters", "obj_history", "n_atoms", "workspace", "ws_bytes", "stream"]
    good = dict(sol=ONE, n_rows=4, stride=256, gap_start=ONE, gap_len=ONE, w=256, red=2, s=1, r=1,
                epsilon=0.1, maxit=257, errdb=-40.0, iters=ONE, obj_history=None, n_atoms=None,
                workspace=ONE, ws_bytes=1 << 30, stream=None)
    big = dict(w=1024, stride=1024)
    einval = [(dict(sol=None), b"bad argument"), (dict(gap_start=None), b"bad argument"),
              (dict(gap_len=None), b"bad argument"), (dict(iters=None), b"bad argument"),
              (dict(n_rows=-1), b"bad argument"),
              (dict(w=200), b"power of two"), (dict(w=4), b"power of two"),
              (dict(w=8192, stride=8192), b"power of two"),
              (dict(red=3), b"red 1, 2 or 4"), (dict(w=4096, red=4, stride=4096), b"red * w <= 8192"),
              (dict(stride=255), b"stride >= w"),
              (dict(s=0), b"s >= 1"), (dict(r=0), b"r >= 1"),
              (dict(maxit=0), b"1 <= maxit"), (dict(maxit=258), b"1 <= maxit"),
              (dict(epsilon=-1e-9), b"epsilon >= 0"), (dict(epsilon=float("nan")), b"epsilon >= 0"),
              (dict(errdb=0.5), b"-300 <= errdb <= 0"), (dict(errdb=-300.5), b"-300 <= errdb <= 0"),
              (dict(errdb=float("nan")), b"-300 <= errdb <= 0"),
              (dict(big, maxit=257), b"512 real unknowns"),
              (dict(big, maxit=129, s=2), b"512 real unknowns"),
              (dict(big, maxit=513, r=2), b"512 real unknowns"),
              (dict(ws_bytes=8), b"workspace"), (dict(workspace=None), b"workspace")]
    for kw, rule in einval:
        a = dict(good, **kw)
        assert _lib.lib.ainp_spain_omp(*(a[k] for k in order)) == -1, kw        # AINP_EINVAL
        msg = _lib.lib.ainp_last_error()
        assert b"ainp_spain_omp" in msg and rule in msg, (kw, msg)
    # an empty batch is a no-op, still no launch; so is the cap where it just holds
    for kw in (dict(n_rows=0), dict(n_rows=0, workspace=None, ws_bytes=0),
               dict(big, n_rows=0, maxit=256), dict(big, n_rows=0, maxit=511, r=2),
               dict(w=512, stride=512, n_rows=0, maxit=513)):
        a = dict(good, **kw)
        assert _lib.lib.ainp_spain_omp(*(a[k] for k in order)) == 0, kw


def test_spain_omp_workspace_is_a_host_call():
    """A row's packed inverse Cholesky factor: D (D + 1) / 2 doubles, D = min(w, 512)."""
    from ainp import _lib
    q = _lib.lib.ainp_spain_omp_workspace
    assert q(0, 64, 2) == 0 and q(1, 200, 2) == 0 and q(1, 4096, 4) == 0 and q(-1, 64, 2) == 0
    assert q(1, 64, 2) == 64 * 65 // 2 * 8 and q(3, 256, 4) == 3 * 256 * 257 // 2 * 8
    assert q(1, 512, 1) == q(1, 4096, 2) == 512 * 513 // 2 * 8 == (1 << 20) + 2048
    assert q(256, 4096, 2) == 256 * 512 * 513 // 2 * 8
