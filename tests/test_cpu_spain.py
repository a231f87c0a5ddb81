"""Host-side tests of A-SPAIN / S-SPAIN: the planner and the refusals of
ainp.spain, the argument checks of ainp_spain, the exports, and the test-only
reference tests/spain_ref.py.  No GPU.

The hard threshold is discontinuous: a change the size of round-off flips a
selection only at a near-tie, and ends the loop one pass early or late only
where an objective lies at epsilon.  test_parity_inputs_are_well_conditioned
asserts, on the reference alone, that no input the GPU parity tests use comes
near either; test_two_formulations_bound_the_parity_bound that the bound
1e-9 * max|clean gap| lies between what two float64 formulations of the
transforms differ by and what float32 input moves.  DESIGN §14 records the
figures both print.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest

import janssen_ref as R
import spain_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")


def _mask(n, *gaps):
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


def _runs():
    """Every (tag, reference dict, epsilon) the GPU parity tests compare with."""
    for case, alg, eps in S.PARITY:
        yield f"{alg} {case} eps {eps}", S.case_reference(case, alg, eps), eps
    for case, kw in S.OTHER:
        for alg in S.ALGS:
            yield f"{alg} {case} {kw}", S.case_reference(case, alg, 0.1, **kw), 0.1
    for alg in S.ALGS:
        yield f"{alg} {S.LONG_GAP}", S.case_reference(S.LONG_GAP, alg), 0.1
        yield f"{alg} largest", S.big_reference(alg), 0.1


# ---------------------------------------------------------- the reference
def test_parity_inputs_are_well_conditioned():
    """At every evaluated iteration of every window of every GPU parity run: the
    k-th and the (k+1)-th ranked magnitude are at least 1e-8 apart (relative;
    two exact zeros are exempt), and the objective is at least 1e-6 (relative)
    from epsilon.  Measured: smallest margin 1.7e-6 (sspain, (64, 16, 100,
    190, 400), epsilon 0.1), smallest distance 6.0e-5."""
    worst_m, worst_d = np.inf, np.inf
    for tag, ref, eps in _runs():
        margin, dist = S.conditions(ref["stats"], eps)
        print(f"{tag}: margin {margin:.2e}, distance to epsilon {dist:.2e}")
        assert margin >= 1e-8, tag
        assert dist >= 1e-6, tag
        worst_m, worst_d = min(worst_m, margin), min(worst_d, dist)
    print(f"smallest margin {worst_m:.2e}, smallest distance to epsilon {worst_d:.2e}")


def test_two_formulations_bound_the_parity_bound():
    """The GPU parity bound is 1e-9 * max|clean gap|.  Two float64 formulations
    of the transforms (numpy's real FFT against the dense DFT-matrix product;
    at M 8192 against the written-out radix-2 FFT) must agree inside 1e-10 with
    the same iteration counts, and float32 input must move the result by more
    than the bound.  The float32 figure is not asked of the largest transform:
    with its 40 passes A-SPAIN's best objective is the first, so its result is
    the gapped row itself."""
    worst, least = 0.0, np.inf
    for case, alg, eps in S.PARITY:
        s0, e0 = case[2], case[3]
        scale = np.max(np.abs(S.case_signal(case)[s0:e0]))
        ref = S.case_reference(case, alg, eps)
        two = S.case_reference(case, alg, eps, transform="dense")
        f32 = S.case_reference(case, alg, eps, float32=True)
        d = np.max(np.abs(ref["out"][s0:e0] - two["out"][s0:e0])) / scale
        f = np.max(np.abs(ref["out"][s0:e0] - f32["out"][s0:e0])) / scale
        print(f"{alg} {case} eps {eps}: formulations {d:.2e}, float32 input {f:.2e}")
        assert ref["iters"] == two["iters"]
        assert d <= 1e-10 and f > 1e-9, (case, alg, eps)
        worst, least = max(worst, d), min(least, f)
    B = S.BIG
    scale = np.max(np.abs(S.big_signal()[0][B["s0"]:B["e0"]]))
    for alg in S.ALGS:
        ref, two = S.big_reference(alg), S.big_reference(alg, transform="radix2")
        d = np.max(np.abs(ref["out"] - two["out"])[B["s0"]:B["e0"]]) / scale
        d_obj = np.nanmax(np.abs(ref["obj"] - two["obj"]) / ref["obj"])
        print(f"{alg} largest: formulations {d:.2e} (objectives {d_obj:.2e})")
        assert ref["iters"] == two["iters"] and d <= 1e-10 and d_obj <= 1e-10
        worst = max(worst, d)
    print(f"two float64 formulations differ by at most {worst:.2e}; float32 moves at least "
          f"{least:.2e}")


def test_bundled_clip_two_formulations():
    """What the end-to-end GPU test takes its bound from: the two formulations
    on the bundled clip, w 1024, a 256, default solver parameters."""
    import utils
    audio, sr = utils.load_audio(os.path.join(FLAC, "81-121543-0008.flac"))
    audio = audio.astype(np.float64)
    s0, h = int(2.0 * sr), int(0.08 * sr)
    ref, two = S.clip_reference(audio, s0, s0 + h, 1024, 256)
    print(f"bundled clip: two formulations differ by {two:.2e} of max|gap|; end-to-end bound "
          f"{max(1e-8, 10 * two):.1e}; reference gap SDR {R.gap_sdr(audio, ref, s0, h):.3f} dB")
    assert np.array_equal(ref[:s0], audio[:s0]) and np.isfinite(two)


def test_transforms_agree_and_are_adjoint():
    rng = np.random.default_rng(3)
    x, M = rng.standard_normal(32), 128
    z = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    for t in ("dense", "radix2"):
        assert np.max(np.abs(S.analysis(x, M, t) - S.analysis(x, M))) <= 1e-13
        assert np.max(np.abs(S.synthesis(z, 32, t) - S.synthesis(z, 32))) <= 1e-13
    # <A x, z> = <x, A* z>, and A* A = red * identity on the block
    assert abs(np.vdot(z, S.analysis(x, M)) - np.vdot(S.synthesis(z, 32), x)) <= 1e-12
    assert np.max(np.abs(S.synthesis(S.analysis(x, M), 32) - x)) <= 1e-13


def test_hard_threshold_rules():
    z = np.zeros(16, complex)
    z[0], z[8] = 3.0, 2.0                     # DC ranks as 1.5, Nyquist as 2
    z[3] = z[13] = 1.8
    z[5], z[11] = 1.8j, -1.8j                 # ties with bin 3: the lower index first
    out = S.hard_threshold(z, 1)
    assert out[8] == 2.0 and np.count_nonzero(out) == 1
    out = S.hard_threshold(z, 2)
    assert out[3] == 1.8 and out[13] == 1.8 and out[5] == 0 and np.count_nonzero(out) == 3
    out = S.hard_threshold(z, 3)
    assert out[5] == 1.8j and out[11] == -1.8j and out[0] == 0
    out = S.hard_threshold(z, 4)
    assert out[0] == 3.0                      # restored in full
    assert np.array_equal(S.hard_threshold(z, 9), z) and np.array_equal(S.hard_threshold(z, 50), z)


def test_tie_row_is_a_tie_once_and_the_rule_matters(monkeypatch):
    """The row of the GPU tie test: the first selection is an exact tie of
    non-zero magnitudes, every later one is at least 1e-8 clear, and sending
    the tie to the higher index instead moves the second objective by more than
    1e-6 -- so the objectives tell which bin was kept."""
    row, obs, _, _ = S.tie_row()
    for alg, solver in (("aspain", S.aspain), ("sspain", S.sspain)):
        for red in (1, 2):
            stats = []
            _, objs = solver(row, obs, red=red, epsilon=1e-3, maxit=4, stats=stats)
            margins = stats[0][0]
            assert len(objs) == 4 and margins[0] == 0.0 and min(margins[1:]) >= 1e-8
            assert min(abs(o - 1e-3) / 1e-3 for o in objs) >= 1e-6
            monkeypatch.setattr(S, "TIES_TO_THE_LOWER_INDEX", False)
            _, other = solver(row, obs, red=red, epsilon=1e-3, maxit=4)
            monkeypatch.setattr(S, "TIES_TO_THE_LOWER_INDEX", True)
            moved = abs(other[1] - objs[1]) / objs[1]
            print(f"{alg} red {red}: margins {['%.1e' % m for m in margins]}, the other rule "
                  f"moves the second objective by {moved:.2e}")
            assert moved > 1e-6


@pytest.mark.parametrize("alg", S.ALGS)
def test_recovers_a_sparse_signal(alg):
    """Two on-bin cosines are 2-sparse in the frame with red = 1.  With s = 2 and
    r = 33 the loop runs at k = 2 throughout and ends within epsilon of a
    2-sparse signal that equals x on the 52 observed of 64 samples.  The frame
    is unitary here, so that signal is within epsilon / sigma of x, sigma^2 >=
    1 - 2 * 12 / 64 the least share of a two-bin signal's energy on the observed
    samples: the error is at most (1 + 1 / sigma) epsilon < 3 epsilon.  Bound:
    10 epsilon."""
    w, eps = 64, 1e-8
    n = np.arange(w)
    x = np.cos(2 * np.pi * 5 * n / w + 0.4) + 0.5 * np.cos(2 * np.pi * 12 * n / w + 1.0)
    obs = _mask(w, (20, 32))
    solver = S.aspain if alg == "aspain" else S.sspain
    rec, objs = solver(np.where(obs, x, 0.0), obs, red=1, s=2, r=33, epsilon=eps, maxit=33)
    d = np.max(np.abs(rec - x))
    print(f"{alg}: {len(objs)} passes, last objective {objs[-1]:.2e}, error {d:.2e}")
    assert objs[-1] <= eps and d <= 10 * eps and np.array_equal(rec[obs], x[obs])


# ------------------------------------------------------------ the planner
def _brute_rows(obs, w, a):
    """(window, first missing, missing count) of every window of the
    reference's loop with some, not all, samples missing."""
    Ls = len(obs)
    L = -(-Ls // a) * a + (-(-w // a) - 1) * a
    miss = np.concatenate((~obs, np.zeros(L - Ls, bool)))
    rows = []
    for n in range(L // a):
        m = miss[(n * a - w // 2 + np.arange(w)) % L]
        if m.any() and not m.all():
            where = np.flatnonzero(m)
            rows.append((n, int(where[0]), len(where)))
    return rows, L


def test_planner_rows_are_the_brute_force_windows():
    from ainp.spain import plan_spain_windows
    for case in S.CASES + [S.LONG_GAP, (128, 64, 3, 40, 300), (64, 16, 580, 600, 600)]:
        w, a, s0, e0, n = case
        obs = _mask(n, (s0, e0))
        plan = plan_spain_windows([obs], w, a)
        rows, L = _brute_rows(obs, w, a)
        got = list(zip(plan.row_tab[:, 4].tolist(), plan.gap_start.tolist(),
                       plan.gap_len.tolist()))
        assert got == rows, case
        assert plan.row_tab[:, :4].tolist() == [[n, 0, n, L]] * len(rows)
        assert plan.gap_tab.tolist() == [[e0 - s0, s0, L, 0, len(rows), 0]]
        assert plan.gap_off.tolist() == [s0] and plan.gap_range.tolist() == [[s0, e0]]
        assert plan.wtypes == ("hann",) and plan.gana.shape == plan.gsyn.shape == (1, w)
        assert plan.row_tab[:, 4].tolist() == S.case_reference(case, "aspain")["windows"] \
            if case in S.CASES else True
    plan = plan_spain_windows([_mask(2000, (900, 980))], 256, 64)
    assert list(zip(plan.gap_start.tolist(), plan.gap_len.tolist())) == [
        (196, 60), (132, 80), (68, 80), (4, 80), (0, 20)]
    assert plan.gap_tab.tolist() == [[80, 900, 2240, 0, 5, 0]]


def test_planner_batches_signals_and_gaps():
    from ainp.spain import plan_spain_windows
    masks = [_mask(3000, (900, 980), (2000, 2050)), _mask(2500, (1200, 1230)), _mask(500)]
    plan = plan_spain_windows(masks, 256, 64)
    assert plan.total == 6000 and plan.gap_off.tolist() == [900, 2000, 4200]
    assert plan.gap_signal.tolist() == [0, 0, 1]
    row0 = np.concatenate(([0], np.cumsum(plan.gap_tab[:, 4])))
    assert plan.gap_tab[:, 3].tolist() == row0[:-1].tolist() and row0[-1] == len(plan)
    for g in range(3):
        r = slice(row0[g], row0[g + 1])
        assert np.all(np.diff(plan.row_tab[r, 4]) > 0)
        assert np.all(plan.sig_off[r] == (0, 0, 3000)[g])
    want = [r for m in masks for r in _brute_rows(m, 256, 64)[0]]
    assert list(zip(plan.row_tab[:, 4].tolist(), plan.gap_start.tolist(),
                    plan.gap_len.tolist())) == want
    assert len(plan_spain_windows([_mask(700)], 64, 16)) == 0


def test_refusals():
    from ainp.spain import plan_spain_windows, spain_inpaint
    x = R.sinusoid_mix(2000)
    m = _mask(2000, (900, 980))
    with pytest.raises(ValueError, match="second gap"):       # 200 apart under windows of 256
        plan_spain_windows([_mask(2000, (900, 980), (1180, 1190))], 256, 64)
    assert len(plan_spain_windows([_mask(2000, (900, 980), (1300, 1310))], 256, 64)) == 5 + 4
    with pytest.raises(ValueError, match="longer than 2048"):
        plan_spain_windows([_mask(40000, (20000, 22100))], 4096, 1024)
    with pytest.raises(ValueError, match="power of two"):
        plan_spain_windows([m], 200, 50)
    with pytest.raises(ValueError, match="power of two"):
        plan_spain_windows([m], 8192, 2048)
    with pytest.raises(ValueError, match="power of two"):
        plan_spain_windows([m], 4, 2)
    with pytest.raises(ValueError, match="divide"):
        plan_spain_windows([m], 256, 60)
    with pytest.raises(ValueError, match="w / a"):
        plan_spain_windows([m], 256, 256)
    with pytest.raises(ValueError, match="red"):
        spain_inpaint(x, m, w=256, a=64, red=3)
    with pytest.raises(ValueError, match="red"):
        spain_inpaint(x, m, w=4096, a=1024, red=4)
    with pytest.raises(ValueError, match="wtype"):
        spain_inpaint(x, m, w=256, a=64, wtype="rect")
    with pytest.raises(ValueError, match="algorithm"):
        spain_inpaint(x, m, algorithm="pspain", w=256, a=64)
    with pytest.raises(ValueError, match="maxit"):
        spain_inpaint(x, m, w=256, a=64, maxit=258)
    with pytest.raises(ValueError, match="maxit"):
        spain_inpaint(x, m, w=256, a=64, maxit=0)
    with pytest.raises(ValueError, match="epsilon"):
        spain_inpaint(x, m, w=256, a=64, epsilon=-1.0)
    with pytest.raises(ValueError, match="s and r"):
        spain_inpaint(x, m, w=256, a=64, s=0)
    with pytest.raises(ValueError, match="differ in length"):
        spain_inpaint(x, m[:-1], w=256, a=64)


def test_model_eval_refuses_unknown_algorithms(tmp_path):
    from models import model_eval
    for bad in ("spain", "janssen", "ASPAIN-MOD"):
        with pytest.raises(ValueError, match="algorithm"):
            model_eval.run_spain_evaluation(str(tmp_path), str(tmp_path / "o"), algorithm=bad)


def test_exports_signatures_and_defaults():
    from ainp import _lib, ops
    from ainp.spain import default_maxit, plan_spain_windows, spain_inpaint
    from models import model_eval
    import models.AudioReg as AR
    assert AR.spain_inpaint is spain_inpaint and "spain_inpaint" in AR.__all__
    assert model_eval.SPAIN_ALGORITHMS == ("aspain", "sspain")
    assert model_eval.AR_ALGORITHMS == ("extrapolation", "janssen", "janssen_hann",
                                        "janssen_rect", "janssen_tukey")
    sig = inspect.signature(spain_inpaint)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("mask", None), ("algorithm", "aspain"), ("w", 4096), ("a", 1024), ("wtype", "hann"),
        ("red", 2), ("s", 1), ("r", 1), ("epsilon", 0.1), ("maxit", None),
        ("return_history", False), ("device", "cuda")]
    assert list(sig.parameters)[0] == "signal"
    ev = inspect.signature(model_eval.run_spain_evaluation).parameters
    assert list(ev) == ["input_dir", "output_dir", "algorithm", "w", "a", "solver"]
    assert (ev["algorithm"].default, ev["w"].default, ev["a"].default) == ("aspain", 4096, 1024)
    assert list(inspect.signature(plan_spain_windows).parameters) == ["masks", "w", "a"]
    assert callable(ops.spain)
    assert {"ainp_spain", "ainp_spain_workspace"} <= set(_lib.EXPORTED)
    # ceil(floor(w red / 2 + 1) r / s), no more than the loop can use
    assert default_maxit(4096) == 4097 and default_maxit(64, 2, 2, 1) == 33
    assert default_maxit(64, 2, 1, 3) == 65 and S.default_maxit(64, 2, 2, 3) == 65


def test_ops_spain_refuses_cpu_tensors():
    import torch
    from ainp import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.spain(torch.zeros(2, 64, dtype=torch.float64), [3, 4], [5, 6])


# ---------------------------------------------------------------- the C ABI
ONE = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced


def _check(f, name, order, good, einval, empty):
    from ainp import _lib

    def call(**kw):
        a = dict(good, **kw)
        return f(*(a[k] for k in order))

    for kw, rule in einval:
        assert call(**kw) == -1, kw                               # AINP_EINVAL
        msg = _lib.lib.ainp_last_error()
        assert name in msg and rule in msg, (kw, msg)
    assert call(**empty) == 0            # an empty batch is a no-op, still no launch


def test_spain_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ["sol", "n_rows", "stride", "gap_start", "gap_len", "w", "red", "algorithm", "s", "r",
             "epsilon", "maxit", "iters", "obj_history", "workspace", "ws_bytes", "stream"]
    good = dict(sol=ONE, n_rows=4, stride=256, gap_start=ONE, gap_len=ONE, w=256, red=2,
                algorithm=0, s=1, r=1, epsilon=0.1, maxit=257, iters=ONE, obj_history=None,
                workspace=None, ws_bytes=0, stream=None)
    einval = [(dict(sol=None), b"bad argument"), (dict(gap_start=None), b"bad argument"),
              (dict(gap_len=None), b"bad argument"), (dict(iters=None), b"bad argument"),
              (dict(n_rows=-1), b"bad argument"),
              (dict(algorithm=2), b"AINP_SPAIN_A"), (dict(algorithm=-1), b"AINP_SPAIN_A"),
              (dict(w=200), b"power of two"), (dict(w=4), b"power of two"),
              (dict(w=8192, stride=8192), b"power of two"),
              (dict(red=3), b"red 1, 2 or 4"), (dict(red=0), b"red 1, 2 or 4"),
              (dict(w=4096, red=4, stride=4096), b"red * w <= 8192"),
              (dict(stride=255), b"stride >= w"),
              (dict(s=0), b"s >= 1"), (dict(r=0), b"r >= 1"),
              (dict(maxit=0), b"1 <= maxit"), (dict(maxit=258), b"1 <= maxit"),
              (dict(epsilon=-1e-9), b"epsilon >= 0"), (dict(epsilon=float("nan")), b"epsilon >= 0"),
              (dict(ws_bytes=8, workspace=None), b"workspace")]
    _check(_lib.lib.ainp_spain, b"ainp_spain", order, good, einval, dict(n_rows=0))


def test_spain_workspace_is_a_host_call():
    from ainp import _lib
    for alg in (0, 1):
        assert _lib.lib.ainp_spain_workspace(0, 8, 1, alg) == 0
        assert _lib.lib.ainp_spain_workspace(1 << 20, 4096, 2, alg) == 0
