"""Host-side tests of the window-wise Janssen rows (ainp.janssen.plan_windows /
janssen_windowed, the argument checks of ainp_janssen_windows and
ainp_janssen_ola, models/model_eval.run_ar_evaluation) and of their test-only
reference tests/janssen_windowed_ref.py.  No GPU.

test_reference_solvers_bound_the_parity_shapes measures, at the shapes the GPU
parity test uses, what two independent float64 solvers differ by and what
rounding the input to float32 moves; DESIGN §14 records the figures.
"""
import ctypes
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest

import janssen_ref as R
import janssen_windowed_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the known answers of the support: (w, a, [s0, e0)) -> 0-based [lo, hi)
SUPPORTS = [((256, 64, 900, 980), (652, 1228)),
            ((128, 32, 531, 555), (431, 655)),
            ((256, 64, 1000, 1300), (798, 1502)),
            ((64, 16, 301, 302), (245, 357)),
            ((64, 16, 350, 440), (291, 499)),
            ((128, 64, 400, 440), (324, 516)),
            ((256, 64, 30, 110), (-218, 358))]


def _mask(n, *gaps):
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


@pytest.mark.parametrize("case,want", SUPPORTS)
def test_support_known_answers(case, want):
    from ainp.janssen import gap_support
    w, a, s0, e0 = case
    assert gap_support(s0, e0, w, a) == want
    assert W.support(s0, e0, w, a) == want
    assert (want[1] - want[0]) % a == 0


@pytest.mark.parametrize("w,a", [(256, 64), (128, 64), (45, 15)])
def test_window_identities(w, a):
    from ainp.janssen import window_pair, window_rescale
    for make in (window_pair, W.windows):
        gana, gsyn = make("hann", w, a)
        assert np.max(np.abs(window_rescale(gana, gsyn, a) - 1.0)) <= 1e-15
        gana, gsyn = make("rect", w, a)
        assert np.all(gana == 1.0)
        assert np.max(np.abs(window_rescale(gana, gsyn, a) - w / (2 * a))) <= 1e-15
        gana, gsyn = make("tukey", w, a)
        assert np.array_equal(gana, gsyn) and np.all(window_rescale(gana, gsyn, a) > 0)
    for t in W.WTYPES:         # the planner's windows are the reference's
        for mine, ref in zip(window_pair(t.upper(), w, a), W.windows(t, w, a)):
            assert np.max(np.abs(mine - ref)) <= 4e-16, t


@pytest.mark.parametrize("wtype", W.WTYPES)
def test_reference_returns_an_ungapped_signal(wtype):
    x = R.sinusoid_mix(576, noise=1e-3)
    out = W.segmentation_inp(x, 32, 2, 256, 64, wtype)
    assert out.shape == (576, 2)
    assert np.max(np.abs(out - x[:, None])) <= 1e-15


def _reference_rows(n, s0, e0, w, a):
    """(start, length) of the missing run of every window of the reference's
    loop that has some, not all, samples missing, and the number that has all."""
    lo, hi = W.support(s0, e0, w, a)
    sup = np.zeros(hi - lo)
    sup[s0 - lo:e0 - lo] = np.nan
    L = -(-len(sup) // a) * a + (-(-w // a) - 1) * a
    data = np.concatenate((sup, np.zeros(L - len(sup))))
    rows, full = [], 0
    for s in range(L // a):
        nan = np.isnan(data[np.mod(s * a - w // 2 + np.arange(w), L)])
        if nan.all():
            full += 1
        elif nan.any():
            where = np.flatnonzero(nan)
            rows.append((int(where[0]), len(where)))
    return rows, full


def test_planner_rows_are_the_reference_windows():
    from ainp.janssen import plan_windows
    plan = plan_windows([_mask(2000, (900, 980))], p=32, w=256, a=64, wtypes=("hann",))
    rows = list(zip(plan.gap_start.tolist(), plan.gap_len.tolist()))
    assert rows == [(248, 8), (184, 72), (120, 80), (56, 80), (0, 72), (0, 8)]
    assert (rows, 0) == _reference_rows(2000, 900, 980, 256, 64)
    assert plan.gap_tab.tolist() == [[80, 248, 768, 0, 6, 0]]
    assert plan.row_tab[:, :4].tolist() == [[2000, 652, 576, 768]] * 6
    assert plan.row_tab[:, 4].tolist() == [2, 3, 4, 5, 6, 7]

    plan = plan_windows([_mask(800, (350, 440))], p=8, w=64, a=16, wtypes=("hann",))
    rows = list(zip(plan.gap_start.tolist(), plan.gap_len.tolist()))
    want, full = _reference_rows(800, 350, 440, 64, 16)
    assert rows == want and len(rows) == 8 and rows[0] == (59, 5) and rows[-1] == (0, 5)
    assert full == 2           # two windows lie inside the gap: no row, counted by the rescale
    windows = plan.row_tab[:, 4]
    assert len(set(range(windows[0], windows[-1] + 1)) - set(windows.tolist())) == full

    for case in W.CASES:       # every parity case, negative and overhanging supports included
        w, a, s0, e0, p, _, n = case
        plan = plan_windows([_mask(n, (s0, e0))], p=p, w=w, a=a, wtypes=("rect",))
        rows = list(zip(plan.gap_start.tolist(), plan.gap_len.tolist()))
        assert rows == _reference_rows(n, s0, e0, w, a)[0], case


def test_planner_batches_shapes_signals_and_gaps():
    from ainp.janssen import plan_windows
    masks = [_mask(3000, (900, 980), (2000, 2050)), _mask(2500, (1200, 1230))]
    plan = plan_windows(masks, p=32, w=256, a=64, wtypes=("Hann", "RECT", "tukey"))
    assert plan.wtypes == ("hann", "rect", "tukey") and plan.total == 3 * 5500
    assert len(plan.gap_off) == 9 and plan.gana.shape == plan.gsyn.shape == (3, 256)
    assert plan.gap_off.tolist() == [k * 5500 + o for k in range(3) for o in (900, 2000, 4200)]
    assert plan.gap_signal.tolist() == [0, 0, 1] * 3
    row0 = np.concatenate(([0], np.cumsum(plan.gap_tab[:, 4])))
    assert plan.gap_tab[:, 3].tolist() == row0[:-1].tolist() and row0[-1] == len(plan)
    for g in range(9):         # a gap's rows: ascending windows of its own signal and shape
        r = slice(row0[g], row0[g + 1])
        assert np.all(np.diff(plan.row_tab[r, 4]) > 0)
        assert np.all(plan.row_tab[r, 5] == g // 3)
        assert np.all(plan.sig_off[r] == (g // 3) * 5500 + (0, 0, 3000)[g % 3])


def test_refusals():
    from ainp.janssen import janssen_windowed, plan_windows
    x = R.sinusoid_mix(2000)
    m = _mask(2000, (900, 980))
    with pytest.raises(ValueError, match="divide"):
        janssen_windowed(x, m, p=32, w=256, a=60)
    with pytest.raises(ValueError, match="w / a"):
        janssen_windowed(x, m, p=32, w=256, a=256)
    with pytest.raises(ValueError, match="w must be in"):
        janssen_windowed(x, m, p=256, w=256, a=64)
    with pytest.raises(ValueError, match="w must be in"):
        janssen_windowed(x, m, p=32, w=32768, a=1024)
    with pytest.raises(ValueError, match="second gap"):       # [1100, 1110) is in [652, 1228)
        janssen_windowed(x, _mask(2000, (900, 980), (1100, 1110)), p=32, w=256, a=64)
    with pytest.raises(ValueError, match="wtype"):
        janssen_windowed(x, m, p=32, w=256, a=64, wtype="hamming")
    with pytest.raises(ValueError, match="wtype"):
        janssen_windowed(x, m, p=32, w=256, a=64, wtype=("hann", "hamming"))
    with pytest.raises(ValueError, match="wtype"):
        janssen_windowed(x, m, p=32, w=256, a=64, wtype=())
    with pytest.raises(ValueError, match="method"):
        janssen_windowed(x, m, p=32, w=256, a=64, method="yule")
    with pytest.raises(ValueError):
        janssen_windowed(x, m, p=0, w=256, a=64)
    with pytest.raises(ValueError, match="at most 2048"):     # a run of 2100 in one window
        plan_windows([_mask(40000, (20000, 22100))], p=32, w=8192, a=2048)
    # the windows that hold the gap reach [652, 1228): a neighbour from 1484 on, whose own
    # windows start at 1229, is no obstacle
    assert len(plan_windows([_mask(2000, (900, 980), (1484, 1490))], p=32, w=256, a=64)) == 6 + 4


def _plan_gen():
    spec = importlib.util.spec_from_file_location(
        "gen_window_plans", os.path.join(GOLDEN, "gen_window_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


plan_gen = _plan_gen()


@pytest.fixture(scope="module")
def golden_plans():
    with open(os.path.join(GOLDEN, "window_plans.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(plan_gen.CASES)
    return want


@pytest.mark.parametrize("name", list(plan_gen.CASES))
def test_plans_unchanged(name, golden_plans):
    """plan_segments, plan_windows and plan_spain_windows give the tables -- every
    field's values, dtype and shape -- or the ValueError text that the package
    gave before the planners shared one row loop (tests/golden/window_plans.json)."""
    got = plan_gen.run_case(name)
    assert sorted(got) == sorted(golden_plans[name])
    for field, want in golden_plans[name].items():
        assert got[field] == want, (name, field)


def test_model_eval_refuses_unknown_algorithms(tmp_path):
    from models import model_eval
    for bad in ("janssen_hamming", "spain", "hann"):
        with pytest.raises(ValueError, match="algorithm"):
            model_eval.run_ar_evaluation(str(tmp_path), str(tmp_path / "o"), algorithm=bad)
    with pytest.raises(ValueError, match="method"):
        model_eval.run_ar_evaluation(str(tmp_path), str(tmp_path / "o"),
                                     algorithm="janssen_hann", method="yule")


def test_signatures_and_defaults():
    from ainp import ops
    from ainp.janssen import janssen_windowed, plan_windows
    from models import model_eval
    import models.AudioReg as AR
    assert AR.janssen_windowed is janssen_windowed and "janssen_windowed" in AR.__all__
    sig = inspect.signature(janssen_windowed)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("mask", None), ("p", 512), ("w", 4096), ("a", 1024), ("wtype", "hann"), ("maxit", 20),
        ("method", "lpc"), ("return_history", False), ("device", "cuda")]
    assert list(sig.parameters)[0] == "signal"
    ev = inspect.signature(model_eval.run_ar_evaluation).parameters
    assert list(ev) == ["input_dir", "output_dir", "algorithm", "method", "p", "w", "maxit", "a"]
    assert ev["a"].default == 1024 and ev["algorithm"].default == "janssen"
    assert list(inspect.signature(plan_windows).parameters) == ["masks", "p", "w", "a", "wtypes"]
    assert callable(ops.janssen_windows) and callable(ops.janssen_ola)


# ---------------------------------------------------------------- the C ABI
ONE = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced


def _check(f, name, order, good, einval, empty):
    from ainp import _lib

    def call(**kw):
        a = dict(good, **kw)
        return f(*(a[k] for k in order))

    for kw in einval:
        assert call(**kw) == -1, kw                               # AINP_EINVAL
        assert name in _lib.lib.ainp_last_error(), kw
    assert call(**empty) == 0            # an empty batch is a no-op, still no launch


def test_janssen_windows_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ["signals", "missing", "total", "sig_off", "row_tab", "n_rows", "w", "a", "gana",
             "n_shapes", "sol", "stride", "stream"]
    good = dict(signals=ONE, missing=ONE, total=1000, sig_off=ONE, row_tab=ONE, n_rows=4, w=256,
                a=64, gana=ONE, n_shapes=1, sol=ONE, stride=256, stream=None)
    einval = [dict(signals=None), dict(missing=None), dict(sig_off=None), dict(row_tab=None),
              dict(gana=None), dict(sol=None), dict(total=0), dict(n_rows=-1), dict(a=60),
              dict(a=0), dict(a=256), dict(w=1, a=1), dict(w=32768, a=1024, stride=32768),
              dict(n_shapes=0), dict(stride=255), dict(n_rows=1 << 31)]
    _check(_lib.lib.ainp_janssen_windows, b"ainp_janssen_windows", order, good, einval,
           dict(n_rows=0))


def test_janssen_ola_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ["sol", "n_rows", "stride", "row_history", "maxit", "hist_stride", "row_tab",
             "gap_start", "gap_len", "miss_off", "miss_idx", "n_idx", "win_row", "n_tab",
             "unit_off", "unit_tab", "n_units", "h_max", "w", "a", "gana", "gsyn", "n_shapes",
             "signals", "total", "history", "out_stride", "stream"]
    good = dict(sol=ONE, n_rows=6, stride=256, row_history=ONE, maxit=5, hist_stride=80,
                row_tab=ONE, gap_start=ONE, gap_len=ONE, miss_off=ONE, miss_idx=ONE, n_idx=40,
                win_row=ONE, n_tab=35, unit_off=ONE, unit_tab=ONE, n_units=2, h_max=80, w=256,
                a=64, gana=ONE, gsyn=ONE, n_shapes=1, signals=ONE, total=2000, history=ONE,
                out_stride=80, stream=None)
    einval = [dict(sol=None), dict(row_tab=None), dict(gap_start=None), dict(gap_len=None),
              dict(miss_off=None), dict(miss_idx=None), dict(win_row=None), dict(unit_off=None),
              dict(unit_tab=None), dict(gana=None), dict(gsyn=None), dict(signals=None),
              dict(total=0), dict(n_rows=-1), dict(n_units=-1), dict(n_idx=-1), dict(n_tab=-1),
              dict(a=60), dict(a=256), dict(w=32768, a=1024, stride=32768), dict(n_shapes=0),
              dict(stride=255), dict(h_max=0), dict(h_max=2001, out_stride=2001),
              dict(h_max=2049, out_stride=2049), dict(history=None), dict(row_history=None),
              dict(maxit=0), dict(maxit=1001), dict(hist_stride=0), dict(out_stride=79),
              dict(n_units=1 << 31), dict(n_rows=1 << 31),
              dict(h_max=1 << 24, total=1 << 25, out_stride=1 << 24)]
    _check(_lib.lib.ainp_janssen_ola, b"ainp_janssen_ola", order, good, einval,
           dict(n_units=0))
    # without a history neither maxit nor the strides matter
    assert _lib.lib.ainp_janssen_ola(*(dict(good, n_units=0, history=None, row_history=None,
                                            maxit=0, hist_stride=0, out_stride=0)[k]
                                       for k in order)) == 0


# ------------------------------------------------- the bound of the GPU test
def test_reference_solvers_bound_the_parity_shapes():
    """The GPU parity bound is 1e-9 * max|clean gap|.  It holds only where two
    correct float64 solvers agree well inside it (<= 3e-10) and float32 input
    would miss it by far (a quarter of its movement stays above 1e-9): dense
    Cholesky with FFT autocorrelation (janssen_ref) against solve_toeplitz
    with direct sums, every history column.  Measured: solvers <= 1.8e-10
    (hann, (256, 64, [1000, 1300))), rect <= 2.8e-11; float32 2.2e-8 .. 1.3e-6."""
    worst, least = 0.0, np.inf
    for case in W.CASES:
        _, _, s0, e0, _, _, _ = case
        scale = np.max(np.abs(W.case_signal(case)[s0:e0]))
        for wtype in W.WTYPES:
            dense = W.case_reference(case, wtype)
            assert np.all(np.isfinite(dense)) and dense.shape == (case[5], e0 - s0)
            d = np.max(np.abs(dense - W.case_reference(case, wtype, solver="toeplitz"))) / scale
            f = np.max(np.abs(dense - W.case_reference(case, wtype, dtype=np.float32))) / scale
            print(f"{case[:4]} {wtype}: solvers {d:.2e}, float32 input {f:.2e}")
            assert d <= 3e-10, (case, wtype)
            assert f / 4 > 1e-9, (case, wtype)
            worst, least = max(worst, d), min(least, f)
    print(f"two float64 solvers differ by at most {worst:.2e}; float32 moves at least {least:.2e}")
