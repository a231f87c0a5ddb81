"""Host-side tests of window-wise Janssen on whole signals with any mask
(ainp.janssen.plan_windows_mask / janssen_windowed_mask; the argument checks of
the gather and the overlap-add, which it shares with the per-gap layout, are in
tests/test_cpu_janssen_windowed.py) and of their test-only reference
tests/janssen_windowed_mask_ref.py.  No GPU.

test_reference_bounds_the_parity_cases re-measures, on the cases of the GPU
parity test, what the bound 1e-9 * max|clean missing| rests on: every row
completes all its iterations, Cholesky against LU moves the result by at most
1e-10 of the largest missing sample, rounding the input to float32 by at least
1e-8.  DESIGN §14 records the figures.
"""
import inspect

import numpy as np
import pytest

import janssen_ref as R
import janssen_windowed_mask_ref as WM
import janssen_windowed_ref as W

def _plan(name, wtypes=("hann",)):
    from ainp.janssen import plan_windows_mask
    w, a, p, _, _, _, _ = WM.CASES[name]
    return plan_windows_mask([WM.case_mask(name)], p=p, w=w, a=a, wtypes=wtypes)


def _reference_rows(name):
    """The missing positions of every window of the reference's loop that has
    some, not all, samples missing, by window."""
    w, a, _, _, n, _, _ = WM.CASES[name]
    L = -(-n // a) * a + (-(-w // a) - 1) * a
    data = np.zeros(L)
    data[:n][~WM.case_mask(name)] = np.nan
    rows = {}
    for s in range(L // a):
        nan = np.isnan(data[np.mod(s * a - w // 2 + np.arange(w), L)])
        if nan.any() and not nan.all():
            rows[s] = np.flatnonzero(nan)
    return rows


def _plan_rows(plan):
    """window -> missing positions, as the plan's tables give them."""
    rows = {}
    for r in range(len(plan)):
        if r < plan.n_one:
            where = np.arange(plan.gap_start[r], plan.gap_start[r] + plan.gap_len[r])
            assert plan.miss_off[r] == plan.miss_off[r + 1]
        else:
            where = plan.miss_idx[plan.miss_off[r]:plan.miss_off[r + 1]]
            assert plan.gap_len[r] == 0
        rows[int(plan.row_tab[r, 4])] = where
    return rows


@pytest.mark.parametrize("name", list(WM.CASES))
def test_planner_rows_are_the_reference_windows(name):
    plan = _plan(name)
    want = _reference_rows(name)
    got = _plan_rows(plan)
    assert sorted(got) == sorted(want)
    for s in want:
        assert np.array_equal(got[s], want[s]), (name, s)
    w, a, _, _, n, runs, _ = WM.CASES[name]
    L = -(-n // a) * a + (w // a - 1) * a
    assert np.all(plan.row_tab[:, 0] == n) and np.all(plan.row_tab[:, 3] == L)
    assert np.all(plan.row_tab[:, 1] == 0) and np.all(plan.row_tab[:, 2] == n)
    # one-run rows first, each part in window order; the table finds every row
    assert np.all(np.diff(plan.row_tab[:plan.n_one, 4]) > 0)
    assert np.all(np.diff(plan.row_tab[plan.n_one:, 4]) > 0)
    assert len(plan.win_row) == L // a
    for r in range(len(plan)):
        assert plan.win_row[plan.row_tab[r, 4]] == r
    assert np.count_nonzero(plan.win_row >= 0) == len(plan)
    assert plan.run_tab.tolist() == [[e - s, s, L, 0, 0] for s, e in runs]
    assert plan.run_off.tolist() == [s for s, _ in runs]
    assert np.array_equal(plan.missing, (~WM.case_mask(name)).astype(np.uint8))


def test_row_counts_and_the_split():
    counts = {name: (len(p), len(p) - p.n_one) for name, p in
              ((name, _plan(name)) for name in WM.CASES)}
    assert counts["two_runs_one_window"] == (5, 3)
    assert counts["both_ends"] == (8, 0)
    assert counts["wrap_row_both_ends"] == (5, 1)
    assert counts["every_9th"] == (13, 13)
    assert counts["single_gap"][1] == 0 and counts["single_gap"][0] == 5
    assert counts["wrap_w192"][1] >= 2
    # a run of 2100: the windows inside it have no row
    plan = _plan("long_run")
    w, a = 64, 16
    inside = [s for s in range(len(plan.win_row))
              if s * a - w // 2 >= 400 and s * a + w // 2 <= 2500]
    assert len(inside) > 100 and np.all(plan.win_row[inside] == -1)
    assert plan.run_tab[0, 0] == 2100


def test_the_wrap_row_lists_the_tail_before_the_head():
    plan = _plan("wrap_row_both_ends")
    assert len(plan) - plan.n_one == 1
    r = plan.n_one
    # n = 508, L = 540, window 35 starts at 503: the tail [505, 508) at 2 .. 4,
    # then, through the wrap, the head [0, 4) at 37 .. 40
    assert plan.row_tab[r].tolist() == [508, 0, 508, 540, 35, 0]
    assert plan.lists()[0].tolist() == [2, 3, 4, 37, 38, 39, 40]
    assert plan.win_row[35] == r


def test_planner_batches_shapes_and_signals():
    from ainp.janssen import plan_windows_mask
    names = ("two_runs_one_window", "single_gap")
    masks = [WM.case_mask(n) for n in names]
    plan = plan_windows_mask(masks, p=32, w=256, a=64, wtypes=("Hann", "RECT", "tukey"))
    assert plan.wtypes == ("hann", "rect", "tukey") and plan.total == 3 * 4000
    assert len(plan) == 3 * (5 + 5) and plan.n_one == 3 * (2 + 5)
    assert plan.gana.shape == plan.gsyn.shape == (3, 256)
    S = (2000 // 64 + 1) + 3
    assert len(plan.win_row) == 6 * S and len(plan.missing) == plan.total
    assert plan.run_tab[:, 3].tolist() == [0, 0, S, 2 * S, 2 * S, 3 * S, 4 * S, 4 * S, 5 * S]
    assert plan.run_tab[:, 4].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert plan.run_signal.tolist() == [0, 0, 1] * 3
    assert plan.run_off.tolist() == [k * 4000 + o for k in range(3) for o in (900, 960, 2900)]
    for r in range(len(plan)):
        _, _, _, _, win, k = plan.row_tab[r]
        i = (plan.sig_off[r] - k * 4000) // 2000
        assert plan.win_row[(k * 2 + i) * S + win] == r


def test_refusals():
    from ainp.janssen import janssen_windowed, janssen_windowed_mask, plan_windows_mask
    x = WM.case_signal("two_runs_one_window")
    m = WM.case_mask("two_runs_one_window")
    with pytest.raises(ValueError, match="divide"):
        janssen_windowed_mask(x, m, p=32, w=256, a=60)
    with pytest.raises(ValueError, match="w / a"):
        janssen_windowed_mask(x, m, p=32, w=256, a=256)
    with pytest.raises(ValueError, match="w must be in"):
        janssen_windowed_mask(x, m, p=256, w=256, a=64)
    with pytest.raises(ValueError, match="w must be in"):
        janssen_windowed_mask(x, m, p=32, w=32768, a=1024)
    with pytest.raises(ValueError, match="wtype"):
        janssen_windowed_mask(x, m, p=32, w=256, a=64, wtype="hamming")
    with pytest.raises(ValueError, match="wtype"):
        janssen_windowed_mask(x, m, p=32, w=256, a=64, wtype=())
    with pytest.raises(ValueError, match="method"):
        janssen_windowed_mask(x, m, p=32, w=256, a=64, method="yule")
    with pytest.raises(ValueError):
        janssen_windowed_mask(x, m, p=0, w=256, a=64)
    with pytest.raises(ValueError):
        janssen_windowed_mask(x, m, p=32, w=256, a=64, maxit=0)
    with pytest.raises(ValueError, match="not positive"):     # tukeywin(2) is [0, 0]
        plan_windows_mask([m], p=1, w=2, a=1, wtypes=("hann", "tukey"))
    big = np.ones(40000, bool)
    big[20000:22100] = False
    with pytest.raises(ValueError, match="at most 2048"):     # 2100 missing in one window
        plan_windows_mask([big], p=32, w=8192, a=2048)
    big[21000:21100] = True                                   # two runs of 1000: 2000 in a window
    assert len(plan_windows_mask([big], p=32, w=8192, a=2048)) > 0
    assert len(_plan("long_run")) > 0                         # a run of 2100, <= 52 per window
    # what the per-gap planner refuses stays refused there
    with pytest.raises(ValueError, match="second gap"):
        janssen_windowed(x, m, p=32, w=256, a=64)


def test_signatures_and_registration():
    import torch
    from ainp import _lib, ops
    from ainp.janssen import janssen_windowed, janssen_windowed_mask, plan_windows_mask
    from models import model_eval
    import models.AudioReg as AR
    assert AR.janssen_windowed_mask is janssen_windowed_mask
    assert "janssen_windowed_mask" in AR.__all__
    sig = inspect.signature(janssen_windowed_mask)
    assert list(sig.parameters.items())[0][0] == "signal"
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == \
        [(k, v.default) for k, v in inspect.signature(janssen_windowed).parameters.items()][1:]
    assert list(inspect.signature(plan_windows_mask).parameters) == \
        ["masks", "p", "w", "a", "wtypes"]
    ev = inspect.signature(model_eval.run_janssen_windowed_mask_evaluation).parameters
    assert [(k, v.default) for k, v in ev.items()][2:] == [
        ("gaps", ((2.0, 0.08),)), ("p", 512), ("w", 4096), ("a", 1024), ("wtype", "hann"),
        ("maxit", 20), ("method", "lpc")]
    # one gather and one overlap-add for every plan: the any-mask pair is gone
    for name in ("janssen_windows_mask", "janssen_ola_mask"):
        assert not hasattr(ops, name) and not hasattr(torch.ops.ainp, name)
        assert not hasattr(_lib.lib, "ainp_" + name)
    for name in ("janssen_windows", "janssen_ola"):
        assert callable(getattr(ops, name)) and hasattr(torch.ops.ainp, name)
        assert hasattr(_lib.lib, "ainp_" + name)


# ------------------------------------------------------------ the reference
@pytest.mark.parametrize("wtype", WM.WTYPES)
def test_reference_agrees_with_the_one_gap_reference(wtype):
    """On single_gap every window holds one run: the dense-Cholesky loop and
    janssen_windowed_ref.segmentation_inp (janssen_ref.janssen per window) on
    the same whole signal agree to 1e-12 relative, and both return the observed
    samples."""
    w, a, p, maxit, n, ((s0, e0),), _ = WM.CASES["single_gap"]
    x = WM.case_signal("single_gap")
    clean = x.copy()
    x[s0:e0] = np.nan
    mine, done = WM.segmentation_inp(x, p, maxit, w, a, wtype)
    theirs = W.segmentation_inp(x, p, maxit, w, a, wtype)
    assert mine.shape == theirs.shape == (n, maxit) and done == [maxit] * 5
    scale = np.max(np.abs(clean[s0:e0]))
    d = np.max(np.abs(mine[s0:e0] - theirs[s0:e0])) / scale
    print(f"single_gap {wtype}: the two references differ by {d:.2e}")
    assert d <= 1e-12
    obs = np.ones(n, bool)
    obs[s0:e0] = False
    assert np.max(np.abs(mine[obs] - clean[obs, None])) <= 1e-15


BOUND_CASES = [(name, t, "lpc") for name in WM.CASES for t in WM.WTYPES] + \
              [(name, t, "arburg") for name in list(WM.CASES)[:2] for t in WM.WTYPES]


def test_reference_bounds_the_parity_cases():
    """The GPU parity bound is 1e-9 * max|clean missing|.  Re-measured from the
    committed reference, on every case, shape and method of the GPU test:
    every row completes all maxit iterations; Cholesky against LU moves the
    result by at most 1e-10 of the largest missing sample (measured 9.5e-11,
    sample_and_run / hann); rounding the input to float32 moves it by at least
    1e-8 (measured 2.2e-8, sample_and_run / rect).  The bound is >= 10 times
    above the solver spread and >= 10 times below a float32 step."""
    worst, least = (0.0, None), (np.inf, None)
    for name, wtype, method in BOUND_CASES:
        maxit = WM.CASES[name][3]
        scale = np.max(np.abs(WM.case_signal(name)[~WM.case_mask(name)]))
        chol, done = WM.case_reference(name, wtype, method)
        assert done and all(k == maxit for k in done), (name, wtype, method)
        assert np.all(np.isfinite(chol)) and chol.shape[0] == maxit
        lu, _ = WM.case_reference(name, wtype, method, solver="lu")
        f32, _ = WM.case_reference(name, wtype, method, dtype=np.float32)
        d = np.max(np.abs(chol - lu)) / scale
        f = np.max(np.abs(chol - f32)) / scale
        print(f"{name} {wtype} {method}: Cholesky vs LU {d:.2e}, float32 input {f:.2e}")
        assert d <= 1e-10, (name, wtype, method)
        assert f >= 1e-8, (name, wtype, method)
        worst, least = max(worst, (d, (name, wtype))), min(least, (f, (name, wtype)))
    print(f"solver spread at most {worst[0]:.2e} {worst[1]}; float32 moves at least "
          f"{least[0]:.2e} {least[1]}")
