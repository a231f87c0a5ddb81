"""Independent float64 transcription of the reference project's
models/AudioReg/utils/segmentation_inp.m with saveall, called the way it is
written: on a whole signal with any NaN pattern, for the tests only.  numpy
alone.

A dense loop over every window of the padded signal; every window with missing
samples, in however many runs, goes through janssen_mask_ref.janssen (the dense
Cholesky of janssen_inp.m) or, with solver="lu", through the same iteration
with np.linalg.solve on the same matrix -- the second solver that measures
what two correct float64 solvers differ by.  Windows come from
janssen_windowed_ref.windows.  It shares nothing with
ainp.janssen.plan_windows_mask or csrc/janssen_windows.hip: no row tables, no
routing by the number of runs, no window-to-row table.
"""
import math

import numpy as np

import ar_ref
import janssen_mask_ref as M
import janssen_ref
import janssen_windowed_ref as W


def janssen_lu(x, miss, p, maxit, fit=janssen_ref.lpc):
    """janssen_mask_ref.janssen with the missing samples from an LU solve
    (np.linalg.solve) of the same |M| x |M| matrix."""
    x = np.array(x, np.float64)
    n = len(x)
    miss = np.asarray(miss, np.int64)
    obs = np.setdiff1d(np.arange(n), miss)
    sol = x.copy()
    sol[miss] = 0.0
    dist = np.abs(miss[:, None] - np.arange(n)[None, :])
    near = dist <= p
    history = []
    for _ in range(maxit):
        if not np.any(sol):
            break
        try:
            a = fit(sol, p)
        except ZeroDivisionError:
            break
        b = np.array([np.dot(a[:p + 1 - k], a[k:]) for k in range(p + 1)])
        AA = np.zeros(dist.shape)
        AA[near] = b[dist[near]]
        sol[miss] = -np.linalg.solve(AA[:, miss], AA[:, obs] @ x[obs])
        history.append(sol[miss].copy())
    return sol, np.array(history).reshape(len(history), len(miss)), len(history)


def segmentation_inp(signal, p, maxit, w, a, wtype, method="lpc", solver="chol"):
    """signal float64 [n] with NaN on the missing samples -> (restored
    [n, maxit], the iterations each window with some, not all, samples missing
    completed, in window order).  A window that stops early has NaN in the
    columns it did not reach, as MATLAB."""
    fit = ar_ref.arburg if method.lower() == "arburg" else janssen_ref.lpc
    solve = {"chol": M.janssen, "lu": janssen_lu}[solver]
    n = len(signal)
    L = math.ceil(n / a) * a + (math.ceil(w / a) - 1) * a
    data = np.concatenate((signal, np.zeros(L - n)))
    gana, gsyn = W.windows(wtype, w, a)
    rescale = np.zeros(L)
    restored = np.zeros((L, maxit))
    done = []
    for s in range(L // a):
        idx = np.mod(s * a - w // 2 + np.arange(w), L)
        seg = data[idx] * gana
        nan = np.isnan(seg)
        if nan.all():
            out = np.zeros((w, maxit))
        elif not nan.any():
            out = np.repeat(seg[:, None], maxit, axis=1)
        else:
            where = np.flatnonzero(nan)
            clean = np.where(nan, 0.0, seg)
            _, hist, k = solve(clean, where, p, maxit, fit)
            done.append(k)
            out = np.repeat(clean[:, None], maxit, axis=1)
            out[where, :k] = hist.T
            out[where, k:] = np.nan
        rescale[idx] += gana * gsyn
        restored[idx] += out * gsyn[:, None]
    return (restored / rescale[:, None])[:n], done


# The parity cases: name -> (w, a, p, maxit, n, runs of missing samples, seed).
CASES = {
    "two_runs_one_window": (256, 64, 32, 5, 2000, ((900, 930), (960, 985)), 201),
    "every_9th": (128, 32, 16, 5, 1200, tuple((c, c + 1) for c in range(400, 700, 9)), 202),
    "both_ends": (256, 64, 32, 5, 1000, ((0, 20), (985, 1000)), 203),
    "all_missing_window": (64, 16, 8, 3, 800, ((350, 440), (460, 470)), 204),
    "w_over_a_2": (128, 64, 16, 4, 900, ((400, 440), (470, 480)), 205),
    "odd_w": (45, 15, 8, 3, 500, ((200, 210), (220, 223)), 206),
    "single_gap": (256, 64, 32, 5, 2000, ((900, 980),), 207),
    "sample_and_run": (128, 32, 16, 5, 1500, ((300, 301), (340, 380), (1000, 1060)), 208),
    "wrap_row_both_ends": (45, 15, 8, 3, 508, ((0, 4), (505, 508)), 209),
    "wrap_w192": (192, 64, 24, 4, 1020, ((0, 10), (500, 530), (540, 550), (1010, 1020)), 210),
    "long_run": (64, 16, 8, 3, 3000, ((400, 2500), (2520, 2530)), 211),
}
WTYPES = W.WTYPES
_cache = {}


def case_signal(name):
    n, seed = CASES[name][4], CASES[name][6]
    return janssen_ref.sinusoid_mix(n, noise=1e-3, seed=seed)


def case_mask(name):
    """Boolean, True where observed."""
    mask = np.ones(CASES[name][4], bool)
    for s0, e0 in CASES[name][5]:
        mask[s0:e0] = False
    return mask


def case_reference(name, wtype, method="lpc", solver="chol", dtype=np.float64):
    """(the missing samples of a parity case after every iteration, [maxit,
    number missing] in signal order; iterations completed per row), computed
    once per (case, shape, method, solver, input precision) and shared."""
    key = (name, wtype, method, solver, np.dtype(dtype).name)
    if key not in _cache:
        w, a, p, maxit, _, _, _ = CASES[name]
        x = case_signal(name).astype(dtype).astype(np.float64)
        mask = case_mask(name)
        x[~mask] = np.nan
        res, done = segmentation_inp(x, p, maxit, w, a, wtype, method, solver)
        out = res[~mask].T.copy()
        out.setflags(write=False)
        _cache[key] = (out, tuple(done))
    return _cache[key]
