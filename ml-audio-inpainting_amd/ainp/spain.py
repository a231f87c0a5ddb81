"""Host side of the sparsity-based row of the reference's model comparison
(models/AudioReg/references/spain: spain_segmentation.m driving aspain.m or
sspain.m with f_update = 'H' or 'OMP'), restated without LTFAT: DESIGN §14.1,
§14.3 for the OMP update.

spain_segmentation pads the whole signal to a circular length L, cuts a window
of w samples every a samples and runs SPAIN on every window with missing
samples.  Here every such window, of every gap and signal, is one row of one
ainp_spain launch (csrc/spain.hip, float64; ainp_spain_omp of
csrc/spain_omp.hip with f_update "OMP") between the gather and the
overlap-add of csrc/janssen_windows.hip, whose tables the plan gives
(WindowPlan.tables: the signal is its own support, every gap a unit).
"""
from __future__ import annotations

import functools
import inspect

import numpy as np

from .gaps import (_cdiv, _normalise, check_shift, find_gaps, restack, solve_windows, window_pairs,
                   window_plan, window_rows)
from .janssen import GAP_MAX

ALGORITHMS = {"aspain": 0, "sspain": 1}      # AINP_SPAIN_A, AINP_SPAIN_S
W_MIN, W_MAX, M_MAX = 8, 4096, 8192          # csrc/spain.hip SP_WMIN, SP_WMAX, SP_MMAX
REDS = (1, 2, 4)
F_UPDATES = ("H", "OMP")                     # sspain.m's param.f_update
OMP_DIMS = 512                               # csrc/ar_limits.h AINP_SPAIN_OMP_DIMS
OMP_ERRDB_MIN = -300.0


def algorithm_id(algorithm):
    """param.algorithm ("aspain" | "sspain", any case) -> the ABI's id."""
    key = algorithm.lower() if isinstance(algorithm, str) else algorithm
    if key not in ALGORITHMS:
        raise ValueError(f"algorithm must be one of {sorted(ALGORITHMS)}, got {algorithm!r}")
    return ALGORITHMS[key]


def default_maxit(w, red=2, s=1, r=1):
    """ceil(floor(w red / 2 + 1) r / s), clipped to what the loop can use: with
    k >= M/2 + 1 the threshold keeps everything."""
    return min(_cdiv((w * red // 2 + 1) * r, s), w * red // 2 + 1)


def _check_w(w):
    if not (W_MIN <= w <= W_MAX and w & (w - 1) == 0):
        raise ValueError(f"w must be a power of two in [{W_MIN}, {W_MAX}], got w = {w}")


def check_window(w, a):
    w, a = int(w), int(a)
    _check_w(w)
    check_shift(w, a)
    return w, a


def check_args(w, red=2, s=1, r=1, epsilon=0.1, maxit=None):
    """The solver's range (ainp_spain's) -> maxit with the default filled in."""
    w, red = int(w), int(red)
    _check_w(w)
    if red not in REDS or red * w > M_MAX:
        raise ValueError(f"red must be one of {REDS} with red * w <= {M_MAX}, got red = {red}")
    if int(s) < 1 or int(r) < 1:
        raise ValueError("s and r must be at least 1")
    if not float(epsilon) >= 0.0:
        raise ValueError("epsilon must not be negative")
    if maxit is None:
        maxit = default_maxit(w, red, int(s), int(r))
    if not 1 <= int(maxit) <= red * w // 2 + 1:
        raise ValueError(f"maxit must be in [1, red * w / 2 + 1 = {red * w // 2 + 1}]")
    return int(maxit)


def f_update_id(f_update, algorithm="sspain"):
    """param.f_update ("H" | "OMP", any case) -> "H" or "OMP"; OMP is S-SPAIN's."""
    key = f_update.upper() if isinstance(f_update, str) else f_update
    if key not in F_UPDATES:
        raise ValueError(f"f_update must be one of {F_UPDATES}, got {f_update!r}")
    if key == "OMP" and algorithm_id(algorithm) != ALGORITHMS["sspain"]:
        raise ValueError("f_update 'OMP' is S-SPAIN's coefficient update: it needs "
                         "algorithm='sspain'")
    return key


def omp_k(cnt, s=1, r=1):
    """The number of atoms pass cnt may choose: s (1 + cnt // r - 1 // r)."""
    return int(s) * (1 + int(cnt) // int(r) - 1 // int(r))


def omp_default_maxit(w, red=2, s=1, r=1):
    """default_maxit, clipped so that min(2 k(maxit), w) <= OMP_DIMS."""
    w, s, r = int(w), int(s), int(r)
    maxit = default_maxit(w, red, s, r)
    if w > OMP_DIMS:
        # the largest cnt with s (1 + cnt // r - 1 // r) <= OMP_DIMS / 2
        q = OMP_DIMS // 2 // s - 1 + 1 // r
        maxit = min(maxit, q * r + r - 1)
    return maxit


def check_omp_args(w, red=2, s=1, r=1, epsilon=0.1, maxit=None, errdb=-40.0):
    """ainp_spain_omp's range -> maxit with the default filled in."""
    if maxit is None:
        check_args(w, red, s, r, epsilon, None)
        maxit = omp_default_maxit(w, red, s, r)
        if maxit < 1:
            raise ValueError(f"s = {s} leaves no pass with 2 k <= {OMP_DIMS} real unknowns "
                             f"at w = {w}")
    maxit = check_args(w, red, s, r, epsilon, maxit)
    if not OMP_ERRDB_MIN <= float(errdb) <= 0.0:
        raise ValueError(f"omp_errdb must be in [{OMP_ERRDB_MIN:g}, 0], got {errdb!r}")
    if min(2 * omp_k(maxit, s, r), int(w)) > OMP_DIMS:
        raise ValueError(f"f_update 'OMP' solves for at most {OMP_DIMS} real unknowns: "
                         f"min(2 k(maxit), w) = min({2 * omp_k(maxit, s, r)}, {int(w)}) with "
                         f"k(maxit) = s (1 + maxit // r - 1 // r)")
    return maxit


def plan_spain_windows(masks, w=4096, a=1024):
    """The batch layout of spain_segmentation.m for a list of boolean observed
    masks: a signal of Ls samples is its own support (origin 0), padded with
    observed zeros to L = ceil(Ls / a) a + (ceil(w / a) - 1) a; window n holds
    the circular indices (n a - floor(w / 2) + i) mod L.  One row per window
    with some, not all, samples missing; a window with all of them missing adds
    zeros and gets none.  Hann windows only.  ValueError for what is not
    covered: w no power of two in [8, 4096], a not dividing w, w / a < 2, a
    window that holds a second gap or two runs, a run of more than 2048."""
    w, a = check_window(w, a)
    pairs = window_pairs(("hann",), w, a, name_shape=False)
    gaps = []
    for i, obs in enumerate(masks):
        obs = np.asarray(obs, bool)
        Ls = len(obs)
        L = _cdiv(Ls, a) * a + (_cdiv(w, a) - 1) * a
        miss_any = np.zeros(L, bool)
        miss_any[:Ls] = ~obs
        for (g0, g1) in find_gaps(obs):
            if g1 - g0 > GAP_MAX:
                raise ValueError(f"signal {i}: gap [{g0}, {g1}) is longer than {GAP_MAX} samples")
            # the windows that can reach the gap: |n a - c| <= w / 2 for a sample c of it
            n_lo, n_hi = (g0 - w // 2) // a, _cdiv(g1 + w // 2, a)
            windows = sorted({n % (L // a) for n in range(n_lo, n_hi + 1)})
            gaps.append((0, i, g0, g1, 0, Ls, L,
                         list(window_rows(miss_any, g0, w, a, windows, i, g0, g1))))
    return window_plan(("hann",), w, a, pairs, masks, gaps)


def _spain_inpaint(signal, mask, algorithm, w, a, wtype, red, s, r, epsilon, maxit,
                   return_history, device, f_update, omp_errdb):
    from . import ops
    algorithm_id(algorithm)
    omp = f_update_id(f_update, algorithm) == "OMP"
    if not (isinstance(wtype, str) and wtype.lower() == "hann"):
        raise ValueError(f"wtype must be 'hann' (the only window SPAIN is set up for), "
                         f"got {wtype!r}")
    w, a = check_window(w, a)
    maxit = (check_omp_args(w, red, s, r, epsilon, maxit, omp_errdb) if omp
             else check_args(w, red, s, r, epsilon, maxit))
    sigs, masks, kind = _normalise(signal, mask)
    plan = plan_spain_windows(masks, w, a)
    atoms = []

    def solve(sol):
        if not omp:
            return ops.spain(sol, plan.gap_start, plan.gap_len, algorithm=algorithm, red=red,
                             s=s, r=r, epsilon=epsilon, maxit=maxit,
                             return_history=return_history)
        it, hist, na = ops.spain_omp(sol, plan.gap_start, plan.gap_len, red=red, s=s, r=r,
                                     epsilon=epsilon, maxit=maxit, errdb=omp_errdb,
                                     return_history=return_history)
        atoms.append(na)
        return it, hist

    (res,), iters, obj = solve_windows(sigs, plan, device, [(0, len(plan), solve)], per_gap=False)
    if obj is None and return_history:
        obj = np.zeros((0, maxit))           # an empty plan
    atoms = (atoms[0].cpu().numpy() if atoms and atoms[0] is not None
             else np.zeros((0, maxit), np.int32))
    info = []
    for g in range(len(plan.gap_off)):
        h, _, _, row0, nrows, _ = (int(v) for v in plan.gap_tab[g])
        g0, g1 = (int(v) for v in plan.gap_range[g])
        # a sample that only all-missing windows cover stays zero, as the reference gives
        info.append({"signal": int(plan.gap_signal[g]), "start": g0, "end": g1,
                     "iters": [int(v) for v in iters[row0:row0 + nrows]],
                     "objective": obj[row0:row0 + nrows].copy() if obj is not None else None})
        if omp and return_history:
            info[-1]["atoms"] = atoms[row0:row0 + nrows].copy()
    out = restack(res, kind)
    return (out, info) if return_history else out


def _takes_f_update(fn):
    """spain_inpaint's positional parameters are a fixed interface (they are
    the reference's param fields, in its order); S-SPAIN's two coefficient-update
    options are keyword-only on top of them and are taken here.  fn carries
    the parameter list and the documentation; the work is _spain_inpaint's."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def call(*args, f_update="H", omp_errdb=-40.0, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        return _spain_inpaint(**bound.arguments, f_update=f_update, omp_errdb=omp_errdb)
    return call


@_takes_f_update
def spain_inpaint(signal, mask=None, algorithm="aspain", w=4096, a=1024, wtype="hann", red=2,
                  s=1, r=1, epsilon=0.1, maxit=None, return_history=False, device="cuda"):
    """Fill every gap of `signal` by A-SPAIN or S-SPAIN on the GPU (the
    reference's spain_segmentation.m): windows of w samples every a samples
    over the signal, each with missing samples solved by the ADMM loop with the
    DFT frame of redundancy red, multiplied by the dual window and
    overlap-added.

    Input layouts, mask / NaN conventions and the return layout are
    janssen_inpaint's; only missing samples are written.  algorithm: "aspain"
    or "sspain" (any case).  wtype: "hann" only.  s, r: k starts at s and grows
    by s every r passes; epsilon: the objective that ends a window's loop;
    maxit None: ceil(floor(w red / 2 + 1) r / s).  return_history: also one
    dict per gap (signal, start, end, iters: passes per window with a row,
    objective [n_windows, maxit]: the objective of every pass, NaN after the
    last).

    Keyword-only, after these: f_update="H", omp_errdb=-40.0.  f_update:
    S-SPAIN's coefficient update, "H" (the hard threshold) or "OMP" (any
    case; needs algorithm "sspain"): orthogonal
    matching pursuit of at most k atoms down to a residual of omp_errdb dB of
    the block, at most 512 real unknowns (every w <= 512; k(maxit) <= 256
    above, which maxit None is clipped to); its history also has atoms
    [n_windows, maxit] int32, the atoms chosen in every pass, -1 after the last.
    """
