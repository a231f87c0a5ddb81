"""Float64 NumPy reference of S-SPAIN with the OMP coefficient update
(references/spain/sspain.m with f_update = 'OMP'), written from the algorithm
as DESIGN §14.3 restates it, for the tests only.  Frame, loop, schedule and
segmentation are tests/spain_ref.py's.

It shares no structure with csrc/spain_omp.hip: the real columns 2 Re d_m and
-2 Im d_m (d_m itself at DC and Nyquist) are built in the time domain, only for
the chosen atoms; the least squares is numpy.linalg.lstsq on them; the
selection is a stable descending sort of the whole half spectrum; the residual
is taken in the time domain.  `solver` chooses a second formulation, "normal":
the normal equations of the same columns by numpy.linalg.solve.  The tests
compare the two to know what two correct float64 solvers differ by.

`stats`, where given, collects per OMP call a dict of lists over its inner
steps: "margin" (the relative margin between the best and the second-best
unselected |c_m|; None where both are zero), "resid" (|‖r‖ / tol − 1| of every
residual test, tol > 0), "pivot" (the relative squared pivot of every new real
column), "cond" (the condition number of the chosen columns after every
append), and "stop", the rule that ended the call.
"""
import functools

import numpy as np

import spain_ref as S

PIVOT = 1e-10
OMP_DIMS = 512


def omp_k(cnt, s=1, r=1):
    return s * (1 + cnt // r - 1 // r)


def atom_columns(m, w, M):
    """The real columns atom m brings, [w, 1] at DC and Nyquist, else [w, 2]."""
    ph = 2.0 * np.pi * ((m * np.arange(w)) % M) / M
    if m in (0, M // 2):
        return (np.cos(ph) / np.sqrt(M))[:, None]
    return np.stack((2.0 * np.cos(ph), -2.0 * np.sin(ph)), axis=1) / np.sqrt(M)


def _solve(C, v, solver):
    if solver == "normal":
        return np.linalg.solve(C.T @ C, C.T @ v)
    return np.linalg.lstsq(C, v, rcond=None)[0]


def omp(v, M, k, errdb=-40.0, solver="lstsq", stats=None):
    """OMP_k(v) -> (z-bar: all M coefficients, the chosen bins in order)."""
    v = np.asarray(v, np.float64)
    w = len(v)
    nh = M // 2 + 1
    tol = 10.0 ** (errdb / 20.0) * np.linalg.norm(v)
    r = v.copy()
    S_, C, coef = [], np.zeros((w, 0)), np.zeros(0)
    Q = np.zeros((w, 0))     # an orthonormal basis of the chosen columns, for the pivots
    st = dict(margin=[], resid=[], pivot=[], cond=[], stop=None)
    while True:
        nr = np.linalg.norm(r)
        if tol > 0.0:
            st["resid"].append(abs(nr / tol - 1.0))
        if nr <= tol:
            st["stop"] = "residual"
            break
        if len(S_) == k:
            st["stop"] = "count"
            break
        mag = np.abs(np.fft.rfft(r, M)) / np.sqrt(M)
        free = np.ones(nh, bool)
        free[S_] = False
        cand = np.flatnonzero(free)
        if len(cand) == 0:
            st["stop"] = "exhausted"
            break
        order = cand[np.argsort(-mag[cand], kind="stable")]
        m = int(order[0])
        if len(order) > 1:
            hi, lo = mag[order[0]], mag[order[1]]
            st["margin"].append(None if hi == 0.0 and lo == 0.0 else (hi - lo) / hi)
        new = atom_columns(m, w, M)
        if C.shape[1] + new.shape[1] > w:
            st["stop"] = "dimension"
            break
        ok, Qn = True, Q
        for j in range(new.shape[1]):
            c = new[:, j]
            perp = c - Qn @ (Qn.T @ c)
            perp = perp - Qn @ (Qn.T @ perp)      # Gram-Schmidt, twice
            rel = float(perp @ perp) / float(c @ c)
            st["pivot"].append(rel)
            if rel < PIVOT:
                ok = False
                break
            Qn = np.concatenate((Qn, perp[:, None] / np.linalg.norm(perp)), axis=1)
        if not ok:
            st["stop"] = "pivot"
            break
        Q, C = Qn, np.concatenate((C, new), axis=1)
        S_.append(m)
        coef = _solve(C, v, solver)
        r = v - C @ coef
        if stats is not None:
            st["cond"].append(float(np.linalg.cond(C)))
    half = np.zeros(nh, complex)
    at = 0
    for m in S_:
        if m in (0, M // 2):
            half[m] = coef[at]
            at += 1
        else:
            half[m] = coef[at] + 1j * coef[at + 1]
            at += 2
    if stats is not None:
        stats.append(st)
    return np.concatenate((half, np.conj(half[-2:0:-1]))), S_


def sspain_omp(row, observed, red=2, s=1, r=1, epsilon=0.1, maxit=None, errdb=-40.0,
               solver="lstsq", stats=None):
    """-> (recorded iterate, objectives, atoms of the evaluated passes)."""
    w = len(row)
    M = red * w
    maxit = S.default_maxit(w, red, s, r) if maxit is None else maxit
    x = np.array(row, np.float64)
    u = np.zeros(w)
    k, cnt, best, rec, objs, atoms = s, 1, np.inf, x.copy(), [], []
    calls = None if stats is None else []
    while cnt <= maxit:
        zb, chosen = omp(x - u, M, k, errdb, solver, calls)
        syn = S.synthesis(zb, w)
        obj = float(np.linalg.norm(syn - x))
        objs.append(obj)
        atoms.append(len(chosen))
        if obj <= best:
            rec, best = x.copy(), obj
        if obj <= epsilon:
            break
        xe = np.real(syn)
        x = np.where(observed, row, xe + u)
        u = u + xe - x
        cnt += 1
        if cnt % r == 0:
            k += s
    if stats is not None:
        stats.append((calls, objs))
    return rec, objs, atoms


def segmentation(x, observed, w, a, red=2, s=1, r=1, epsilon=0.1, maxit=None, errdb=-40.0,
                 solver="lstsq", stats=None):
    """spain_ref.spain_segmentation with sspain_omp on every window -> (restored
    signal, passes per solved window, objectives and atoms [solved windows][maxit]
    padded with NaN and -1, the solved windows' indices)."""
    maxit = S.default_maxit(w, red, s, r) if maxit is None else maxit
    x = np.asarray(x, np.float64)
    observed = np.asarray(observed, bool)
    Ls = len(x)
    L = -(-Ls // a) * a + (-(-w // a) - 1) * a
    data = np.concatenate((np.where(observed, x, 0.0), np.zeros(L - Ls)))
    obs = np.concatenate((observed, np.ones(L - Ls, bool)))
    gana, gsyn = S.windows(w, a)
    out = np.zeros(L)
    iters, objs, atoms, solved = [], [], [], []
    for n in range(L // a):
        idx = (n * a - w // 2 + np.arange(w)) % L
        if obs[idx].all() or not obs[idx].any():
            continue
        rec, o, na = sspain_omp(data[idx] * gana, obs[idx], red, s, r, epsilon, maxit, errdb,
                                solver, stats)
        out[idx] += rec * gsyn
        iters.append(len(o))
        objs.append(o + [np.nan] * (maxit - len(o)))
        atoms.append(na + [-1] * (maxit - len(na)))
        solved.append(n)
    out[obs] = data[obs]
    return (out[:Ls], iters, np.array(objs).reshape(len(objs), maxit),
            np.array(atoms, np.int32).reshape(len(atoms), maxit), solved)


# ------------------------------------------------------------- the cases
# (case, epsilon, errdb, solver parameters): every GPU parity run
PARITY = [(c, 0.1, -40.0, {}) for c in S.CASES] + \
         [(S.CASES[1], 1e-3, -120.0, {}), (S.CASES[0], 1e-3, -120.0, {}),
          (S.CASES[0], 0.1, -40.0, dict(red=1)), (S.CASES[0], 0.1, -40.0, dict(red=4)),
          (S.CASES[1], 0.1, -40.0, dict(s=2, r=3))]
PARITY_IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{e}-{d:g}" + "".join(f"-{k}{v}" for k, v in kw.items())
              for c, e, d, kw in PARITY]
# the largest transform, spain_ref.BIG's signal and gap: 12 passes
BIG_MAXIT = 12


@functools.lru_cache(maxsize=None)
def _case_reference(case, epsilon, errdb, kw, solver, float32):
    x = S.case_signal(case)
    if float32:
        x = x.astype(np.float32).astype(np.float64)
    stats = []
    out, iters, obj, atoms, solved = segmentation(x, S.case_mask(case), case[0], case[1],
                                                  epsilon=epsilon, errdb=errdb, solver=solver,
                                                  stats=stats, **dict(kw))
    return dict(out=out, iters=iters, obj=obj, atoms=atoms, windows=solved, stats=stats)


def case_reference(case, epsilon=0.1, errdb=-40.0, kw=None, solver="lstsq", float32=False):
    """-> dict(out, iters, obj, atoms, windows, stats) of segmentation on the
    case; float32: the signal rounded to float32 first.  Cached: do not modify."""
    return _case_reference(case, epsilon, errdb, tuple(sorted((kw or {}).items())), solver,
                           float32)


@functools.lru_cache(maxsize=None)
def big_reference():
    x, m = S.big_signal()
    B = S.BIG
    stats = []
    out, iters, obj, atoms, solved = segmentation(x, m, B["w"], B["a"], B["red"], maxit=BIG_MAXIT,
                                                  stats=stats)
    return dict(out=out, iters=iters, obj=obj, atoms=atoms, windows=solved, stats=stats)


# one window of w = 512 with 130 atoms a pass: 260 real unknowns, more than the
# 256 lanes of the kernel that runs it
WIDE = dict(w=512, red=2, s=130, r=3, maxit=2, epsilon=1e-3, errdb=-120.0)


def wide_row():
    """-> (the windowed row with its run zeroed, observed, run start, run length)."""
    import janssen_ref as R
    w = WIDE["w"]
    row = R.sinusoid_mix(2000, noise=1e-3)[700:700 + w] * S.windows(w, 128)[0]
    obs = np.ones(w, bool)
    obs[240:300] = False
    return np.where(obs, row, 0.0), obs, 240, 60


@functools.lru_cache(maxsize=None)
def wide_reference(solver="lstsq"):
    """-> dict(rec, obj, atoms, stats) of sspain_omp on wide_row().  Cached: do
    not modify."""
    row, obs, g0, h = wide_row()
    kw = {k: v for k, v in WIDE.items() if k != "w"}
    stats = []
    rec, objs, atoms = sspain_omp(row, obs, solver=solver, stats=stats, **kw)
    return dict(rec=rec, obj=objs, atoms=atoms, stats=stats)


def conditions(stats, epsilon):
    """Over every OMP call of every pass of every window in `stats` -> dict of
    the smallest selection margin, residual-stop distance, relative squared
    pivot and |obj - epsilon| / epsilon, the largest condition number and the
    set of stop rules met."""
    out = dict(margin=np.inf, resid=np.inf, pivot=np.inf, eps=np.inf, cond=0.0, stops=set())
    for calls, objs in stats:
        for st in calls:
            out["margin"] = min([out["margin"]] + [m for m in st["margin"] if m is not None])
            out["resid"] = min([out["resid"]] + st["resid"])
            out["pivot"] = min([out["pivot"]] + st["pivot"])
            out["cond"] = max([out["cond"]] + st["cond"])
            out["stops"].add(st["stop"])
        for o in objs:
            out["eps"] = min(out["eps"], abs(o - epsilon) / epsilon)
    return out
