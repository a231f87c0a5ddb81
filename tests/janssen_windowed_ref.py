"""Independent float64 restatement of the window-wise Janssen algorithm (the
reference project's models/AudioReg/utils/segmentation_inp.m on the support
that train.m:146-172 cuts with offset.m and min_sig_supp_2.m), for the tests
only.  numpy (and scipy for the second solver) alone.

It shares no structure with ainp.janssen.plan_windows or
csrc/janssen_windows.hip: NaN marks the missing samples, the loop is dense over
every window of the whole padded support (observed samples included, as the
reference overlap-adds them), each window with missing samples goes through
janssen_ref.janssen / ar_ref.janssen, and the support comes from the 1-based
formulas in floating point.

LTFAT is replaced by closed forms: fftshift(normalize(gabwin('hann', a, w, L),
'peak')) is the periodic Hann window, and gabdual(gana, a, w) * w for a window
as long as the number of channels is the painless dual, gana over the sum of
its squared shifts by a.  The constant factor is immaterial: the final
`restored ./ rescale` cancels it.
"""
import math

import numpy as np

import ar_ref
import janssen_ref


def support(s0, e0, w, a):
    """0-based [lo, hi) of the signal that train.m hands to segmentation_inp
    for the missing range [s0, e0)."""
    s, f = s0 + 1, e0                               # MATLAB's first and last missing index
    c = math.ceil((s + f) / 2)                      # offset(s, f, a, 'half')
    d = 1 + math.floor((c - 1) / a) * a + math.ceil(a / 2)
    off = (c - d) % a
    S = math.ceil((s - math.ceil(w / 2)) / a) + 1   # min_sig_supp_2
    mid = 1 + (S - 1) * a + off
    if mid - a + math.ceil(w / 2) - 1 >= s:
        mid = mid - a
    q = mid - math.ceil(math.floor(w / 2) / a) * a
    steps = math.floor((f + math.floor(w / 2) - mid) / a)
    Q = mid + steps * a + math.ceil(math.ceil(w / 2) / a) * a
    jans, jane = q, Q - 1                           # 1-based, inclusive
    return jans - 1, jane


def tukeywin(w, r=0.5):
    """MATLAB tukeywin(w, r), by its index form."""
    t = np.linspace(0.0, 1.0, w)
    per = r / 2
    tl = int(math.floor(per * (w - 1))) + 1
    th = w - tl + 1
    return np.concatenate(((1 + np.cos(np.pi / per * (t[:tl] - per))) / 2,
                           np.ones(th - tl - 1),
                           (1 + np.cos(np.pi / per * (t[th - 1:] - 1 + per))) / 2))


def windows(wtype, w, a):
    """(gana, gsyn) of segmentation_inp.m."""
    hann = np.array([0.5 - 0.5 * math.cos(2 * math.pi * i / w) for i in range(w)])
    kind = wtype.lower()
    if kind == "rect":
        return np.ones(w), hann
    if kind == "tukey":
        g = tukeywin(w)
        return g, g
    assert kind == "hann"
    den = sum(np.roll(hann, k * a) ** 2 for k in range(w // a))
    return hann, hann / den


def janssen_toeplitz(x, gap_start, gap_len, p, maxit, method="lpc"):
    """A second float64 formulation of janssen_ref.janssen for measuring what
    two correct solvers differ by: autocorrelation by direct sums, both
    symmetric Toeplitz systems through scipy.linalg.solve_toeplitz.  "lpc" only."""
    from scipy.linalg import solve_toeplitz
    assert method == "lpc"
    x = np.array(x, np.float64)
    n, h = len(x), gap_len
    sol = x.copy()
    sol[gap_start:gap_start + h] = 0.0
    history = []
    for _ in range(maxit):
        if not np.any(sol):
            break
        r = np.array([np.dot(sol[:n - k], sol[k:]) for k in range(p + 1)]) / n
        a = np.concatenate(([1.0], solve_toeplitz(r[:p], -r[1:])))
        b = np.zeros(max(p + 1, h))
        b[:p + 1] = [np.dot(a[:p + 1 - k], a[k:]) for k in range(p + 1)]
        rhs = np.zeros(h)
        for i in range(h):
            t = gap_start + i
            for j in range(max(0, t - p), min(n, t + p + 1)):
                if not gap_start <= j < gap_start + h:
                    rhs[i] -= b[abs(t - j)] * x[j]
        sol[gap_start:gap_start + h] = solve_toeplitz(b[:h], rhs)
        history.append(sol[gap_start:gap_start + h].copy())
    return sol, np.array(history).reshape(len(history), h), len(history)


def _solve(method, solver):
    if solver == "toeplitz":
        return lambda x, s, h, p, maxit: janssen_toeplitz(x, s, h, p, maxit, method)
    if method.lower() == "arburg":
        return lambda x, s, h, p, maxit: ar_ref.janssen(x, s, h, p, maxit, "arburg")
    return janssen_ref.janssen


def segmentation_inp(signal, p, maxit, w, a, wtype, method="lpc", solver="dense"):
    """segmentation_inp.m with saveall: signal float64 [n] with NaN on the
    missing samples -> restored [n, maxit].  A window that stops early keeps
    its last iterate for the columns it did not reach (MATLAB has NaN there;
    none of the tests' windows stops)."""
    solve = _solve(method, solver)
    n = len(signal)
    L = math.ceil(n / a) * a + (math.ceil(w / a) - 1) * a
    S = L // a
    data = np.concatenate((signal, np.zeros(L - n)))
    gana, gsyn = windows(wtype, w, a)
    rescale = np.zeros(L)
    restored = np.zeros((L, maxit))
    for s in range(S):
        idx = np.mod(s * a - w // 2 + np.arange(w), L)
        seg = data[idx] * gana
        nan = np.isnan(seg)
        if nan.all():
            out = np.zeros((w, maxit))
        elif not nan.any():
            out = np.repeat(seg[:, None], maxit, axis=1)
        else:
            where = np.flatnonzero(nan)
            start, length = int(where[0]), len(where)
            assert where[-1] - start + 1 == length, "one run of missing samples per window"
            clean = np.where(nan, 0.0, seg)
            _, hist, done = solve(clean, start, length, p, maxit)
            out = np.repeat(clean[:, None], maxit, axis=1)
            for k in range(maxit):
                if done:
                    out[start:start + length, k] = hist[min(k, done - 1)]
        rescale[idx] += gana * gsyn
        restored[idx] += out * gsyn[:, None]
    return (restored / rescale[:, None])[:n]


def inpaint_gap(x, s0, e0, p, maxit, w, a, wtype, method="lpc", solver="dense"):
    """The gap [s0, e0) of x as train.m:146-172 fills it -> (restored support
    [hi - lo, maxit], lo).  Samples of the support outside x are observed
    zeros (train.m would index out of range)."""
    lo, hi = support(s0, e0, w, a)
    sup = np.zeros(hi - lo)
    a0, a1 = max(lo, 0), min(hi, len(x))
    sup[a0 - lo:a1 - lo] = x[a0:a1]
    sup[s0 - lo:e0 - lo] = np.nan
    return segmentation_inp(sup, p, maxit, w, a, wtype, method, solver), lo


# The parity cases of the window-wise tests: (w, a, gap start, gap end, p,
# maxit, signal length).  What the less obvious ones exercise: [1000, 1300)
# windows that are almost all gap; [301, 302) a single missing sample;
# [350, 440) windows with every sample missing; (128, 64) w / a = 2; [30, 110)
# a support that starts at -218; [1000, 1080) in 1100 samples a support that
# runs 228 samples past the end; (45, 15) an odd window length.
CASES = [(256, 64, 900, 980, 32, 5, 2000),
         (128, 32, 531, 555, 16, 5, 1200),
         (256, 64, 1000, 1300, 32, 3, 2400),
         (64, 16, 301, 302, 8, 3, 600),
         (64, 16, 350, 440, 8, 3, 800),
         (128, 64, 400, 440, 16, 4, 900),
         (256, 64, 30, 110, 32, 5, 1100),
         (256, 64, 1000, 1080, 32, 5, 1100),
         (45, 15, 200, 210, 8, 3, 500)]
WTYPES = ("hann", "rect", "tukey")
_cache = {}


def case_signal(case):
    return janssen_ref.sinusoid_mix(case[6], noise=1e-3)


def case_reference(case, wtype, method="lpc", solver="dense", dtype=np.float64):
    """The gap of a parity case after every iteration, [maxit, h]; computed
    once per (case, shape, method, solver, input precision) and shared."""
    key = (case, wtype, method, solver, np.dtype(dtype).name)
    if key not in _cache:
        w, a, s0, e0, p, maxit, _ = case
        x = case_signal(case).astype(dtype).astype(np.float64)
        res, lo = inpaint_gap(x, s0, e0, p, maxit, w, a, wtype, method, solver)
        out = res[s0 - lo:e0 - lo].T.copy()
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]
