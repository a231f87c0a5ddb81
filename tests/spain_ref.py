"""Float64 NumPy reference of A-SPAIN and S-SPAIN (Mokry, Zaviska, Rajmic,
Vesely 2019; the reference project's references/spain: spain_segmentation.m
driving aspain.m / sspain.m with f_update = 'H'), written from the algorithm as
DESIGN §14 restates it, for the tests only.

It shares no structure with csrc/spain.hip: whole length-M transforms of the
zero-padded block, a stable descending sort for the threshold, the full
spectrum in memory.  The two transforms come in three formulations, chosen by
`transform`: "rfft" (numpy's real FFT, the default), "dense" (the product with
the M x w DFT matrix and with its adjoint) and "radix2" (a decimation-in-time
FFT of the whole complex length M written out below).  The tests compare two of
them to know what two correct float64 solvers differ by.

`stats`, where given, collects per evaluated iteration the relative margin
between the k-th and the (k+1)-th ranked magnitude (None where the threshold
keeps everything or both are exactly zero) and the objective.
"""
import functools

import numpy as np

import janssen_ref as R

# (w, a, s0, e0, n) on sinusoid_mix(n, noise=1e-3); the last has a gap longer
# than w, so all-missing windows
CASES = [(64, 16, 301, 321, 600),
         (128, 32, 531, 555, 1200),
         (256, 64, 900, 980, 2000),
         (64, 16, 100, 190, 400)]
# the largest supported transform: w 4096, red 2 -> M 8192; 600 samples of
# harmonic_signal(16000) missing, 40 passes
BIG = dict(w=4096, a=1024, s0=7000, e0=7600, n=16000, red=2, maxit=40)


def windows(w, a):
    """(gana, gsyn): the periodic Hann window (peak 1) and its painless dual
    for the shift a."""
    i = np.arange(w)
    g = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / w)
    den = np.zeros(w)
    for k in range(w // a):
        den += np.roll(g, k * a) ** 2
    return g, g / den


# ------------------------------------------------------------- the frame
def _fft_radix2(v, sign):
    """sum_n v[n] exp(sign 2 pi i n k / M), M a power of two, by iterative
    decimation in time (bit reversal first)."""
    M = len(v)
    lg = M.bit_length() - 1
    idx = np.arange(M)
    rev = np.zeros(M, dtype=np.int64)
    for b in range(lg):
        rev |= ((idx >> b) & 1) << (lg - 1 - b)
    out = np.asarray(v, np.complex128)[rev]
    half = 1
    while half < M:
        tw = np.exp(sign * 1j * np.pi * np.arange(half) / half)
        out = out.reshape(-1, 2 * half)
        lo, hi = out[:, :half], out[:, half:] * tw
        out = np.concatenate((lo + hi, lo - hi), axis=1)
        half *= 2
    return out.reshape(M)


@functools.lru_cache(maxsize=4)
def _dft_matrix(M, w):
    return np.exp(-2j * np.pi * np.outer(np.arange(M), np.arange(w)) / M) / np.sqrt(M)


def analysis(x, M, transform="rfft"):
    """A x = FFT_M([x; 0]) / sqrt(M), all M coefficients."""
    w = len(x)
    if transform == "dense":
        return _dft_matrix(M, w) @ x
    if transform == "radix2":
        return _fft_radix2(np.concatenate((x, np.zeros(M - w))), -1.0) / np.sqrt(M)
    h = np.fft.rfft(x, M) / np.sqrt(M)
    return np.concatenate((h, np.conj(h[-2:0:-1])))


def synthesis(z, w, transform="rfft"):
    """A* z = first w samples of IFFT_M(z) sqrt(M) (complex)."""
    M = len(z)
    if transform == "dense":
        return _dft_matrix(M, w).conj().T @ z
    if transform == "radix2":
        return _fft_radix2(z, 1.0)[:w] / np.sqrt(M)
    return np.fft.ifft(z)[:w] * np.sqrt(M)


TIES_TO_THE_LOWER_INDEX = True     # MATLAB's stable descending sort; the tests flip it once


def hard_threshold(z, k, stats=None):
    """Keep the k largest of the M/2 + 1 half-spectrum coefficients, DC ranked
    by half its magnitude (Nyquist by all of it), ties to the lower index, and
    mirror the conjugates."""
    M = len(z)
    nh = M // 2 + 1
    half = np.array(z[:nh])
    if k >= nh:
        if stats is not None:
            stats.append(None)
        kept = half
    else:
        rank = np.abs(half)
        rank[0] *= 0.5
        order = np.argsort(-rank, kind="stable")
        if not TIES_TO_THE_LOWER_INDEX:
            order = nh - 1 - np.argsort(-rank[::-1], kind="stable")
        if stats is not None:
            hi, lo = rank[order[k - 1]], rank[order[k]]
            stats.append(None if hi == 0.0 and lo == 0.0 else (hi - lo) / hi)
        kept = np.zeros(nh, complex)
        kept[order[:k]] = half[order[:k]]
    return np.concatenate((kept, np.conj(kept[-2:0:-1])))


def _schedule(cnt, k, s, r):
    cnt += 1
    if cnt % r == 0:
        k += s
    return cnt, k


def aspain(row, observed, red=2, s=1, r=1, epsilon=0.1, maxit=None, transform="rfft",
           stats=None):
    """-> (recorded iterate, objectives of the evaluated iterations)."""
    w = len(row)
    M = red * w
    maxit = default_maxit(w, red, s, r) if maxit is None else maxit
    x = np.array(row, np.float64)
    z = analysis(x, M, transform)
    u = np.zeros(M, complex)
    k, cnt, best, rec, objs = s, 1, np.inf, x.copy(), []
    margins = None if stats is None else []
    while cnt <= maxit:
        zb = hard_threshold(z + u, k, margins)
        obj = float(np.linalg.norm(z - zb))
        objs.append(obj)
        if obj <= best:
            rec, best = x.copy(), obj
        if obj <= epsilon:
            break
        syn = np.real(synthesis(zb - u, w, transform))
        x = np.where(observed, row, syn)
        z = analysis(x, M, transform)
        u = u + z - zb
        cnt, k = _schedule(cnt, k, s, r)
    if stats is not None:
        stats.append((margins, objs))
    return rec, objs


def sspain(row, observed, red=2, s=1, r=1, epsilon=0.1, maxit=None, transform="rfft",
           stats=None):
    w = len(row)
    M = red * w
    maxit = default_maxit(w, red, s, r) if maxit is None else maxit
    x = np.array(row, np.float64)
    u = np.zeros(w)
    k, cnt, best, rec, objs = s, 1, np.inf, x.copy(), []
    margins = None if stats is None else []
    while cnt <= maxit:
        zb = hard_threshold(analysis(x - u, M, transform), k, margins)
        syn = synthesis(zb, w, transform)
        obj = float(np.linalg.norm(syn - x))
        objs.append(obj)
        if obj <= best:
            rec, best = x.copy(), obj
        if obj <= epsilon:
            break
        xe = np.real(syn)
        x = np.where(observed, row, xe + u)
        u = u + xe - x
        cnt, k = _schedule(cnt, k, s, r)
    if stats is not None:
        stats.append((margins, objs))
    return rec, objs


def default_maxit(w, red=2, s=1, r=1):
    return min(-(-((w * red // 2 + 1) * r) // s), w * red // 2 + 1)


def spain_segmentation(x, observed, algorithm="aspain", w=4096, a=1024, red=2, s=1, r=1,
                       epsilon=0.1, maxit=None, transform="rfft", stats=None):
    """-> (restored signal, iterations per solved window, objectives
    [solved windows][maxit] NaN-padded, the solved windows' indices)."""
    solver = {"aspain": aspain, "sspain": sspain}[algorithm]
    maxit = default_maxit(w, red, s, r) if maxit is None else maxit
    x = np.asarray(x, np.float64)
    observed = np.asarray(observed, bool)
    Ls = len(x)
    L = -(-Ls // a) * a + (-(-w // a) - 1) * a
    data = np.concatenate((np.where(observed, x, 0.0), np.zeros(L - Ls)))
    obs = np.concatenate((observed, np.ones(L - Ls, bool)))
    gana, gsyn = windows(w, a)
    out = np.zeros(L)
    iters, objs, solved = [], [], []
    for n in range(L // a):
        idx = (n * a - w // 2 + np.arange(w)) % L
        if obs[idx].all():
            continue
        if not obs[idx].any():
            continue                   # a block of zeros: SPAIN returns it at once
        rec, o = solver(data[idx] * gana, obs[idx], red, s, r, epsilon, maxit, transform, stats)
        out[idx] += rec * gsyn
        iters.append(len(o))
        objs.append(o + [np.nan] * (maxit - len(o)))
        solved.append(n)
    out[obs] = data[obs]
    return out[:Ls], iters, np.array(objs).reshape(len(objs), maxit), solved


# ------------------------------------------------------------- the cases
def case_signal(case):
    return R.sinusoid_mix(case[4], noise=1e-3)


def case_mask(case):
    m = np.ones(case[4], bool)
    m[case[2]:case[3]] = False
    return m


@functools.lru_cache(maxsize=None)
def case_reference(case, algorithm, epsilon=0.1, red=2, s=1, r=1, transform="rfft",
                   float32=False):
    """-> dict(out, iters, obj, windows, stats) of spain_segmentation on the
    case; float32: the signal rounded to float32 first.  Cached: do not modify."""
    w, a = case[0], case[1]
    x = case_signal(case)
    if float32:
        x = x.astype(np.float32).astype(np.float64)
    stats = []
    out, iters, obj, solved = spain_segmentation(x, case_mask(case), algorithm, w, a, red, s, r,
                                                 epsilon, None, transform, stats)
    return dict(out=out, iters=iters, obj=obj, windows=solved, stats=stats)


def big_signal():
    x = R.harmonic_signal(BIG["n"])
    m = np.ones(BIG["n"], bool)
    m[BIG["s0"]:BIG["e0"]] = False
    return x, m


@functools.lru_cache(maxsize=None)
def big_reference(algorithm, transform="rfft", float32=False):
    x, m = big_signal()
    if float32:
        x = x.astype(np.float32).astype(np.float64)
    stats = []
    out, iters, obj, solved = spain_segmentation(x, m, algorithm, BIG["w"], BIG["a"], BIG["red"],
                                                 1, 1, 0.1, BIG["maxit"], transform, stats)
    return dict(out=out, iters=iters, obj=obj, windows=solved, stats=stats)


def conditions(stats, epsilon):
    """(smallest relative margin, smallest |obj - epsilon| / epsilon) over every
    evaluated iteration of every window in `stats`."""
    margin, dist = np.inf, np.inf
    for margins, objs in stats:
        for m in margins:
            if m is not None:
                margin = min(margin, m)
        for o in objs:
            dist = min(dist, abs(o - epsilon) / epsilon)
    return margin, dist


# the 200-sample gap of the "no rows" test: the windows of its interior hold no
# observed sample
LONG_GAP = (64, 16, 250, 450, 700)

_CLIPS = {}


def clip_reference(audio, s0, e0, w, a, algorithm="aspain"):
    """-> (spain_segmentation of `audio` with [s0, e0) missing and the default
    solver parameters, what the "radix2" formulation differs from it by on the
    gap relative to max|clean gap|).  Cached: do not modify."""
    key = (len(audio), float(np.sum(audio)), s0, e0, w, a, algorithm)
    if key not in _CLIPS:
        m = np.ones(len(audio), bool)
        m[s0:e0] = False
        one = spain_segmentation(audio, m, algorithm, w, a)[0]
        two = spain_segmentation(audio, m, algorithm, w, a, transform="radix2")[0]
        _CLIPS[key] = (one, float(np.max(np.abs(one[s0:e0] - two[s0:e0]))
                                  / np.max(np.abs(audio[s0:e0]))))
    return _CLIPS[key]


ALGS = ("aspain", "sspain")
# the GPU parity runs: every case at epsilon 0.1; 1e-3 only at w <= 128 (at w 256
# the two CPU formulations come within a factor 10 of the bound there)
PARITY = [(c, g, 0.1) for c in CASES for g in ALGS] + \
         [(c, g, 1e-3) for c in CASES if c[0] <= 128 for g in ALGS]
# other frame lengths and another schedule, at epsilon 0.1
OTHER = [(CASES[0], dict(red=1)), (CASES[0], dict(red=4)), (CASES[1], dict(s=2, r=3))]


def tie_row(w=64):
    """A row whose first threshold is an exact tie: a unit impulse at sample 0
    has a flat spectrum, so H_1 chooses among equal magnitudes (every bin but
    DC, which ranks by half).  -> (row, observed, run start, run length)."""
    row = np.zeros(w)
    row[0] = 1.0
    obs = np.ones(w, bool)
    obs[20:30] = False
    return row, obs, 20, 10
