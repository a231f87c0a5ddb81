"""Float64 numpy statement of the gap-constrained Griffin-Lim (DESIGN §16,
include/ainp.h: ainp_gap_phase), with np.fft, and the fixtures the CPU and GPU
tests share.

Frames are librosa's (center, zero padding, T = 1 + S // hop), the window
periodic Hann of `win` samples centred in n_fft.  Frame t is unreliable when
one of the `win` samples under its window is missing; padding is reliable.  A
maximal set of consecutive unreliable frames is a run, solved on its own:

    y0 = x (missing samples: the value passed, NaN read as 0)
    for k < n_iter, over the frames U of the run:
        C = STFT_U(y);  resid[k] = sqrt(sum c_f (|C| - A)^2), c_f = 1 (DC, Nyquist) or 2
        a = C - alpha / (1 + alpha) tprev   (not at k = 0);  tprev = C
        ang = a / (|a| + tiny);  f_t = irfft(A ang) w
        y[n] = sum_t f_t[n - t hop] / sum_t w^2[n - t hop]   on the run's missing samples
"""
import functools

import numpy as np
import scipy.signal

TINY = np.finfo(np.float64).tiny


def window(n_fft, win):
    w = np.zeros(n_fft)
    lpad = (n_fft - win) // 2
    w[lpad:lpad + win] = scipy.signal.get_window("hann", win, fftbins=True)
    return w


def unreliable_frames(mask, n_fft, hop, win):
    """bool [T] by the definition, sample by sample."""
    m = np.asarray(mask, bool)
    S = m.size
    T = 1 + S // hop
    bad = np.zeros(T, bool)
    for t in range(T):
        a = t * hop - n_fft // 2 + (n_fft - win) // 2
        lo, hi = max(a, 0), min(a + win, S)
        bad[t] = hi > lo and not m[lo:hi].all()
    return bad


def runs(mask, n_fft, hop, win):
    """[(first frame, frame count)] of the maximal runs of unreliable frames."""
    bad = unreliable_frames(mask, n_fft, hop, win)
    out, first = [], None
    for t, b in enumerate(list(bad) + [False]):
        if b and first is None:
            first = t
        if not b and first is not None:
            out.append((first, t - first))
            first = None
    return out


def stft_mag(x, n_fft, hop, win):
    """|STFT| [F, T] of x in float64 (center, zero padding)."""
    x = np.asarray(x, np.float64)
    T = 1 + x.size // hop
    xp = np.concatenate((np.zeros(n_fft // 2), x, np.zeros(n_fft)))
    fr = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)]) * window(n_fft, win)
    return np.abs(np.fft.rfft(fr, axis=1)).T


def gap_phase(x, mask, A, n_fft, hop, win, n_iter, alpha, cond=None):
    """Returns (y, resid [runs, n_iter]).  cond: a list that receives, per run
    and iteration, (smallest nonzero |a|, largest |a|)."""
    x = np.asarray(x, np.float64)
    m = np.asarray(mask, bool)
    A = np.asarray(A, np.float64)
    S = x.size
    w = window(n_fft, win)
    y = x.copy()
    y[~m & np.isnan(y)] = 0.0
    cf = np.full(n_fft // 2 + 1, 2.0)
    cf[0] = cf[-1] = 1.0
    c = alpha / (1.0 + alpha)
    resid = []
    for t0, R in runs(m, n_fft, hop, win):
        s0, L = t0 * hop - n_fft // 2, (R - 1) * hop + n_fft
        idx = np.arange(s0, s0 + L)
        inside = (idx >= 0) & (idx < S)
        seg = np.zeros(L)
        seg[inside] = y[idx[inside]]
        miss = np.zeros(L, bool)
        miss[inside] = ~m[idx[inside]]
        den = np.zeros(L)
        for t in range(R):
            den[t * hop:t * hop + n_fft] += w * w
        own = miss & (den > 0)
        At = A[:, t0:t0 + R].T
        tprev, rr = None, []
        for k in range(n_iter):
            fr = np.stack([seg[t * hop:t * hop + n_fft] for t in range(R)]) * w
            C = np.fft.rfft(fr, axis=1)
            rr.append(np.sqrt(np.sum(cf * (np.abs(C) - At) ** 2)))
            a = C if k == 0 else C - c * tprev
            tprev = C
            mag = np.abs(a)
            if cond is not None:
                nz = mag[mag > 0]
                cond.append((nz.min() if nz.size else np.inf, mag.max()))
            f = np.fft.irfft(At * (a / (mag + TINY)), n=n_fft, axis=1) * w
            num = np.zeros(L)
            for t in range(R):
                num[t * hop:t * hop + n_fft] += f[t]
            seg[own] = num[own] / den[own]
        y[idx[own]] = seg[own]
        resid.append(rr)
    return y, np.asarray(resid, np.float64).reshape(len(resid), n_iter)


# ------------------------------------------------------------------ fixtures
class Fixture:
    def __init__(self, name, S, n_fft, hop, win, gaps, kind, seed):
        self.name, self.S, self.n_fft, self.hop, self.win = name, S, n_fft, hop, win
        self.gaps, self.kind, self.seed = gaps, kind, seed

    def __repr__(self):
        return self.name

    @functools.cached_property
    def clean(self):
        rng = np.random.default_rng(self.seed)
        if self.kind == "noise":
            return rng.standard_normal(self.S)
        n = np.arange(self.S)      # tones plus 0.01 noise, never pure tones
        f = rng.uniform(0.01, 0.45, 3)
        ph = rng.uniform(0, 2 * np.pi, 3)
        return sum(np.sin(2 * np.pi * fk * n + pk) for fk, pk in zip(f, ph)) / 3 \
            + 0.01 * rng.standard_normal(self.S)

    @functools.cached_property
    def mask(self):
        m = np.ones(self.S, bool)
        for s, e in self.gaps:
            m[s:e] = False
        return m

    @functools.cached_property
    def observed(self):
        return np.where(self.mask, self.clean, 0.0)

    @functools.cached_property
    def mag(self):
        """|STFT(clean)| as float32, the target both sides take."""
        return np.ascontiguousarray(
            stft_mag(self.clean, self.n_fft, self.hop, self.win).astype(np.float32))


SMALL_GAPS = [
    ("short", [(500, 520)]),                 # shorter than the window
    ("long", [(400, 500)]),                  # longer than n_fft: all-zero frames
    ("one", [(300, 301)]),
    ("head", [(0, 30)]),                     # at sample 0
    ("tail", [(1000, 1024)]),                # ending at S
    ("near", [(400, 410), (430, 440)]),      # closer than a window: one run
    ("far", [(200, 210), (700, 710)]),       # two runs
]
FIXTURES = [Fixture(f"{name}-w{win}", 1024, 64, 16, win, gaps, kind, 100 + 10 * i + (win == 64))
            for win in (48, 64)
            for i, (name, gaps) in enumerate(SMALL_GAPS)
            for kind in (("noise",) if i % 2 == 0 else ("tones",))]
FIXTURES += [
    Fixture("n512-h192-w384", 8000, 512, 192, 384, [(3000, 4280)], "tones", 7),
    Fixture("n512-h128-w512", 8000, 512, 128, 512, [(3000, 4280)], "noise", 8),
    Fixture("n2048-h512", 8000, 2048, 512, 2048, [(3000, 4280)], "tones", 9),   # workspace
]
BY_NAME = {f.name: f for f in FIXTURES}
PARITY_ITERS = (1, 2, 4, 8)
PARITY_ALPHAS = (0.0, 0.99)


@functools.lru_cache(maxsize=None)
def reference(name, n_iter, alpha):
    """(y, resid) of a fixture from its zero-filled observed signal; computed
    once, shared, never modified."""
    f = BY_NAME[name]
    y, r = gap_phase(f.observed, f.mask, f.mag, f.n_fft, f.hop, f.win, n_iter, alpha)
    y.setflags(write=False)
    r.setflags(write=False)
    return y, r


@functools.lru_cache(maxsize=None)
def sensitivity(name):
    """E of a fixture: the largest change of the output through 8 iterations
    (over the iteration counts and momenta of the parity test) when the
    RELIABLE samples are perturbed by 1e-13 randn -- never the start values in
    the gap, so a frame wholly inside the gap still starts as exact zeros."""
    f = BY_NAME[name]
    rng = np.random.default_rng(f.seed + 1000)
    xp = f.observed + np.where(f.mask, 1e-13 * rng.standard_normal(f.S), 0.0)
    E = 0.0
    for alpha in PARITY_ALPHAS:
        for n in PARITY_ITERS:
            yp, _ = gap_phase(xp, f.mask, f.mag, f.n_fft, f.hop, f.win, n, alpha)
            E = max(E, float(np.max(np.abs(yp - reference(name, n, alpha)[0]))))
    return E
