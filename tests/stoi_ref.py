"""Float64 numpy statement of STOI and ESTOI as DESIGN §17 defines them
(include/ainp.h: ainp_stoi), with np.fft, and the fixtures the CPU and GPU
tests share.  Written from the definition, not from the kernel.

    frames of 256 every 128 under w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257))
    e[k] = 20 log10(|w x_k| + EPS) of the CLEAN signal; keep k iff e[k] > max(e) - 40
    s = overlap-add of the kept windowed frames, 128 apart (clean and restored alike)
    X[j, t] = sqrt(sum over band j of |rfft(w s_t, 512)|^2), 15 bands from 150 Hz
    segments of 30 frames: d_m by the measure; score = mean d_m, 1e-5 for T < 30
"""
import functools

import numpy as np

FS, NF, HOP, NFFT, J, N = 10000, 256, 128, 512, 15, 30
BETA, DYN, EPS = -15.0, 40.0, 2.0 ** -52
SENTINEL = 1e-5
LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]     # the issue's literals
HI = LO[1:] + [219]


def window():
    i = np.arange(NF)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (i + 1) / (NF + 1)))


def frames(length):
    return 0 if length < NF else (length - NF) // HOP + 1


def band_edges():
    """(lo, hi) by the formula: the bins nearest 150 2^((2j -+ 1) / 6) Hz."""
    f = np.arange(NFFT // 2 + 1) * FS / NFFT
    j = np.arange(J)
    lo = [int(np.argmin(np.abs(f - 150.0 * 2.0 ** ((2 * k - 1) / 6.0)))) for k in j]
    hi = [int(np.argmin(np.abs(f - 150.0 * 2.0 ** ((2 * k + 1) / 6.0)))) for k in j]
    return lo, hi


def frame_energies(x):
    """e[k] in dB of every frame of x."""
    x = np.asarray(x, np.float64)
    w = window()
    K = frames(x.size)
    return np.array([20.0 * np.log10(np.linalg.norm(w * x[k * HOP:k * HOP + NF]) + EPS)
                     for k in range(K)], np.float64)


def kept_frames(x):
    e = frame_energies(x)
    if e.size == 0:
        return np.zeros(0, np.int64)
    return np.flatnonzero(e > e.max() - DYN)


def remove_silence(sig, keep):
    sig = np.asarray(sig, np.float64)
    w = window()
    T = len(keep)
    s = np.zeros((T - 1) * HOP + NF if T else 0)
    for j, k in enumerate(keep):
        s[j * HOP:j * HOP + NF] += w * sig[k * HOP:k * HOP + NF]
    return s


def envelopes(s, T):
    """[J, T] band envelopes of the silence-removed signal s (exactly T frames)."""
    w = window()
    out = np.zeros((J, T))
    for t in range(T):
        S = np.fft.rfft(w * s[t * HOP:t * HOP + NF], NFFT)
        p = S.real ** 2 + S.imag ** 2
        for j in range(J):
            out[j, t] = np.sqrt(np.sum(p[LO[j]:HI[j]]))
    return out


def _rows(a):
    a = a - a.mean(axis=1, keepdims=True)
    return a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)


def _cols(a):
    a = a - a.mean(axis=0, keepdims=True)
    return a / (np.linalg.norm(a, axis=0, keepdims=True) + EPS)


def score(x, y, extended=False, detail=None):
    """-> (score, T).  detail: a dict that receives `clipped`, the elements of
    all segments where the clipping bound was the smaller (STOI only)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 1
    keep = kept_frames(x)
    T = len(keep)
    if detail is not None:
        detail["clipped"] = 0
    if T < N:
        return SENTINEL, T
    X = envelopes(remove_silence(x, keep), T)
    Y = envelopes(remove_silence(y, keep), T)
    clip = 1.0 + 10.0 ** (-BETA / 20.0)
    d = []
    for m in range(N, T + 1):
        Xm, Ym = X[:, m - N:m], Y[:, m - N:m]
        if extended:
            d.append(np.sum(_cols(_rows(Xm)) * _cols(_rows(Ym))) / N)
        else:
            alpha = np.linalg.norm(Xm, axis=1, keepdims=True) / (
                np.linalg.norm(Ym, axis=1, keepdims=True) + EPS)
            Yp = np.minimum(alpha * Ym, clip * Xm)
            if detail is not None:
                detail["clipped"] += int(np.sum(clip * Xm < alpha * Ym))
            d.append(np.sum(_rows(Xm) * _rows(Yp)) / J)
    return float(np.sum(d) / len(d)), T


# ------------------------------------------------------------------ fixtures
def speechlike(length, seed):
    """A harmonic stack with a slow envelope plus weak noise, at 10 kHz."""
    rng = np.random.default_rng(seed)
    n = np.arange(length)
    f0 = rng.uniform(110.0, 190.0)
    x = np.zeros(length)
    for h in range(1, 22):
        x += np.sin(2 * np.pi * h * f0 * n / FS + rng.uniform(0, 2 * np.pi)) / h ** 0.7
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.0, 5.0) * n / FS + rng.uniform(0, 6.0))
    return 0.1 * env * x + 1e-3 * rng.standard_normal(length)


class Fixture:
    def __init__(self, name, length, seed, noise=0.02, zeroed=None, quiet=(), zeros=False):
        self.name, self.length, self.seed = name, length, seed
        self.noise, self.zeroed, self.quiet, self.zeros = noise, zeroed, quiet, zeros

    def __repr__(self):
        return self.name

    @functools.cached_property
    def clean(self):
        if self.zeros:
            return np.zeros(self.length)
        x = speechlike(self.length, self.seed)
        for a, b in self.quiet:
            x[a:b] *= 1e-4
        x.setflags(write=False)
        return x

    @functools.cached_property
    def restored(self):
        if self.zeros:
            return np.zeros(self.length)
        rng = np.random.default_rng(self.seed + 500)
        y = self.clean + self.noise * rng.standard_normal(self.length)
        if self.zeroed:
            y[self.zeroed[0]:self.zeroed[1]] = 0.0
        y.setflags(write=False)
        return y


FIXTURES = [
    Fixture("len255", 255, 1),                              # no frame: sentinel
    Fixture("len3840", 3840, 2),                            # 29 frames: sentinel
    Fixture("len3968", 3968, 3, zeroed=(1500, 1900)),       # 30 frames: one segment
    Fixture("len4095", 4095, 4),                            # 30 frames
    Fixture("len4096", 4096, 5, zeroed=(2000, 2300)),       # 31 frames
    Fixture("len4224", 4224, 6),                            # 32 frames
    Fixture("len8000", 8000, 7, zeroed=(3000, 3800)),       # 61 frames
    Fixture("silence", 9000, 8, zeroed=(5000, 5600),
            quiet=((0, 700), (3000, 4500), (8500, 9000))),  # frames dropped at both ends and inside
    Fixture("clip", 6000, 9, noise=0.3),                    # noisy enough to reach the clipping bound
    Fixture("zeros", 5000, 10, zeros=True),
]
BY_NAME = {f.name: f for f in FIXTURES}
FRAME_COUNTS = {255: 0, 3840: 29, 3968: 30, 4095: 30, 4096: 31, 4224: 32, 8000: 61}


@functools.lru_cache(maxsize=None)
def reference(name, extended):
    """(score, T) of a fixture; computed once, shared."""
    f = BY_NAME[name]
    return score(f.clean, f.restored, extended)


def pair_sensitivity(x, y, seed=0):
    """The largest change of the oracle's score (either measure) when both
    inputs are perturbed by a relative 1e-13 randn, over three seeds."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    base = [score(x, y, ext)[0] for ext in (False, True)]
    E = 0.0
    for k in range(3):
        rng = np.random.default_rng(seed + 1000 + k)
        xp = x * (1.0 + 1e-13 * rng.standard_normal(x.size))
        yp = y * (1.0 + 1e-13 * rng.standard_normal(y.size))
        for ext in (False, True):
            E = max(E, abs(score(xp, yp, ext)[0] - base[ext]))
    return E


def threshold_margin(x):
    """The smallest distance in dB of a frame energy of x from the keep threshold."""
    e = frame_energies(x)
    return float(np.min(np.abs(e - (e.max() - DYN)))) if e.size else np.inf


@functools.lru_cache(maxsize=None)
def sensitivity(name):
    """pair_sensitivity of a fixture; computed once, shared."""
    f = BY_NAME[name]
    return pair_sensitivity(f.clean, f.restored, f.seed)
