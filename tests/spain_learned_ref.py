"""Float64 NumPy reference of A-SPAIN and S-SPAIN over the whole signal with a
Gabor frame and a unitary sparsity-enhancing basis (the reference project's
references/basisopt: a_spain_learned.m, s_spain_learned.m and
hard_thresholding_dgtreal.m), written from the algorithm as DESIGN §14.2
restates it, by LTFAT's documented definitions.  Test-only.

It shares no structure with csrc/spain_learned.hip: whole-array transforms with
numpy.fft, matrix products with @, a stable argsort for the threshold.  Every
pass records the smallest relative margin between the k-th and the (k+1)-th
ranked magnitude over the columns, and the objective, so that the tests can
assert that no parity input sits at a near-tie or at epsilon.  formulation 2
computes the same thing another way (full complex transforms, the basis
products summed in a permuted order) to measure what float64 round-off moves.
"""
import functools

import numpy as np

ALGS = ("aspain", "sspain")


# ------------------------------------------------------------ the Gabor frame
def windows(w, a, M):
    """-> (g, gd): the periodic Hann window and its painless canonical dual."""
    i = np.arange(w)
    g = 0.5 - 0.5 * np.cos(2 * np.pi * i / w)
    gd = g / (M * (g ** 2).reshape(-1, a).sum(axis=0)[i % a])
    return g, gd


def _index(L, w, a):
    n = np.arange(L // a)
    return (n[None, :] * a - w // 2 + np.arange(w)[:, None]) % L      # [w, N]


def dgt(x, win, a, M, full=False):
    """-> coefficients [K, N]."""
    w, L = len(win), len(x)
    buf = np.zeros((M, L // a))
    buf[(np.arange(w) - w // 2) % M] = x[_index(L, w, a)] * win[:, None]
    if full:
        return np.fft.fft(buf, axis=0)[:M // 2 + 1]
    return np.fft.rfft(buf, axis=0)


def idgt(c, win, a, M, L, full=False):
    w, K = len(win), M // 2 + 1
    if full:
        c = c.copy()
        c[0], c[K - 1] = c[0].real, c[K - 1].real
        spec = np.concatenate([c, np.conj(c[K - 2:0:-1])], axis=0)
        buf = np.fft.ifft(spec, axis=0).real * M
    else:
        buf = np.fft.irfft(c, M, axis=0) * M
    fr = buf[(np.arange(w) - w // 2) % M] * win[:, None]
    idx = _index(L, w, a)
    x = np.zeros(L)
    for n in range(L // a):                      # frame order
        x[idx[:, n]] += fr[:, n]
    return x


def hard_threshold(z, k, ties="low"):
    """-> (H_k(z) per column, the smallest relative margin over the columns
    between the k-th and the (k+1)-th ranked magnitude; two exact zeros are
    exempt).  Rows 0 and K-1 rank by |z| / sqrt 2; ties "low": the lower row
    first (a stable sort), "high": the higher row first."""
    K = z.shape[0]
    if k >= K:
        return z.copy(), np.inf
    mag = np.abs(z)
    mag[0] /= np.sqrt(2.0)
    mag[K - 1] /= np.sqrt(2.0)
    if ties == "low":
        order = np.argsort(-mag, axis=0, kind="stable")
    else:
        order = K - 1 - np.argsort(-mag[::-1], axis=0, kind="stable")
    ranked = np.take_along_axis(mag, order, axis=0)
    hi, lo = ranked[k - 1], ranked[k]
    live = hi > 0
    margin = float(((hi[live] - lo[live]) / hi[live]).min()) if live.any() else np.inf
    keep = np.zeros(z.shape, bool)
    np.put_along_axis(keep, order[:k], True, axis=0)
    return np.where(keep, z, 0.0), margin


def default_maxit(M, s=1, r=1):
    return -((-(M // 2 + 1) * r) // s)


def _products(U, formulation):
    """-> (apply U, apply U^H) on [K, N] arrays."""
    if U is None:
        return (lambda c: c), (lambda c: c)
    if formulation == 1:
        UH = U.conj().T
        return (lambda c: U @ c), (lambda c: UH @ c)
    perm = np.random.default_rng(3).permutation(U.shape[0])
    Up, UHp = U[:, perm], U.conj().T[:, perm]
    return (lambda c: Up @ c[perm]), (lambda c: UHp @ c[perm])


def spain_learned(x0, observed, U=None, algorithm="aspain", w=1024, a=256, M=None, s=1, r=1,
                  epsilon=0.1, maxit=None, ties="low", formulation=1):
    """-> dict(out, iters, obj [maxit] NaN after the last pass, stats [(margin,
    objective)] per evaluated pass).  len(x0) is a multiple of M."""
    M = 2 * w if M is None else M
    maxit = default_maxit(M, s, r) if maxit is None else maxit
    L = len(x0)
    assert L % M == 0
    g, gd = windows(w, a, M)
    full = formulation == 2
    fwd, adj = _products(U, formulation)
    obs = np.asarray(observed, bool)
    x = np.where(obs, x0, 0.0)
    x0 = x.copy()
    out, best = x.copy(), np.inf
    obj_hist, stats = np.full(maxit, np.nan), []
    k, cnt = s, 1
    if algorithm == "aspain":
        z = fwd(dgt(x, g, a, M, full))
        u = np.zeros_like(z)
    else:
        u = np.zeros(L)
    while cnt <= maxit:
        if algorithm == "aspain":
            zb, margin = hard_threshold(z + u, k, ties)
            obj = float(np.sqrt((np.abs(z - zb) ** 2).sum()))
        else:
            zb, margin = hard_threshold(fwd(dgt(x - u, gd, a, M, full)), k, ties)
            xe = idgt(adj(zb), g, a, M, L, full)
            obj = float(np.sqrt(((xe - x) ** 2).sum()))
        obj_hist[cnt - 1] = obj
        stats.append((margin, obj))
        if obj <= best:
            best, out = obj, x.copy()
        if obj <= epsilon:
            break
        if algorithm == "aspain":
            x = idgt(adj(zb - u), gd, a, M, L, full)
            x[obs] = x0[obs]
            z = fwd(dgt(x, g, a, M, full))
            u = u + z - zb
        else:
            xn = xe + u
            xn[obs] = x0[obs]
            u = u + xe - xn
            x = xn
        cnt += 1
        if cnt % r == 0:
            k += s
    return {"out": out, "iters": len(stats), "obj": obj_hist, "stats": stats}


def conditions(stats, epsilon):
    """-> (smallest margin, smallest |obj - epsilon| / epsilon) of a run."""
    margin = min(m for m, _ in stats)
    dist = min(abs(o - epsilon) / epsilon for _, o in stats) if epsilon > 0 else np.inf
    return margin, dist


# ------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def basis(K, level):
    """U = prod_{j<3} expm(2 pi i A_j), A_j tridiagonal Hermitian with entries
    bounded by `level`, through numpy.linalg.eigh."""
    rng = np.random.default_rng(7)
    U = np.eye(K, dtype=complex)
    for _ in range(3):
        d = rng.uniform(-level, level, K)
        off = (rng.uniform(-level, level, K - 1) + 1j * rng.uniform(-level, level, K - 1)) / np.sqrt(2)
        A = np.diag(d).astype(complex) + np.diag(off, 1) + np.diag(off.conj(), -1)
        lam, V = np.linalg.eigh(A)
        U = U @ ((V * np.exp(2j * np.pi * lam)) @ V.conj().T)
    return U


def signal(L):
    rng = np.random.default_rng(1)
    phase = rng.uniform(0, 6, 4)
    n = np.arange(L)
    amp, freq = (1, .6, .4, .3), (.031, .0777, .123, .211)
    clean = sum(a * np.sin(2 * np.pi * c * n + p) for a, c, p in zip(amp, freq, phase))
    return clean + 1e-3 * rng.standard_normal(L)


def mask(L, gaps):
    m = np.ones(L, bool)
    for g0, g1 in gaps:
        m[g0:g1] = False
    return m


# (w, a, M, L, gaps, level[, amplitude])
CASES = {
    "w8": (8, 2, 8, 64, ((30, 33),), 0.02),
    "w16_wraps": (16, 4, 32, 192, ((2, 10),), 0.02),
    "w64": (64, 16, 128, 768, ((301, 321),), 0.02),
    "w128": (128, 32, 256, 1024, ((531, 555),), 0.05),
    "w16_odd_frames": (16, 4, 32, 160, ((70, 78),), 0.02),       # N = 40: no multiple of 16 or 32
    "w64_two_gaps": (64, 16, 128, 768, ((301, 321), (350, 362)), 0.02),
    "w64_quiet": (64, 16, 128, 768, ((420, 431),), 0.02, 0.25),  # with w64: a batch, two stops
}
PARITY = ("w8", "w16_wraps", "w64", "w128", "w16_odd_frames", "w64_two_gaps", "w64_quiet")
BIG = dict(w=1024, a=256, M=2048, L=8192, gaps=((4000, 4300),), level=0.02, maxit=8)
# s 2, r 3, and maxit below the second keep-everything pass: there u = 0 and
# A-SPAIN's objective is pure round-off, which no relative bound can hold
SCHEDULE = ("w64", (("s", 2), ("r", 3), ("maxit", 90)))
# a unit impulse at a frame centre with w = M, a = w / 2: the neighbouring frames
# meet it at g[0] = 0, so one frame has an exactly flat spectrum and all others
# are zero but for two more samples that the impulse's frame does not reach.
# The gap lies in the impulse's frame and in the next one, so the kept row shapes
# what follows.  (An impulse alone will not do: x[n] -> (-1)^n x[n] mirrors the
# rows, the impulse is its own image, and the two tie rules would give mirrored
# runs with equal objectives.)
TIE = dict(w=16, a=8, M=16, L=64, at=16, more=((26, 0.7), (29, -0.4)), gap=(18, 21), epsilon=1e-3,
           maxit=4)
EPSILON = 0.1
# run_spain_learned_evaluation: of the nine bundled clips the first whose four
# runs (both algorithms, with and without a basis) stay 1e-8 clear of a tie
EVAL = dict(clip="1012-133424-0012.flac", w=256, a=64, M=512, maxit=6, level=0.02)


def case_input(name):
    """-> (clean, observed, U, w, a, M)."""
    w, a, M, L, gaps, level = CASES[name][:6]
    amplitude = CASES[name][6] if len(CASES[name]) > 6 else 1.0
    return amplitude * signal(L), mask(L, gaps), basis(M // 2 + 1, level), w, a, M


@functools.lru_cache(maxsize=None)
def case_reference(name, alg, with_basis, formulation=1, float32=False, ties="low", extra=()):
    clean, obs, U, w, a, M = case_input(name)
    x = clean.astype(np.float32).astype(np.float64) if float32 else clean
    return spain_learned(x, obs, U if with_basis else None, alg, w, a, M, epsilon=EPSILON,
                         ties=ties, formulation=formulation, **dict(extra))


@functools.lru_cache(maxsize=None)
def big_reference(alg, formulation=1):
    B = BIG
    clean, obs = signal(B["L"]), mask(B["L"], B["gaps"])
    return spain_learned(clean, obs, basis(B["M"] // 2 + 1, B["level"]), alg, B["w"], B["a"], B["M"],
                         epsilon=EPSILON, maxit=B["maxit"], formulation=formulation)


def tie_input():
    x = np.zeros(TIE["L"])
    x[TIE["at"]] = 1.0
    for at, v in TIE["more"]:
        x[at] = v
    return x, mask(TIE["L"], (TIE["gap"],))


@functools.lru_cache(maxsize=None)
def tie_reference(alg, ties="low"):
    x, obs = tie_input()
    return spain_learned(x, obs, None, alg, TIE["w"], TIE["a"], TIE["M"], epsilon=TIE["epsilon"],
                         maxit=TIE["maxit"], ties=ties)


def padded_reference(x, obs, U, alg, w, a, M, **kw):
    """spain_learned on x padded with observed zeros to the next multiple of M."""
    L = -(-len(x) // M) * M
    xp, mp = np.zeros(L), np.ones(L, bool)
    xp[:len(x)], mp[:len(x)] = x, obs
    return spain_learned(xp, mp, U, alg, w, a, M, epsilon=EPSILON, **kw)


def gap_scale(name):
    clean, obs = case_input(name)[:2]
    return float(np.abs(clean[~obs]).max())


def gap_sdr(clean, restored, obs):
    e = clean[~obs] - restored[~obs]
    return float(10 * np.log10((clean[~obs] ** 2).sum() / (e ** 2).sum()))
