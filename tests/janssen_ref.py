"""Independent float64 reference of the gap-wise Janssen algorithm, written
from the definition (Janssen, Veldhuis, Vries 1986; the reference project's
models/AudioReg/utils/janssen_inp.m with method "lpc"), for the tests only.

It shares no structure with csrc/janssen.hip: the AR fit takes MATLAB lpc's
route (biased autocorrelation by FFT, then Levinson-Durbin), the missing
samples come from the dense |M| x N matrix AA[i, n] = b[|M_i - n|] (|.| <= p)
and a dense Cholesky factorisation of its |M| x |M| block -- no Toeplitz
shortcut anywhere.
"""
import numpy as np


def lpc(x, p):
    """MATLAB lpc(x, p): [1, a_1 .. a_p] from the biased autocorrelation
    (computed by FFT as MATLAB does) and the Levinson-Durbin recursion."""
    x = np.asarray(x, np.float64)
    n = len(x)
    nfft = 1 << int(np.ceil(np.log2(2 * n - 1)))
    X = np.fft.rfft(x, nfft)
    r = np.fft.irfft(np.abs(X) ** 2, nfft)[:p + 1] / n
    a = np.zeros(p + 1)
    a[0] = 1.0
    e = r[0]
    for m in range(1, p + 1):
        k = -(r[m] + np.dot(a[1:m], r[m - 1:0:-1])) / e
        a[1:m] = a[1:m] + k * a[m - 1:0:-1]
        a[m] = k
        e *= 1.0 - k * k
    return a


def janssen(x, gap_start, gap_len, p, maxit):
    """-> (solution, history [iterations done, gap_len], iterations done).
    x: the segment (whatever it holds on the gap is ignored)."""
    x = np.array(x, np.float64)
    n = len(x)
    miss = np.arange(gap_start, gap_start + gap_len)
    obs = np.setdiff1d(np.arange(n), miss)
    sol = x.copy()
    sol[miss] = 0.0
    dist = np.abs(miss[:, None] - np.arange(n)[None, :])
    near = dist <= p
    history = []
    for _ in range(maxit):
        if not np.any(sol):
            break
        a = lpc(sol, p)
        b = np.array([np.dot(a[:p + 1 - k], a[k:]) for k in range(p + 1)])
        AA = np.zeros(dist.shape)
        AA[near] = b[dist[near]]
        try:
            L = np.linalg.cholesky(AA[:, miss])
        except np.linalg.LinAlgError:
            break
        rhs = AA[:, obs] @ x[obs]
        sol[miss] = -np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        history.append(sol[miss].copy())
    return sol, np.array(history).reshape(len(history), gap_len), len(history)


def gap_sdr(clean, restored, gap_start, gap_len):
    g = slice(gap_start, gap_start + gap_len)
    return 10.0 * np.log10(np.sum(clean[g] ** 2) / np.sum((clean[g] - restored[g]) ** 2))


def sinusoid_mix(n, noise=0.0, seed=0):
    """The known-answer signal of the Janssen tests (16 kHz), optionally with
    seeded Gaussian noise."""
    t = np.arange(n, dtype=np.float64)
    x = (0.5 * np.sin(2 * np.pi * 440 / 16000 * t + 0.3)
         + 0.3 * np.sin(2 * np.pi * 1210 / 16000 * t + 1.1)
         + 0.2 * np.sin(2 * np.pi * 3170 / 16000 * t + 2.0))
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(n)
    return x


def harmonic_signal(n, seed=0, sr=16000):
    """24 harmonics of a 120 Hz tone with 3 Hz vibrato plus 1e-3 noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    phase = 2 * np.pi * 120.0 * t + (120.0 * 0.02 / 3.0) * np.sin(2 * np.pi * 3.0 * t)
    x = np.zeros(n)
    for k in range(1, 25):
        x += rng.uniform(0.3, 1.0) / k * np.sin(k * phase + rng.uniform(0, 2 * np.pi))
    return x / np.max(np.abs(x)) * 0.8 + 1e-3 * rng.standard_normal(n)
