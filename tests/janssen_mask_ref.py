"""Independent float64 reference of the gap-wise Janssen algorithm for an
arbitrary set of missing samples (the reference project's
models/AudioReg/utils/janssen_inp.m, which takes any NaN pattern), for the
tests only: tests/janssen_ref.py::janssen with `miss` given.

It shares no structure with csrc/janssen_mask.hip: the AR fit is janssen_ref's
lpc (or ar_ref's arburg), the missing samples come from the dense |M| x N
matrix AA[i, n] = b[|M_i - n|] (|.| <= p) and numpy's dense Cholesky
factorisation of its |M| x |M| block -- no band, no envelope, no blocking.
"""
import numpy as np

from janssen_ref import gap_sdr, harmonic_signal, lpc, sinusoid_mix  # noqa: F401


def janssen(x, miss, p, maxit, fit=lpc):
    """-> (solution, history [iterations done, len(miss)], iterations done).
    x: the segment (whatever it holds on `miss` is ignored); miss: the missing
    samples, ascending; fit(x, p) -> [1, a_1 .. a_p]."""
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
        try:
            L = np.linalg.cholesky(AA[:, miss])
        except np.linalg.LinAlgError:
            break
        rhs = AA[:, obs] @ x[obs]
        sol[miss] = -np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        history.append(sol[miss].copy())
    return sol, np.array(history).reshape(len(history), len(miss)), len(history)


def runs(*pairs):
    """The index list of the runs [a, b) given."""
    return np.concatenate([np.arange(a, b) for a, b in pairs])


def set_sdr(clean, restored, miss):
    """The SDR over the samples `miss`, in dB."""
    return 10.0 * np.log10(np.sum(clean[miss] ** 2) / np.sum((clean[miss] - restored[miss]) ** 2))
