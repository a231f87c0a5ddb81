"""Independent float64 references of the two autoregressive baselines beyond
Janssen + "lpc", written from the definitions (MATLAB arburg for real input;
the reference project's models/AudioReg/utils/janssen_inp.m with method
"arburg" and utils/arinpaint.m), for the tests only.  numpy alone.

They share no structure with csrc/ar_fit.h or csrc/ar_extrapolate.hip: Burg
works on whole vectors that really shrink, Janssen keeps janssen_ref's dense
|M| x N matrix and dense Cholesky, and the extrapolation is a plain loop over
the recursion.
"""
import numpy as np

from janssen_ref import lpc


def arburg(x, p, dtype=np.float64):
    """MATLAB arburg(x, p), real x: [1, a_1 .. a_p].  dtype: the accumulation
    width (np.longdouble gives the second formulation of the CPU tests).
    Raises ZeroDivisionError where the denominator is not positive."""
    x = np.asarray(x, dtype)
    ef, eb = x[1:].copy(), x[:-1].copy()
    a = np.ones(1, dtype)
    for _ in range(p):
        den = np.sum(ef * ef) + np.sum(eb * eb)
        if not den > 0:
            raise ZeroDivisionError("Burg denominator is not positive")
        k = -2 * np.sum(eb * ef) / den
        ef, eb = (ef + k * eb)[1:], (eb + k * ef)[:-1]
        a = np.concatenate((a, [0])) + k * np.concatenate(([0], a[::-1]))
    return a.astype(np.float64)


def fit(x, p, method):
    return arburg(x, p) if method == "arburg" else lpc(x, p)


def janssen(x, gap_start, gap_len, p, maxit, method="arburg"):
    """janssen_ref.janssen with the estimator chosen -> (solution, history
    [iterations done, gap_len], iterations done)."""
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
        a = fit(sol, p, method)
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


def crossfade_weights(h):
    """cos^2(linspace(0, pi/2, h)) with MATLAB's linspace: for h = 1 the single
    point is the END of the interval, pi/2 (numpy's would be the start)."""
    ang = np.array([np.pi / 2]) if h == 1 else np.linspace(0.0, np.pi / 2, h)
    return np.cos(ang) ** 2


def predict(context, h, p, method):
    """h samples past the end of `context`: mean removed, AR fit, the recursion
    y[t] = -sum_k a[k] y[t-k] as a direct loop, mean added back.  -> (samples,
    constant) with constant True where the context is constant and the side
    predicts its mean."""
    c = np.asarray(context, np.float64)
    mean = np.sum(c) / len(c)
    y = c - mean
    if not np.any(y):
        return np.full(h, mean), True
    a = fit(y, p, method)
    buf = np.concatenate((y[len(y) - p:], np.zeros(h)))
    for t in range(h):
        buf[p + t] = -np.dot(a[1:], buf[t:p + t][::-1])      # k = 1..p: buf[p + t - k]
    return buf[p:] + mean, False


def extrapolate(x, gap_start, gap_len, p, w, method="lpc"):
    """arinpaint.m on one segment -> (solution, status): status 1, or 0 when a
    side had a constant context."""
    x = np.array(x, np.float64)
    n, s, h = len(x), gap_start, gap_len
    pre = x[max(0, s - w):s]
    post = x[s + h:min(n, s + h + w)][::-1]
    assert len(pre) > p and len(post) > p
    fwd, c0 = predict(pre, h, p, method)
    bwd, c1 = predict(post, h, p, method)
    wts = crossfade_weights(h)
    x[s:s + h] = wts * fwd + (1.0 - wts) * bwd[::-1]
    return x, 0 if (c0 or c1) else 1
