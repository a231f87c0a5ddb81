"""float64 reference of scipy.signal.resample_poly(x, up, down) with its
defaults (window=("kaiser", 5.0), padtype="constant"), in closed form.  Plain
numpy, no scipy: the GPU tests compare against this, test_cpu_resample.py
compares this against scipy.

    g = gcd(up, down); up /= g; down /= g; R = max(up, down); half = 10 R
    L = 2 half + 1
    h[t] = up sinc((t - half) / R) / R kaiser_5(L)[t] / sum(the same without up)
    y[m] = sum_i x[i] h[m down + half - i up],  0 <= i < n_in, h index in [0, L)
    len(y) = ceil(n_in up / down)
"""
from math import gcd

import numpy as np


def reduce_ratio(up, down):
    g = gcd(int(up), int(down))
    return int(up) // g, int(down) // g


def design(up, down, beta=5.0):
    """(h, half) for the reduced ratio; (array([1.]), 0) when it is 1:1."""
    up, down = reduce_ratio(up, down)
    if up == 1 and down == 1:
        return np.ones(1), 0
    R = max(up, down)
    half = 10 * R
    L = 2 * half + 1
    t = np.arange(L, dtype=np.float64)
    # sinc((t - half) / R) / R in scipy.signal.firwin's order of evaluation: at
    # the taps where the sinc is zero both sides then hold the same rounding
    # residue of sin(pi k), which no bound relative to |h| would cover
    fc = 1.0 / R
    h = fc * np.sinc(fc * (t - half)) * np.kaiser(L, beta)
    return up * (h / h.sum()), half


def out_len(n_in, up, down):
    up, down = reduce_ratio(up, down)
    return -(-(int(n_in) * up) // down)


def _direct(x, h, half, up, down):
    """sum_i x[i] h[m down + half - i up] for every m at once: with
    c = m down + half the h indices congruent to c modulo up are c mod up + j up,
    met by the inputs i = c // up - j."""
    n_in = len(x)
    n_out = -(-(n_in * up) // down)
    L = len(h)
    c = np.arange(n_out, dtype=np.int64) * down + half
    p, q = c % up, c // up
    y = np.zeros(n_out)
    for j in range(-(-L // up)):
        hi, i = p + j * up, q - j
        ok = (hi < L) & (i >= 0) & (i < n_in)
        y[ok] += x[i[ok]] * h[hi[ok]]
    return y


def resample(x, up, down):
    """The reference result, float64 [ceil(n_in up / down)]."""
    x = np.asarray(x, dtype=np.float64)
    up, down = reduce_ratio(up, down)
    if up == 1 and down == 1:
        return x.copy()
    h, half = design(up, down)
    return _direct(x, h, half, up, down)


def abs_sum(x, up, down):
    """S[m] = sum_i |x[i]| |h[m down + half - i up]|: the scale of the rounding
    error of output m."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    up, down = reduce_ratio(up, down)
    if up == 1 and down == 1:
        return x.copy()
    h, half = design(up, down)
    return _direct(x, np.abs(h), half, up, down)


def taps_per_phase(up, down):
    up, down = reduce_ratio(up, down)
    if up == 1 and down == 1:
        return 1
    return -(-(20 * max(up, down) + 1) // up)
