"""The filter of scipy.signal.resample_poly, designed on the host.

resample_poly(x, up, down) with its defaults (window=("kaiser", 5.0),
padtype="constant"; scipy documents them as MATLAB resample(x, p, q)'s, which
models/AudioReg/train.m:72,203 calls) is, with the ratio reduced by its gcd,
R = max(up, down), half = 10 R and L = 2 half + 1:

    h[t] = up * sinc((t - half) / R) / R * kaiser_5(L)[t] / sum(the same without up)
    y[m] = sum_i x[i] * h[m * down + half - i * up],   0 <= i < n_in, h index in [0, L)
    len(y) = ceil(n_in * up / down)

design builds h in float64 from np.sinc and np.kaiser (no scipy at run time);
device_table lays it out phase-major as ainp_resample_poly reads it
(include/ainp.h, csrc/resample_plan.h): table[p][k] = h[p + (tpp - 1 - k) * up],
zero-padded to the plan's pitch.  plan and out_len are the C queries; they
launch nothing and work without a GPU.  Host results are cached per argument
set, device copies per (arguments, device).
"""
from __future__ import annotations

import functools
from math import gcd
from typing import NamedTuple, Tuple

import numpy as np

from . import _lib

RS_COPY = 0            # include/ainp.h AINP_RS_COPY
RS_LDS_TABLE = 1       # AINP_RS_LDS_TABLE
RS_GLOBAL_TABLE = 2    # AINP_RS_GLOBAL_TABLE
ROUTE_NAMES = {RS_COPY: "RS_COPY", RS_LDS_TABLE: "RS_LDS_TABLE",
               RS_GLOBAL_TABLE: "RS_GLOBAL_TABLE"}


def reduce_ratio(up: int, down: int) -> Tuple[int, int]:
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("resampling needs up >= 1 and down >= 1")
    g = gcd(up, down)
    return up // g, down // g


@functools.lru_cache(maxsize=None)
def _design(up: int, down: int, beta: float):
    R = max(up, down)
    half = 10 * R
    t = np.arange(2 * half + 1, dtype=np.float64)
    # sinc((t - half) / R) / R evaluated as scipy.signal.firwin does: where the
    # sinc is zero, both then hold the same rounding residue of sin(pi k)
    fc = 1.0 / R
    h = fc * np.sinc(fc * (t - half)) * np.kaiser(2 * half + 1, beta)
    h = up * (h / h.sum())
    h.setflags(write=False)
    return h, half


def design(up: int, down: int, beta: float = 5.0):
    """(h, half): the float64 filter of resample_poly(x, up, down) for the
    reduced ratio, L = 2 half + 1 taps (read-only, cached)."""
    return _design(*reduce_ratio(up, down), float(beta))


class Plan(NamedTuple):
    """AinpResamplePlan (include/ainp.h)."""
    up: int
    down: int
    half: int
    taps: int
    tpp: int
    pitch: int
    tile: int
    span: int
    route: int
    table_elems: int
    lds_bytes: int

    @property
    def route_name(self) -> str:
        return ROUTE_NAMES[self.route]


def _dtype_id(dtype) -> int:
    name = str(dtype).replace("torch.", "")
    if name not in ("float32", "float64"):
        raise TypeError(f"resampling runs in float32 or float64, not {dtype}")
    return int(name == "float64")


def plan(up: int, down: int, dtype="float32") -> Plan:
    """The plan ainp_resample_poly launches with (a host query)."""
    p = _lib.ResamplePlan()
    _lib.call("ainp_resample_plan_query", int(up), int(down), _dtype_id(dtype), p)
    return Plan(*(int(getattr(p, f)) for f in Plan._fields))


def out_len(n_in: int, up: int, down: int) -> int:
    """ceil(n_in * up / down), in exact integer arithmetic (a host query)."""
    n = int(_lib.lib.ainp_resample_out_len(int(n_in), int(up), int(down)))
    if n < 0:
        raise ValueError("out_len needs 0 <= n_in <= 2**31 - 1, up >= 1 and down >= 1")
    return n


def phase_table(h: np.ndarray, up: int, tpp: int, pitch: int) -> np.ndarray:
    """[up, pitch]: row p holds h[p + j * up] for j = tpp - 1 .. 0 (the order in
    which the inner loop meets ascending inputs), zeros past the end of h and
    in the padding."""
    table = np.zeros((up, pitch), dtype=h.dtype)
    for p in range(min(up, len(h))):
        taps = h[p::up]
        table[p, tpp - len(taps):tpp] = taps[::-1]
    return table


def table_to_filter(table: np.ndarray, up: int, tpp: int, taps: int) -> np.ndarray:
    """phase_table inverted: h back from its table."""
    h = np.zeros(taps, dtype=table.dtype)
    for p in range(min(up, taps)):
        n = len(h[p::up])
        h[p::up] = table[p, tpp - n:tpp][::-1]
    return h


@functools.lru_cache(maxsize=None)
def _host_table(up: int, down: int, dtype_name: str) -> np.ndarray:
    p = plan(up, down, dtype_name)
    if p.route == RS_COPY:
        raise ValueError("up == down needs no table")
    h, _ = design(up, down)
    # rounded once, float64 -> the element type, as scipy casts the filter
    table = phase_table(h, p.up, p.tpp, p.pitch).astype(dtype_name)
    table.setflags(write=False)
    return table


def host_table(up: int, down: int, dtype="float32") -> np.ndarray:
    up, down = reduce_ratio(up, down)
    return _host_table(up, down, ("float32", "float64")[_dtype_id(dtype)])


# device copies, keyed (up, down, dtype, device); ops._release_device_caches
# drops them at exit
_DEVICE_CACHE: dict = {}


def device_table(up: int, down: int, dtype, device):
    """host_table(...) as a tensor on `device`."""
    import torch
    up, down = reduce_ratio(up, down)
    name = ("float32", "float64")[_dtype_id(dtype)]
    key = (up, down, name, str(device))
    d = _DEVICE_CACHE.get(key)
    if d is None:
        d = torch.from_numpy(np.array(_host_table(up, down, name))).to(device)
        _DEVICE_CACHE[key] = d
    return d
