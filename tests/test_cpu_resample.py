"""Host side of the polyphase resampler (no GPU): the filter design and the
closed-form reference against scipy, the output-length rule, the host plan of
csrc/resample_plan.h through its C query, and the ABI."""
import os
import re
from math import gcd

import numpy as np
import pytest

import resample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ainp.h")

RATIOS = [(3, 1), (1, 3), (2, 1), (1, 2), (6, 2), (5, 7), (147, 160), (160, 441), (441, 160)]
LDS_MAX = 160 * 1024
PLAN_RATIOS = [(147, 160), (160, 147), (160, 441), (441, 160), (1009, 1000)]


def _tpp(up, down):
    return resample_ref.taps_per_phase(up, down)


# ----------------------------------------------------------- filter design
@pytest.mark.parametrize("up,down", RATIOS)
def test_design_matches_firwin(up, down):
    """An indexing or normalisation mistake is O(1); measured 6.1e-16 max|h|.
    The bound leaves two orders for i0 implementations that differ between
    numpy and scipy versions."""
    signal = pytest.importorskip("scipy.signal")
    from ainp import resample as rs
    g = gcd(up, down)
    R = max(up, down) // g
    L = 20 * R + 1
    want = (up // g) * signal.firwin(L, 1.0 / R, window=("kaiser", 5.0))
    for name, (h, half) in (("ref", resample_ref.design(up, down)), ("ainp", rs.design(up, down))):
        assert half == 10 * R and h.shape == (L,) and h.dtype == np.float64, name
        err = np.max(np.abs(h - want)) / np.max(np.abs(want))
        print(f"{name} ({up},{down}): filter error {err:.2e} of max|h|")
        assert err <= 1e-13, (name, err)


# -------------------------------------------------------------- direct sum
def _lengths(up, down):
    g = gcd(up, down)
    return [1, 2, 7, 63, 64, 65, 1000, 20 * max(up, down) // g + 1]


@pytest.mark.parametrize("up,down", RATIOS)
def test_direct_sum_matches_scipy(up, down):
    """Both sides round: 2 (tpp + 3) 2^-53 S[m]."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(1000 * up + down)
    tpp = _tpp(up, down)
    for n in _lengths(up, down):
        x = rng.standard_normal(n)
        want = signal.resample_poly(x, up, down)
        got = resample_ref.resample(x, up, down)
        assert got.shape == want.shape, (n, got.shape, want.shape)
        assert got.shape[0] == resample_ref.out_len(n, up, down)
        bound = 2 * (tpp + 3) * 2.0 ** -53 * resample_ref.abs_sum(x, up, down)
        err = np.abs(got - want)
        print(f"({up},{down}) n={n}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), (n, float(np.max(err - bound)))


def test_direct_sum_is_a_copy_at_unit_ratio():
    x = np.random.default_rng(3).standard_normal(17)
    assert np.array_equal(resample_ref.resample(x, 4, 4), x)
    assert np.array_equal(resample_ref.abs_sum(x, 4, 4), np.abs(x))


# ----------------------------------------------------------- output length
def test_out_len_is_exact():
    from ainp import resample as rs
    ns = [0, 1, 2, 3, 63, 64, 65, 1000, 65535, 65536, 2 ** 24 + 1, 2 ** 31 - 2, 2 ** 31 - 1]
    ratios = RATIOS + [(4, 4), (1009, 1000), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1),
                       (2 ** 31 - 1, 2 ** 31 - 2)]
    for up, down in ratios:
        for n in ns:
            want = -(-(n * up) // down)          # Python integers: exact
            assert rs.out_len(n, up, down) == want, (n, up, down)
            assert resample_ref.out_len(n, up, down) == want
    # unchanged by a common factor
    for up, down in RATIOS:
        for f in (2, 3, 1000):
            for n in ns:
                assert rs.out_len(n, f * up, f * down) == rs.out_len(n, up, down)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 1, 0), (2 ** 31, 1, 1)):
        with pytest.raises(ValueError):
            rs.out_len(*bad)


# -------------------------------------------------------------------- plan
def _plan_cases():
    for up in range(1, 65):
        for down in range(1, 65):
            yield up, down
    yield from PLAN_RATIOS


def _read_indices(m, p):
    """Every input index the closed form reads for output m (n_in unbounded)."""
    c = m * p.down + p.half
    # 0 <= c - i up < L
    lo = -((p.taps - 1 - c) // p.up)        # ceil((c - L + 1) / up)
    hi = c // p.up
    return lo, hi


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_plan_fits_lds_and_covers_the_span(dtype):
    from ainp import resample as rs
    esize = np.dtype(dtype).itemsize
    for up, down in _plan_cases():
        p = rs.plan(up, down, dtype)
        g = gcd(up, down)
        assert (p.up, p.down) == (up // g, down // g)
        assert 0 <= p.lds_bytes <= LDS_MAX, (up, down, p)
        if p.up == p.down == 1:
            assert p.route == rs.RS_COPY
            continue
        R = max(p.up, p.down)
        assert p.half == 10 * R and p.taps == 20 * R + 1
        assert p.tpp == -(-p.taps // p.up) and p.pitch >= p.tpp and p.pitch % 2 == 1
        assert p.table_elems == p.up * p.pitch
        assert p.tile >= 64 and p.tile % 64 == 0
        # the table goes to LDS when it fits beside the span of the smallest
        # tile (64 outputs, staged in whole 16-byte groups from an aligned start)
        table_bytes = p.table_elems * esize
        v = 16 // esize
        span64 = ((p.up - 1) + 63 * p.down) // p.up + p.tpp
        fits = table_bytes + (span64 + 2 * (v - 1)) // v * v * esize <= LDS_MAX
        assert p.route == (rs.RS_LDS_TABLE if fits else rs.RS_GLOBAL_TABLE), (up, down, p)
        assert p.lds_bytes >= (table_bytes if fits else 0) + (p.span + v - 1) * esize
        # the span staged for the tile starting at m0 holds every index its
        # first and its last output read
        for tile_no in (0, 1, 2, 7, 12345):
            m0 = tile_no * p.tile
            base = (m0 * p.down + p.half) // p.up - p.tpp + 1
            for m in (m0, m0 + p.tile - 1):
                lo, hi = _read_indices(m, p)
                assert base <= lo and hi < base + p.span, (up, down, tile_no, m, lo, hi, base, p)


def test_plan_routes_of_the_large_ratio():
    from ainp import resample as rs
    assert rs.plan(1009, 1000, "float64").route == rs.RS_GLOBAL_TABLE   # 1009 * 21 * 8 B > 160 KB
    assert rs.plan(1009, 1000, "float32").route == rs.RS_LDS_TABLE
    assert rs.plan(3, 1, "float64").route == rs.RS_LDS_TABLE
    assert rs.plan(6, 2, "float32") == rs.plan(3, 1, "float32")


def test_plan_refuses_what_it_cannot_stage():
    from ainp import _lib, resample as rs
    for up, down in ((0, 1), (1, 0), (-3, 2), (1, 100000), (2 ** 31 - 1, 2 ** 31 - 2)):
        with pytest.raises(_lib.AinpError, match="bad argument"):
            rs.plan(up, down, "float32")
    with pytest.raises(TypeError):
        rs.plan(3, 1, "float16")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("up,down", RATIOS + [(1009, 1000)])
def test_table_layout_inverts_to_the_filter(up, down, dtype):
    from ainp import resample as rs
    p = rs.plan(up, down, dtype)
    h, half = rs.design(up, down)
    table = rs.host_table(up, down, dtype)
    assert table.shape == (p.up, p.pitch) and table.dtype == np.dtype(dtype)
    assert table.size == p.table_elems
    back = rs.table_to_filter(table, p.up, p.tpp, p.taps)
    assert np.array_equal(back, h.astype(dtype))
    # element by element: table[p][k] = h[p + (tpp - 1 - k) up], zero elsewhere
    hd = h.astype(dtype)
    for ph in {0, 1 % p.up, p.up // 2, p.up - 1}:
        for k in range(p.pitch):
            t = ph + (p.tpp - 1 - k) * p.up
            want = hd[t] if (k < p.tpp and 0 <= t < p.taps) else 0
            assert table[ph, k] == want, (ph, k)


# --------------------------------------------------------------------- ABI
def test_entry_points_are_declared_bound_and_exported():
    import ctypes
    from ctypes import c_int, c_int64, c_void_p
    from ainp import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert ("int ainp_resample_poly(void* y, const void* x, const void* table, int64_t rows, "
            "int64_t stride_in, int64_t stride_out, const int32_t* n_in, int up, int down, "
            "int dtype, void* stream);") in src
    assert "int64_t ainp_resample_out_len(int64_t n_in, int up, int down);" in src
    assert ("int ainp_resample_plan_query(int up, int down, int dtype, "
            "AinpResamplePlan* plan);") in src
    P = c_void_p
    f = _lib.lib.ainp_resample_poly
    assert f.restype is c_int
    assert list(f.argtypes) == [P, P, P, c_int64, c_int64, c_int64, P, c_int, c_int, c_int, P]
    f = _lib.lib.ainp_resample_out_len
    assert f.restype is c_int64 and list(f.argtypes) == [c_int64, c_int, c_int]
    f = _lib.lib.ainp_resample_plan_query
    assert f.restype is c_int
    assert list(f.argtypes) == [c_int, c_int, c_int, ctypes.POINTER(_lib.ResamplePlan)]
    # the struct as the header lays it out: nine ints, padding, two int64
    assert ctypes.sizeof(_lib.ResamplePlan) == 56
    assert _lib.ResamplePlan.table_elems.offset == 40
    # bad arguments stop before any launch, through the usual error record
    assert _lib.lib.ainp_resample_poly(None, None, None, 1, 8, 8, None, 0, 1, 0, None) == -1
    assert b"ainp_resample_poly: bad argument" in _lib.lib.ainp_last_error()
    assert _lib.lib.ainp_resample_poly(None, None, None, 1, 8, 8, None, 3, 1, 2, None) == -1
    assert _lib.lib.ainp_resample_poly(None, None, None, 1, 8, 8, None, 3, 1, 0, None) == -1
    # rows == 0 is a no-op
    assert _lib.lib.ainp_resample_poly(None, None, None, 0, 8, 8, None, 3, 1, 0, None) == 0


def test_torch_operators_are_registered():
    import torch
    from ainp import ops  # noqa: F401
    assert hasattr(torch.ops.ainp, "resample_poly")
    assert torch.ops.ainp.resample_out_len(7, 3, 2) == 11
    assert list(torch.ops.ainp.resample_plan_query(6, 2, 1))[:3] == [3, 1, 30]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.resample_poly(torch.zeros(8), 3, 1)
