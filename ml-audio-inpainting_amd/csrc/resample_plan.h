// resample_plan.h — what the polyphase resampler (resample.hip) decides on the
// host: the reduced ratio, the filter's extent, the phase-major coefficient
// table's layout, the output tile of a workgroup with the input span it stages,
// and the route.  Plain C++17, no HIP: the launcher and the host query
// (ainp_resample_plan_query) both call rs_plan.
//
// The filter is scipy.signal.resample_poly's default (a Kaiser-5 windowed sinc
// of L = 2 half + 1 taps, half = 10 max(up, down)):
//   y[m] = sum_i x[i] h[m down + half - i up],  0 <= i < n_in, h index in [0, L).
// With c = m down + half, phase p = c mod up and q = floor(c / up), output m
// reads x[q - tpp + 1 + k] for k = 0 .. tpp - 1 (tpp = ceil(L / up) taps per
// phase) against table[p][k] = h[p + (tpp - 1 - k) up], zero where that index
// is >= L: each phase's taps lie in the order the inner loop reads x ascending.
//
// Limits: up, down >= 1 (any int), n_in <= 2^31 - 1 per row; after reduction
// 20 max(up, down) + 1 must fit an int and the span of RS_TILE_MIN outputs must
// fit in LDS (RS_LDS_MAX), else the plan is refused (ok == 0) and nothing is
// launched.  Every byte count here is the launch's: the plan is never wrong
// about LDS.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ainp.h"

namespace ainp {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE_MAX = 2048;          // outputs per workgroup, a multiple of RS_TILE_MIN
constexpr int RS_TILE_MIN = 64;            // one wave's worth
constexpr size_t RS_LDS_MAX = 160 * 1024;  // gfx950: one workgroup may take the whole CU's LDS
// the input span a tile is sized for while larger tiles would still fit: with
// a typical table beside it two workgroups share a CU
constexpr size_t RS_SPAN_PREF = 32 * 1024;

inline int64_t rs_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// ceil(n_in up / down) in exact integer arithmetic (n_in <= 2^31 - 1 and
// up < 2^31, so the product fits 64 bits); unchanged by a common factor
inline int64_t rs_out_len(int64_t n_in, int up, int down) {
  if (n_in < 0 || up < 1 || down < 1) return -1;
  const int64_t g = rs_gcd(up, down);
  const int64_t u = up / g, d = down / g;
  return (n_in * u + d - 1) / d;
}

// inputs staged for `tile` consecutive outputs: the first output's tpp taps
// and the largest advance of floor(c / up) over the tile, whatever the phase
// of its first output
inline int64_t rs_span(int64_t tile, int64_t up, int64_t down, int64_t tpp) {
  return ((up - 1) + (tile - 1) * down) / up + tpp;
}

// what the kernel allocates for a span: it stages from the 16-byte boundary
// at or below the first sample, in whole 16-byte groups
inline int64_t rs_span_lds(int64_t span, int esize) {
  const int64_t v = 16 / esize;
  return (span + (v - 1) + (v - 1)) / v * v;
}

struct RsPlan {
  int ok;        // 0: refused (see the limits above); nothing else is meaningful
  int up, down;  // reduced
  int half;      // 10 max(up, down); 0 for a copy
  int taps;      // L = 2 half + 1; 0 for a copy
  int tpp;       // ceil(L / up)
  int pitch;     // elements between phases in the table: tpp made odd
  int tile;      // outputs per workgroup
  int span;      // inputs a tile reads, from floor((m0 down + half) / up) - tpp + 1
  int route;     // AINP_RS_COPY / AINP_RS_LDS_TABLE / AINP_RS_GLOBAL_TABLE
  int64_t table_elems;   // up * pitch
  int64_t lds_bytes;     // dynamic LDS of a workgroup: span (+ table on AINP_RS_LDS_TABLE)
};

// esize: 4 (float32) or 8 (float64)
inline RsPlan rs_plan(int up, int down, int esize) {
  RsPlan p = {};
  if (up < 1 || down < 1 || (esize != 4 && esize != 8)) return p;
  const int g = (int)rs_gcd(up, down);
  p.up = up / g;
  p.down = down / g;
  if (p.up == 1 && p.down == 1) {
    p.ok = 1;
    p.route = AINP_RS_COPY;
    p.tile = RS_TILE_MAX;
    p.span = RS_TILE_MAX;
    return p;
  }
  const int64_t R = p.up > p.down ? p.up : p.down;
  if (20 * R + 1 > 0x7fffffff) return p;
  p.half = (int)(10 * R);
  p.taps = 2 * p.half + 1;
  p.tpp = (int)(((int64_t)p.taps + p.up - 1) / p.up);
  // An odd pitch (in elements) sends phases that differ modulo 32 to different
  // LDS banks, for 4-byte reads (bank = dword mod 32) and for 8-byte reads
  // (bank = dword mod 64, two dwords an element) alike; lanes of one phase
  // read one address, which is a broadcast.
  p.pitch = p.tpp | 1;
  p.table_elems = (int64_t)p.up * p.pitch;
  const int64_t table_bytes = p.table_elems * esize;
  auto span_bytes = [&](int64_t tile) {
    return rs_span_lds(rs_span(tile, p.up, p.down, p.tpp), esize) * esize;
  };
  const int64_t lds_max = (int64_t)RS_LDS_MAX;
  if (span_bytes(RS_TILE_MIN) > lds_max) return p;   // cannot be staged at all
  const bool tlds = table_bytes + span_bytes(RS_TILE_MIN) <= lds_max;
  p.route = tlds ? AINP_RS_LDS_TABLE : AINP_RS_GLOBAL_TABLE;
  const int64_t avail = lds_max - (tlds ? table_bytes : 0);
  const int64_t pref = avail < (int64_t)RS_SPAN_PREF ? avail : (int64_t)RS_SPAN_PREF;
  int tile = RS_TILE_MIN;   // fits in avail by the route's own test
  for (int t = RS_TILE_MAX; t > RS_TILE_MIN; t -= RS_TILE_MIN)
    if (span_bytes(t) <= pref) {
      tile = t;
      break;
    }
  p.tile = tile;
  p.span = (int)rs_span(tile, p.up, p.down, p.tpp);
  p.lds_bytes = span_bytes(tile) + (tlds ? table_bytes : 0);
  p.ok = 1;
  return p;
}

}  // namespace ainp
