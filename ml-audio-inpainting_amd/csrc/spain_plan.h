// spain_plan.h — what the SPAIN launchers decide on the host: the shape rules,
// lgN, the LDS plan of the transform and of a window kernel, the lane route.
// Plain C++17, no HIP: tests/sanitize/spain_plan_check.cpp walks it under ASan
// + UBSan without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ar_limits.h"

namespace ainp {

// ---- the window solvers (ainp_spain, ainp_spain_omp): w samples, M = red * w
constexpr int SP_WMIN = 8, SP_WMAX = 4096, SP_MMAX = 8192;
constexpr char SP_SHAPE_RULE[] =
    "w a power of two, 8 <= w <= 4096, red 1, 2 or 4, red * w <= 8192";
inline bool sp_shape_ok(int w, int red) {
  return w >= SP_WMIN && w <= SP_WMAX && (w & (w - 1)) == 0 && (red == 1 || red == 2 || red == 4) &&
         (int64_t)red * w <= SP_MMAX;
}

// ---- the whole-signal solver (ainp_spain_learned, ainp_spain_dgt)
constexpr int SL_MMIN = 8, SL_MMAX = 2048, SL_WMIN = 8;
constexpr int64_t SL_LMAX = (int64_t)1 << 22;   // the frame cap is SL_LMAX / a frames a signal
// the first rule (w, a, M, L) breaks, or nullptr
inline const char* sl_shape_rule(int64_t L, int w, int a, int M) {
  auto pow2 = [](int64_t v) { return v > 0 && (v & (v - 1)) == 0; };
  if (!pow2(M) || M < SL_MMIN || M > SL_MMAX) return "M a power of two, 8 <= M <= 2048";
  if (!pow2(w) || w < SL_WMIN || w > M) return "w a power of two, 8 <= w <= M";
  if (a < 1 || w % a != 0 || w / a < 2) return "a divides w, w / a >= 2";
  if (L < M || L % M != 0) return "L a positive multiple of M";
  if (L > SL_LMAX) return "L / a <= 2^22 / a frames, L <= 4194304";
  return nullptr;
}

// ---- the length-M real transform as N = M / 2 complex points in LDS
inline int sp_lgN(int M) {   // N = 1 << lgN
  int lgN = 0;
  while ((2 << lgN) < M) ++lgN;
  return lgN;
}
// Doubles: one of re / im (element i at i + i / 32), the quarter wave; for a
// window kernel also the row and, with OMP, each of its four vectors (z, b, a,
// l) beside nD column codes and two atom lists of nA ints.
struct SpLds {
  int nF, nCos, nRow, nD, nA;
  size_t bytes() const {
    return ((size_t)2 * nF + nRow + nCos + 4 * nD) * sizeof(double) +
           ((size_t)nD + 2 * nA) * sizeof(int);
  }
};
inline SpLds sp_fft_lds(int M) {
  const int N = M / 2;
  return {N + N / 32 + 2, (M / 4 + 2) & ~1, 0, 0, 0};
}
inline int sp_omp_dims(int w) { return w < AINP_SPAIN_OMP_DIMS ? w : AINP_SPAIN_OMP_DIMS; }
inline SpLds sp_window_lds(int w, int M, bool omp) {
  const SpLds f = sp_fft_lds(M);
  const int nD = omp ? sp_omp_dims(w) : 0;
  return {f.nF, f.nCos, w, nD, omp ? nD / 2 + 2 : 0};
}

// ---- lanes.  A lane holds EPL spectrum slots, 2 EPL time-domain sample pairs
// and ranks 2 EPL + 1 half-spectrum bins: transforms of N <= 1024 points run
// 256 lanes with 2 slots, longer ones (up to 4096) 512 lanes with 4.
constexpr int SP_NMAX_256 = 1024;
constexpr int SP_NT_BIG = 512, SP_EPL_BIG = 2048 / SP_NT_BIG;
inline bool sp_lanes_256(int M) { return M / 2 <= SP_NMAX_256; }

}  // namespace ainp
