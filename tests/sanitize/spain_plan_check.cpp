// spain_plan_check — walks csrc/spain_plan.h on the host, built with ASan +
// UBSan (csrc/Makefile `sanitize`):
//  - every legal (w, red) of the window solvers and the neighbours just outside:
//    the shape rule refuses what the launchers' former condition refused; nF,
//    nCos, lgN and the byte counts of the plain and the OMP plan are the former
//    expressions; the lane route is the former condition; with the kernels'
//    static arrays every plan fits the 160 KiB of a CU, and the largest plain
//    plan is 67584 + 32768 + 16392 bytes and 40 of padding;
//  - every legal M of the whole-signal solver and its neighbours, with legal
//    and illegal (w, a, L): the rule's text under a function name is the former
//    message, and the transform's plan is the former expression in its other
//    spelling.
// Exits 0 with "spain_plan_check OK".
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "../../ml-audio-inpainting_amd/csrc/spain_plan.h"

using namespace ainp;

static long long g_cells = 0;
static int g_fail = 0;

#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (g_fail++ < 20) {                                   \
        fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                        \
        fprintf(stderr, "\n");                               \
      }                                                      \
    }                                                        \
  } while (0)

// the static LDS of the kernels at 512 lanes (the compiler's resource report):
// histogram 1024 + wave sums 64 + the select's result 16; OMP: wave sums,
// argmax keys and bins, the two new solution entries
constexpr size_t STATIC_SPAIN = 1024 + 64 + 16, STATIC_OMP = 64 + 64 + 32 + 16;
constexpr size_t CU_LDS = 160 * 1024;

// the rules as spain.hip / spain_omp.hip and spain_learned.hip wrote them
static bool old_shape_ok(int w, int red) {
  return w >= 8 && w <= 4096 && (w & (w - 1)) == 0 && (red == 1 || red == 2 || red == 4) &&
         (int64_t)red * w <= 8192;
}
static bool old_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
static const char* old_sl_rule(int64_t L, int w, int a, int M) {
  if (!old_pow2(M) || M < 8 || M > 2048)
    return "ainp_spain_learned: bad argument (M a power of two, 8 <= M <= 2048)";
  if (!old_pow2(w) || w < 8 || w > M)
    return "ainp_spain_learned: bad argument (w a power of two, 8 <= w <= M)";
  if (a < 1 || w % a != 0 || w / a < 2)
    return "ainp_spain_learned: bad argument (a divides w, w / a >= 2)";
  if (L < M || L % M != 0) return "ainp_spain_learned: bad argument (L a positive multiple of M)";
  if (L > ((int64_t)1 << 22))
    return "ainp_spain_learned: bad argument (L / a <= 2^22 / a frames, L <= 4194304)";
  return nullptr;
}
static int old_lgN(int M) {
  int lgN = 0;
  while ((2 << lgN) < M) ++lgN;
  return lgN;
}

static void check_sl(int64_t L, int w, int a, int M) {
  ++g_cells;
  const char* was = old_sl_rule(L, w, a, M);
  const char* rule = sl_shape_rule(L, w, a, M);
  CHECK(!was == !rule, "L %lld w %d a %d M %d", (long long)L, w, a, M);
  if (!was || !rule) return;
  char msg[256];
  snprintf(msg, sizeof(msg), "ainp_spain_learned: bad argument (%s)", rule);
  CHECK(!strcmp(msg, was), "L %lld w %d a %d M %d: %s", (long long)L, w, a, M, msg);
}

int main() {
  static_assert(SP_WMIN == 8 && SP_WMAX == 4096 && SP_MMAX == 8192 && SP_NMAX_256 == 1024 &&
                    SP_NT_BIG == 512 && SP_EPL_BIG == 4 && AINP_SPAIN_OMP_DIMS == 512,
                "the window solvers' limits");
  static_assert(SL_MMIN == 8 && SL_MMAX == 2048 && SL_WMIN == 8 && SL_LMAX == 4194304,
                "the whole-signal solver's limits");
  CHECK(!strcmp(SP_SHAPE_RULE, "w a power of two, 8 <= w <= 4096, red 1, 2 or 4, red * w <= 8192"),
        "%s", SP_SHAPE_RULE);

  // ---- the window solvers: every w up to past the cap and a few far out
  int legal = 0;
  size_t largest = 0;
  for (int red = -1; red <= 9; ++red)
    for (int w = -2; w <= 8200; ++w) {
      ++g_cells;
      CHECK(sp_shape_ok(w, red) == old_shape_ok(w, red), "w %d red %d", w, red);
      if (!sp_shape_ok(w, red)) continue;
      ++legal;
      const int M = red * w, N = M / 2;
      CHECK(sp_lgN(M) == old_lgN(M) && (1 << sp_lgN(M)) == N, "lgN of M %d", M);
      const int nF = N + N / 32 + 2, nCos = (M / 4 + 2) & ~1;
      CHECK(nF == M / 2 + M / 64 + 2, "the two spellings at M %d", M);
      const SpLds f = sp_fft_lds(M), p = sp_window_lds(w, M, false), o = sp_window_lds(w, M, true);
      CHECK(f.nF == nF && f.nCos == nCos && f.nRow == 0 && f.nD == 0 && f.nA == 0 &&
                f.bytes() == ((size_t)2 * nF + nCos) * sizeof(double),
            "transform plan at M %d", M);
      CHECK(p.nF == nF && p.nCos == nCos && p.nRow == w && p.nD == 0 && p.nA == 0 &&
                p.bytes() == ((size_t)2 * nF + w + nCos) * sizeof(double),
            "window plan at w %d red %d", w, red);
      const int nD = std::min(w, 512), nA = nD / 2 + 2;
      CHECK(sp_omp_dims(w) == nD && o.nF == nF && o.nCos == nCos && o.nRow == w && o.nD == nD &&
                o.nA == nA &&
                o.bytes() == ((size_t)2 * nF + w + nCos + 4 * nD) * sizeof(double) +
                                 ((size_t)nD + 2 * nA) * sizeof(int),
            "OMP plan at w %d red %d", w, red);
      CHECK(p.bytes() + STATIC_SPAIN <= CU_LDS && o.bytes() + STATIC_OMP <= CU_LDS,
            "LDS at w %d red %d: %zu, %zu", w, red, p.bytes(), o.bytes());
      CHECK(p.bytes() <= sp_window_lds(SP_WMAX, SP_MMAX, false).bytes() &&
                o.bytes() <= sp_window_lds(SP_WMAX, SP_MMAX, true).bytes(),
            "the reserved plan covers w %d red %d", w, red);
      largest = std::max(largest, p.bytes());
      CHECK(sp_lanes_256(M) == (M / 2 <= 1024), "lanes at M %d", M);
      // a lane's slots cover the half spectrum and the sample pairs
      const int nt = sp_lanes_256(M) ? 256 : SP_NT_BIG, epl = sp_lanes_256(M) ? 2 : SP_EPL_BIG;
      CHECK(nt * epl >= N / 2 && 2 * nt * epl >= N, "slots at M %d", M);
    }
  for (int w : {-4096, 16384, 65536, 1 << 30, INT32_MAX, INT32_MIN})
    for (int red : {1, 2, 4, INT32_MAX}) {
      ++g_cells;
      CHECK(!sp_shape_ok(w, red) && !old_shape_ok(w, red), "w %d red %d", w, red);
    }
  CHECK(legal == 10 + 10 + 9, "%d legal (w, red)", legal);   // w = 8 .. 4096, 4 w <= 8192
  // spain.hip's table (67584 + 32768 + 16392) and what it rounds away: the two
  // spare doubles of re and of im, and the quarter wave evened to 2050 entries
  CHECK(largest == 67584 + 32768 + 16392 + 2 * 2 * 8 + 8 &&
            largest == sp_window_lds(SP_WMAX, SP_MMAX, false).bytes(),
        "largest window plan %zu", largest);

  // ---- the whole-signal solver: every M up to past the cap, w and a around
  // their limits, L around the multiples of M and the cap
  for (int M = -1; M <= 2050; ++M)
    for (int w : {0, 4, 7, 8, 12, 16, M / 2, M - 1, M, M + 1, 2 * M})
      for (int a : {-1, 0, 1, 3, w / 4, w / 2, w / 2 + 1, w})
        for (int64_t L : {(int64_t)-M, (int64_t)0, (int64_t)M - 1, (int64_t)M, (int64_t)M + 1,
                          (int64_t)3 * M, SL_LMAX - 1, SL_LMAX, SL_LMAX + 1, SL_LMAX + M,
                          2 * SL_LMAX})
          check_sl(L, w, a, M);
  for (int M : {4096, 8192, 1 << 30, INT32_MAX, INT32_MIN})
    check_sl(M, 8, 4, M);
  for (int M = SL_MMIN; M <= SL_MMAX; M *= 2) {
    ++g_cells;
    const SpLds f = sp_fft_lds(M);
    const int nF = M / 2 + M / 64 + 2, nCos = (M / 4 + 2) & ~1;
    CHECK(!sl_shape_rule(M, 8, 4, M) && f.nF == nF && f.nCos == nCos &&
              f.bytes() == ((size_t)2 * nF + nCos) * sizeof(double) &&
              sp_lgN(M) == old_lgN(M) && (2 << sp_lgN(M)) == M,
          "transform plan at M %d", M);
  }
  CHECK(sp_fft_lds(2048).bytes() == 16928 + 4112, "M 2048: %zu", sp_fft_lds(2048).bytes());

  if (g_fail) {
    fprintf(stderr, "spain_plan_check: %d failure(s) in %lld cells\n", g_fail, g_cells);
    return 1;
  }
  printf("spain_plan_check OK (%lld cells)\n", g_cells);
  return 0;
}
