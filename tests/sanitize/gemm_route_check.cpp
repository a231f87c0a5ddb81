// gemm_route_check — walks csrc/gemm_route.h on the host, built with ASan +
// UBSan (csrc/Makefile `sanitize`):
//  - splitk_covers against the launchers' former two-product expression over a
//    grid where that expression cannot overflow: equal everywhere;
//  - the extremes (kc = INT64_MAX, K = INT64_MAX, nsplit = 65535, non-positive
//    values), where the former expression overflowed: refused, no runtime error;
//  - route_gemm_bf16nt over a shape grid under both AINP_GEMM16_256 settings
//    and both K-tile depths, the layer-0 shapes of the C2 / C3 step included:
//    the tile is the former launcher condition's, the name is that tile's
//    kernel, and the layer-0 GEMMs get the kernels DESIGN section 4 names.
// Exits 0 with "gemm_route_check OK".
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../ml-audio-inpainting_amd/csrc/gemm_route.h"

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

// the rule as the five launchers wrote it (each behind nsplit in 1..65535)
static bool old_covers(int64_t K, int64_t nsplit, int64_t kc, int64_t g) {
  if (nsplit < 1 || nsplit > 65535) return false;
  return !(nsplit > 1 && (kc < g || kc % g || nsplit * kc < K || (nsplit - 1) * kc >= K));
}

// ainp_gemm_bf16nt's former condition (sizes small enough for its products)
static int old_tile(int64_t M, int64_t N, int64_t K, int64_t nsplit, int64_t kc, const GemmEnv& e) {
  const int64_t tiles128 = ((M + 127) / 128) * ((N + 127) / 128);
  if (e.gemm16_256 && (nsplit == 1 || M >= 8 * N) && M >= 512 && N >= 512 && tiles128 <= 1536 &&
      K % 32 == 0)
    return (e.g256_bk64 && K % 64 == 0 && kc % 64 == 0) ? AINP_GEMM_TILE_G256_BK64
                                                        : AINP_GEMM_TILE_G256;
  return AINP_GEMM_TILE_G16;
}

static const char* tile_kernel(int tile) {
  return tile == AINP_GEMM_TILE_G16    ? "g16::gemm_bf16nt_kernel"
         : tile == AINP_GEMM_TILE_G256 ? "g256::gemm_bf16nt_256_kernel"
                                       : "g256::gemm_bf16nt_256b_kernel";
}

int main() {
  static_assert(G16_BK == 64 && G256_BK == 32 && G256_BK64 == 64 && X6_256_BK == 16 &&
                    X6R_BK == 16, "K-tile depths");
  const int64_t GRAN[] = {16, 32, 64};
  // every K up to 700, every nsplit up to 20 and a few large ones, kc around
  // every multiple of the granule: products stay below 2^40
  const int64_t NSPLIT_BIG[] = {255, 4096, 65535, 65536, 70000};
  for (int64_t g : GRAN)
    for (int64_t K = 0; K <= 700; ++K)
      for (int64_t kc = -g; kc <= 720 + g; ++kc) {
        for (int64_t S = -1; S <= 20; ++S) {
          ++g_cells;
          CHECK(splitk_covers(K, S, kc, g) == old_covers(K, S, kc, g), "K %lld S %lld kc %lld g %lld",
                (long long)K, (long long)S, (long long)kc, (long long)g);
        }
        for (int64_t S : NSPLIT_BIG) {
          ++g_cells;
          CHECK(splitk_covers(K, S, kc, g) == old_covers(K, S, kc, g), "K %lld S %lld kc %lld g %lld",
                (long long)K, (long long)S, (long long)kc, (long long)g);
        }
      }
  // large K with exact covers, one chunk short and one chunk too many
  for (int64_t g : GRAN)
    for (int64_t K : {(int64_t)16448, (int64_t)10688, (int64_t)320512, ((int64_t)1 << 31) + 64})
      for (int64_t S : {2, 3, 16, 501, 65535}) {
        const int64_t kc = ((K + S - 1) / S + g - 1) / g * g;
        for (int64_t dS = -1; dS <= 1; ++dS)
          for (int64_t dk = -g; dk <= g; dk += g) {
            ++g_cells;
            CHECK(splitk_covers(K, S + dS, kc + dk, g) == old_covers(K, S + dS, kc + dk, g),
                  "K %lld S %lld kc %lld", (long long)K, (long long)(S + dS), (long long)(kc + dk));
          }
      }
  // the extremes: the former products overflow here; refused without one
  const int64_t BIG = INT64_MAX, BIG64 = INT64_MAX / 64 * 64;
  for (int64_t g : GRAN) {
    CHECK(!splitk_covers(BIG, 65535, BIG, g), "kc = K = INT64_MAX");
    CHECK(!splitk_covers(BIG, 65535, BIG64, g), "kc = largest multiple of 64");
    CHECK(!splitk_covers(1024, 65535, BIG64, g), "huge kc over a small K");
    CHECK(!splitk_covers(1024, 2, BIG64, g), "huge kc, two chunks");
    CHECK(!splitk_covers(BIG, 65535, g, g), "K = INT64_MAX in 65535 K-tiles");
    CHECK(!splitk_covers(BIG, 2, g, g), "K = INT64_MAX in two K-tiles");
    CHECK(splitk_covers(((int64_t)1 << 62) + 64, 2, (int64_t)1 << 62, g), "two chunks of 2^62");
    CHECK(!splitk_covers(BIG, 65536, BIG64, g) && !splitk_covers(BIG, INT64_MAX, g, g) &&
              !splitk_covers(BIG, 0, g, g) && !splitk_covers(BIG, INT64_MIN, g, g),
          "nsplit out of range");
    CHECK(!splitk_covers(1024, 2, 0, g) && !splitk_covers(1024, 2, INT64_MIN, g) &&
              !splitk_covers(INT64_MIN, 2, g, g) && !splitk_covers(0, 2, g, g),
          "non-positive kc / K");
    CHECK(splitk_covers(BIG, 1, BIG, g) && splitk_covers(0, 1, 0, g), "unsplit");
    g_cells += 14;
  }
  CHECK(splitk_granule(AINP_GEMM_FAMILY_G16, 200) == 64 &&
            splitk_granule(AINP_GEMM_FAMILY_G256, 128) == 64 &&
            splitk_granule(AINP_GEMM_FAMILY_G256, 96) == 32 &&
            splitk_granule(AINP_GEMM_FAMILY_X6, 112) == 16 && splitk_granule(7, 64) == 0,
        "granules");

  // ---- the bf16 tile route
  const int64_t MS[] = {1, 200, 511, 512, 520, 4095, 4096, 4104, 8191, 8192, 10688, 16448, 40000,
                        196608, 196609};
  const int64_t NS[] = {1, 136, 511, 512, 1024, 1025, 16448};
  const int64_t KS[] = {8, 40, 64, 72, 96, 128, 384, 1024, 10688, 16448};
  for (int on = 0; on < 2; ++on)
    for (int bk64 = 0; bk64 < 2; ++bk64) {
      GemmEnv env;
      env.gemm16_256 = on != 0;
      env.g256_bk64 = bk64 != 0;
      for (int64_t M : MS)
        for (int64_t N : NS)
          for (int64_t K : KS)
            for (int64_t S : {1, 2, 3, 16}) {
              const int64_t kc = S == 1 ? K : ((K + S - 1) / S + 63) / 64 * 64;
              const GemmBf16Route r = route_gemm_bf16nt(M, N, K, S, kc, env);
              ++g_cells;
              CHECK(r.tile == old_tile(M, N, K, S, kc, env), "M %lld N %lld K %lld S %lld: tile %d",
                    (long long)M, (long long)N, (long long)K, (long long)S, r.tile);
              CHECK(!strcmp(r.name, tile_kernel(r.tile)), "name %s of tile %d", r.name, r.tile);
              CHECK(on || r.tile == AINP_GEMM_TILE_G16, "GEMM16_256 off took tile %d", r.tile);
              CHECK(bk64 || r.tile != AINP_GEMM_TILE_G256_BK64, "G256_BK64 off took the b64 kernel");
            }
      // layer 0 of the C2 / C3 step (M = N*T = 10688, 8H = 1024, I = 16448):
      // the projection split 3 on g256 (the tall split GEMM),
      // the data gradient (10836 tiles) and the split weight gradient on g16
      const int64_t NT = 10688, G8 = 1024, I = 16448;
      const char* proj = route_gemm_bf16nt(NT, G8, I, 3, 5504, env).name;
      const char* proj1 = route_gemm_bf16nt(NT, G8, I, 1, I, env).name;
      const char* dx = route_gemm_bf16nt(NT, I, G8, 1, G8, env).name;
      const char* dw = route_gemm_bf16nt(G8, I, NT, 2, 5376, env).name;
      const char* want = !on ? "g16::gemm_bf16nt_kernel"
                             : bk64 ? "g256::gemm_bf16nt_256b_kernel" : "g256::gemm_bf16nt_256_kernel";
      CHECK(!strcmp(proj, want) && !strcmp(proj1, want), "layer-0 projection on %s / %s", proj, proj1);
      CHECK(!strcmp(dx, "g16::gemm_bf16nt_kernel") && !strcmp(dw, "g16::gemm_bf16nt_kernel"),
            "layer-0 gradients on %s / %s", dx, dw);
      printf("model gemm16_256=%d g256_bk64=%d proj=%s dx=%s dw=%s\n", on, bk64, proj, dx, dw);
    }
  // sizes whose tile count or 8N would overflow: g16, no runtime error
  GemmEnv env;
  CHECK(route_gemm_bf16nt(INT64_MAX, INT64_MAX, 64, 1, 64, env).tile == AINP_GEMM_TILE_G16 &&
            route_gemm_bf16nt(INT64_MAX, INT64_MAX, 64, 3, 64, env).tile == AINP_GEMM_TILE_G16 &&
            route_gemm_bf16nt(INT64_MAX, 512, 64, 3, 64, env).tile == AINP_GEMM_TILE_G16 &&
            route_gemm_bf16nt(0, 0, 0, 1, 0, env).tile == AINP_GEMM_TILE_G16,
        "oversized shapes");
  // the environment reader: defaults when nothing is set
  const GemmEnv d = GemmEnv();
  CHECK(!d.b16_kt64 && d.g256_bk64 && d.gemm16_256 && d.x6_splitpass && d.x6r_mfast && d.x6r_apf,
        "defaults");
  (void)gemm_env_read();

  if (g_fail) {
    fprintf(stderr, "gemm_route_check: %d failure(s) in %lld cells\n", g_fail, g_cells);
    return 1;
  }
  printf("gemm_route_check OK (%lld cells)\n", g_cells);
  return 0;
}
