// gemm_route.h — what the GEMM launchers (gemm.hip, gemm16.hip, gemm_x6r.hip)
// decide on the host: K-tile depths, the split-K cover rule, the A/B
// environment and the tile ainp_gemm_bf16nt takes.  Plain C++17, no HIP:
// ainp_gemm_splitk_granule and ainp_gemm_bf16nt_tile (capi.cpp) answer ainp.ops
// from the same functions, and tests/sanitize/gemm_route_check.cpp walks them
// under ASan + UBSan without a GPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/ainp.h"

namespace ainp {

// K-tile depths (the kernels' namespaces alias these; a split-K chunk is whole K-tiles)
constexpr int G16_BM = 128, G16_BN = 128, G16_BK = 64;   // bf16 128 x 128 tile (g16)
constexpr int G256_BK = 32;        // bf16 256 x 256 LDS-DMA tile: 4-stage ring
constexpr int G256_BK64 = 64;      //   its 64-deep 2-stage variant (b64)
constexpr int X6_256_BK = 16;      // fp32 (three bf16 pieces) 256 x 256 tile
constexpr int X6R_BK = 16;         // the split-plane tile

// nsplit chunks of kc, kc whole K-tiles of `granule`, cover K with no empty
// chunk.  No product of caller-supplied values: for kc > 0,
// nsplit*kc >= K && (nsplit-1)*kc < K is nsplit == ceil(K / kc).
inline bool splitk_covers(int64_t K, int64_t nsplit, int64_t kc, int64_t granule) {
  if (nsplit == 1) return true;
  return nsplit > 1 && nsplit <= 65535 && kc >= granule && kc % granule == 0 &&
         nsplit == K / kc + (K % kc != 0);
}

// chunk granule of a family (AINP_GEMM_FAMILY_*); g256: 64-deep K-tiles where K
// allows (the b64 kernel needs 64 | K and 64 | kc)
inline int splitk_granule(int family, int64_t K) {
  if (family == AINP_GEMM_FAMILY_G16) return G16_BK;
  if (family == AINP_GEMM_FAMILY_G256) return K % G256_BK64 == 0 ? G256_BK64 : G256_BK;
  return family == AINP_GEMM_FAMILY_X6 ? X6R_BK : 0;
}

// The A/B switches, read once per process (gemm_env()); the route takes them
// as an argument so a host program can try any setting.
struct GemmEnv {
  bool b16_kt64 = false;     // AINP_GEMM_B16_KT=64: ainp_gemm_f32_ex's bf16 loop on 64-deep K-tiles
  bool g256_bk64 = true;     // AINP_G256_BK64=0: the 32-deep 4-stage ring for every g256 GEMM
  bool gemm16_256 = true;    // AINP_GEMM16_256=0 keeps every ainp_gemm_bf16nt on g16
  bool x6_splitpass = true;  // AINP_X6_SPLITPASS=0 keeps the per-fragment-split x6_256 kernel
  bool x6r_mfast = true;     // AINP_X6R_MFAST=0: n-first tile order everywhere
  bool x6r_apf = true;       // AINP_X6R_APF=0: A fragments read right before their MFMA group,
                             //   the split skipped past the last tile (the round-4 main loop)
};
inline GemmEnv gemm_env_read() {
  auto first = [](const char* name) {
    const char* e = getenv(name);
    return e ? e[0] : '\0';
  };
  GemmEnv v;
  v.b16_kt64 = first("AINP_GEMM_B16_KT") == '6';
  v.g256_bk64 = first("AINP_G256_BK64") != '0';
  v.gemm16_256 = first("AINP_GEMM16_256") != '0';
  v.x6_splitpass = first("AINP_X6_SPLITPASS") != '0';
  v.x6r_mfast = first("AINP_X6R_MFAST") != '0';
  v.x6r_apf = first("AINP_X6R_APF") != '0';
  return v;
}
inline const GemmEnv& gemm_env() {
  static const GemmEnv v = gemm_env_read();
  return v;
}

struct GemmBf16Route {
  int tile;           // AINP_GEMM_TILE_*
  const char* name;   // the profiler's kernel name
};
// ainp_gemm_bf16nt: the 256 x 256 tile (one workgroup per CU, 128 KB of LDS;
// bit-identical to g16: same MFMA, same k order) only for unsplit GEMMs whose
// 128 x 128 grid is at most two rounds of its 768 resident slots -- the layer-0
// projection (672 tiles): 522 -> 482 us inside the step.  Measured inside the
// step it loses where another GEMM runs beside it on the side stream: the data
// gradient (10836 tiles) 706 -> 891 us, the split-K weight gradient
// 621 -> 1325 us (it cannot co-reside with the 3-workgroups-per-CU kernel
// next to it).  A split tall-and-narrow GEMM (M >= 8N: the layer-0 projection,
// 168 tiles of 256 x 256 -> 504 workgroups at split 3) also runs on g256.
// kc: the chunk as launched (K when nsplit == 1).
inline GemmBf16Route route_gemm_bf16nt(int64_t M, int64_t N, int64_t K, int64_t nsplit, int64_t kc,
                                       const GemmEnv& env) {
  auto tiles = [](int64_t n, int64_t t) { return n / t + (n % t != 0); };
  // at most 1536 tiles of 128 x 128, by division: no product of caller-supplied sizes
  const bool fits = M >= 512 && N >= 512 && tiles(M, G16_BM) <= 1536 / tiles(N, G16_BN);
  const bool tall = N <= INT64_MAX / 8 && M >= 8 * N;
  if (env.gemm16_256 && (nsplit == 1 || tall) && fits && K % G256_BK == 0) {
    if (env.g256_bk64 && K % G256_BK64 == 0 && kc % G256_BK64 == 0)
      return {AINP_GEMM_TILE_G256_BK64, "g256::gemm_bf16nt_256b_kernel"};
    return {AINP_GEMM_TILE_G256, "g256::gemm_bf16nt_256_kernel"};
  }
  return {AINP_GEMM_TILE_G16, "g16::gemm_bf16nt_kernel"};
}

}  // namespace ainp
