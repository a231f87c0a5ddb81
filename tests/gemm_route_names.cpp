// gemm_route_names — csrc/gemm_route.h asked on the host, for
// tests/test_cpu_gemm_ref.py: one line "bits M N K nsplit kc granule" in, one
// line "tile kernel covers" out.  bits: which GemmEnv field differs from its
// default, in the order of the struct (gemm_ref.ENV_FIELDS).
#include <cstdio>

#include "../ml-audio-inpainting_amd/csrc/gemm_route.h"

int main() {
  long long bits, M, N, K, nsplit, kc, granule;
  while (scanf("%lld %lld %lld %lld %lld %lld %lld", &bits, &M, &N, &K, &nsplit, &kc, &granule) == 7) {
    ainp::GemmEnv env;
    if (bits & 1) env.b16_kt64 = !env.b16_kt64;
    if (bits & 2) env.g256_bk64 = !env.g256_bk64;
    if (bits & 4) env.gemm16_256 = !env.gemm16_256;
    if (bits & 8) env.x6_splitpass = !env.x6_splitpass;
    if (bits & 16) env.x6r_mfast = !env.x6r_mfast;
    if (bits & 32) env.x6r_apf = !env.x6r_apf;
    const ainp::GemmBf16Route r =
        ainp::route_gemm_bf16nt(M, N, K, nsplit, nsplit == 1 ? K : kc, env);
    const char* name = r.name;
    for (const char* p = r.name; *p; ++p)
      if (*p == ':') name = p + 1;
    printf("%d %s %d\n", r.tile, name, ainp::splitk_covers(K, nsplit, kc, granule) ? 1 : 0);
  }
  return 0;
}
