// conv3x3_route_names — which kernel serves which call of the conv tests
// (host only; plain C++17 over csrc/conv_route.h, no HIP).
//
// Reads lines "envbits op N Cin Cout H W flags ci0" from stdin, with Cin /
// Cout of the nn.Conv2d and the ABI's flags (include/ainp.h):
//   op  fwd     ainp_conv3x3_fwd_ex with bias and statistics (flags & 1024:
//               with the in_scale / in_shift prologue)
//       dgrad   ainp_conv3x3_dgrad_ex
//       bnr     ainp_conv3x3_dgrad_bnr (AINP_BN_Y16 with AINP_CONV_DY16)
//       wgrad   the pass of ainp_conv3x3_wgrad_ex starting at channel ci0
//   envbits     1 AINP_CONV_EXACT=1, 2 AINP_CONV_X6_TILED, 4 AINP_SMALL_ROWS=0,
//               8 AINP_DGRAD_BNR=0, 16 AINP_CONV16_DMA=0, 32 AINP_DGRAD16_DMA=0,
//               64 AINP_WGRAD16_DMA=0, 128 / 256 AINP_X6_OCC16=2 / 4,
//               512 AINP_SMALL_WGRAD_TILE=1
// and prints, per line, "kernel refusal fast dg8 two_pass gx gy gz rows"
// (rows: BatchNorm partial rows, or the weight gradient's slabs; refusal: the
// ConvRefusal enumerator's value, 0 when served).
// tests/test_cpu_conv3x3_ref.py compiles and runs it.
#include <stdio.h>
#include <string.h>

#include "../ml-audio-inpainting_amd/csrc/conv_route.h"

using namespace ainp;

int main() {
  char op[16];
  long long N, H, W;
  int bits, Cin, Cout, flags, ci0;
  while (scanf("%d %15s %lld %d %d %lld %lld %d %d", &bits, op, &N, &Cin, &Cout, &H, &W, &flags,
               &ci0) == 9) {
    ConvEnv env;
    env.exact = bits & 1;
    env.x6_tiled = bits & 2;
    env.small_rows = !(bits & 4);
    env.dgrad_bnr = !(bits & 8);
    env.conv16_dma = !(bits & 16);
    env.dgrad16_dma = !(bits & 32);
    env.wgrad16_dma = !(bits & 64);
    env.x6_occ16 = (bits & 256) ? 4 : (bits & 128) ? 2 : 1;
    const bool pro = flags & 1024;
    flags &= ~1024;
    if (!strcmp(op, "wgrad")) {
      WgradCall c = wgrad_call(N, Cin, Cout, H, W, flags);
      c.small_tile = bits & 512;
      c.ci0 = ci0;
      const WgradRoute r = route_wgrad(env, c);
      printf("%s %d 0 0 0 %lld %lld %lld %lld\n", wgrad_kernel_name(r.kernel), (int)r.refuse,
             (long long)r.gx, (long long)r.gy, (long long)r.gz, (long long)r.slabs);
      continue;
    }
    ConvCall c;
    if (!strcmp(op, "bnr")) {
      c = dgrad_bnr_call(N, Cin, Cout, H, W, flags, (flags & AINP_CONV_DY16) ? AINP_BN_Y16 : 0,
                         false);
    } else {
      c = conv_call(!strcmp(op, "dgrad"), N, Cin, Cout, H, W, flags);
      if (!c.dgrad) {
        c.stats = c.bias = true;
        c.pro = pro;
      }
    }
    const ConvRoute r = route_conv(env, c);
    printf("%s %d %d %d %d %lld %lld %lld %lld\n", conv_kernel_name(r.kernel), (int)r.refuse,
           (int)r.fast, (int)r.dg8, (int)r.two_pass, (long long)r.gx, (long long)r.gy,
           (long long)r.gz, (long long)r.rows_pad);
  }
  return 0;
}
