// conv_gen_route_check — walks the routing table of the GAN's general
// convolution (csrc/conv_gen_route.h) on the host, built with ASan + UBSan
// (csrc/Makefile `sanitize`).  For every cell of channel pairs x kernels x
// strides x source sizes x shapes x (bf16, stats, y16, crop) x policies x
// routing environments, an oversized shape included, it checks that the route
// refuses with a known message or names a kernel whose grid is positive and
// within the launch limits, whose K splits cover every K tile with none
// empty, whose workspace holds the split-K partial sums, whose statistic rows
// are the kernel's pixel tiles, and that the host-only queries answer what
// the route says.  Exits 0 with "conv_gen_route_check OK".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../ml-audio-inpainting_amd/csrc/conv_gen_route.h"

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

struct Pair { int C0, C1, Cout; };
struct Shape { int64_t N, Ho, Wo; };
static const Pair PAIRS[] = {{1, 0, 16}, {3, 0, 64}, {4, 0, 64}, {5, 0, 64}, {2, 0, 64},
                             {64, 0, 1}, {33, 0, 1}, {64, 1, 64}, {32, 32, 48}, {64, 0, 96},
                             {128, 0, 70}, {256, 0, 130}, {512, 512, 512}, {512, 0, 260},
                             {33, 33, 200}};
static const int KERNELS[] = {3, 4, 5, 7};
static const Shape GRID[] = {{1, 1, 1}, {2, 9, 11}, {8, 256, 256}, {16, 4096, 4096}};
// no launch can serve it: every product saturates
static const Shape OVERSIZED = {65535, (int64_t)1 << 24, (int64_t)1 << 24};

static void check_route(const ConvGenEnv& env, const ConvGenPolicy& pol, const ConvGenCall& c) {
  ++g_cells;
  const ConvGenRoute r = route_conv_gen(env, pol, c);
  const char* k = conv_gen_kernel_id(r.kernel);
  const int64_t NP = sat_mul(c.N, c.Ho, c.Wo), KK = (int64_t)c.KH * c.KW;
  const int Cin = c.C0 + c.C1;
  CHECK(r.stat_rows >= 1 && r.workspace >= 0, "rows %lld workspace %lld", (long long)r.stat_rows,
        (long long)r.workspace);
  if (!r.ok()) {
    CHECK(r.kernel == CGK_NONE, "refused with kernel %s", k);
    CHECK(r.refuse > CGR_OK && r.refuse < CGR_COUNT && r.refuse != CGR_Y16 &&
              conv_gen_refusal_text(r.refuse)[0], "refusal %d", (int)r.refuse);
    CHECK(r.refuse != CGR_COUT1 || c.Cout == 1, "Cout = 1 refusal of Cout %d", c.Cout);
    CHECK(r.refuse != CGR_CROP || (c.Cout > 1 && (c.crop_h > 0 || c.crop_w > 0)), "crop refusal");
    CHECK(r.refuse != CGR_SIZE || NP >= LIM_OFF32 / 256 || c.Cout > 65535, "size refusal of %lld",
          (long long)NP);
    return;
  }
  CHECK(NP < INT64_MAX, "accepted a saturated shape");
  CHECK(r.kernel > CGK_NONE && r.kernel < CGK_COUNT && conv_gen_kernel_name(r)[0], "kernel %d",
        (int)r.kernel);
  // launch limits: x < 2^31, y and z < 2^16
  CHECK(r.gx >= 1 && r.gx <= INT_MAX && r.gy >= 1 && r.gy <= 65535 && r.gz >= 1 && r.gz <= 65535,
        "%s grid %lld %lld %lld", k, (long long)r.gx, (long long)r.gy, (long long)r.gz);
  if (r.epilogue != CGP_NONE)
    CHECK(r.ex >= 1 && r.ex <= INT_MAX && r.ey >= 1 && r.ey <= 65535, "%s epilogue grid", k);
  // the entry and the kernel belong together
  const bool n16 = r.kernel >= CGK_NHWC16_TILES;
  CHECK((r.entry == CGE_NHWC16) == n16, "%s on entry %d", k, (int)r.entry);
  CHECK(!n16 || (pol.nhwc16 && c.b16 && c.Cout > 1), "%s for a call off the channel-last path", k);
  CHECK(r.expand == (n16 && (c.C0 % 32 || c.C1 % 32)), "%s expand", k);
  if (c.Cout == 1) {
    CHECK(r.kernel == CGK_COUT1_LOOP || r.kernel == CGK_COUT1_TAPS, "Cout = 1 on %s", k);
    CHECK(r.epilogue == CGP_COUT1_FINISH && r.nsplit == 1 && !c.stats, "Cout = 1 epilogue");
    const int64_t np = c.N * (c.crop_h > 0 ? c.crop_h : c.Ho) * (c.crop_w > 0 ? c.crop_w : c.Wo);
    CHECK(r.workspace == ceil_div(Cin, C1_CC) * np * 4 && r.gx == ceil_div(np, 256) &&
              r.gy == ceil_div(Cin, C1_CC), "Cout = 1 workspace / grid");
    CHECK(r.kernel != CGK_COUT1_TAPS ||
              (env.cout1_taps && (r.kt == 3 || r.kt == 4) && r.kt == c.KH && c.KH == c.KW &&
               c.C1 == 0 && c.up0 == 0 && Cin % C1_CC == 0), "batched taps");
    CHECK(r.y16 == CGY_NOBODY, "Cout = 1 y16");
    return;
  }
  if (r.kernel == CGK_SMALLCIN) {
    // what the kernel's LDS holds
    CHECK(env.smallcin && c.C1 == 0 && c.up0 == 0 && !c.stats && c.Cout <= SC_CO &&
              c.C0 * KK <= SC_K && c.C0 <= SC_CIN, "few-input-channel kernel for %d x %lld -> %d",
          c.C0, (long long)KK, c.Cout);
    CHECK(r.nsplit == 1 && r.workspace == 0 && r.epilogue == CGP_NONE && r.gx == ceil_div(NP, 256),
          "few-input-channel launch");
    CHECK(r.y16 == CGY_NOBODY || (r.y16 == CGY_KERNEL && c.y16 && c.Cout % 8 == 0 && pol.out16 &&
                                  pol.out16_direct), "few-input-channel y16");
    CHECK(!r.lds16 || r.y16 == CGY_KERNEL, "lds16 without y16");
    return;
  }
  // the implicit GEMM: tiles, K splits, workspace, statistic rows
  const int BM = conv_gen_bm(c.Cout);
  const int64_t nkt = n16 ? (nhwc16_seg(c.C0, (int)KK) + nhwc16_seg(c.C1, (int)KK)) / CG_BK
                          : ceil_div((int64_t)Cin * KK, CG_BK);
  CHECK(r.nsplit >= 1 && r.nsplit <= nkt, "%s nsplit %d of %lld tiles", k, r.nsplit,
        (long long)nkt);
  if (r.nsplit > 1) {
    CHECK((int64_t)r.nsplit * r.ktiles_per_split >= nkt, "%s: %d x %d K tiles < %lld", k, r.nsplit,
          r.ktiles_per_split, (long long)nkt);
    CHECK((int64_t)(r.nsplit - 1) * r.ktiles_per_split < nkt, "%s: empty split (%d x %d, %lld)", k,
          r.nsplit, r.ktiles_per_split, (long long)nkt);
    CHECK(r.workspace >= (int64_t)r.nsplit * c.Cout * NP * 4, "%s workspace %lld", k,
          (long long)r.workspace);
    CHECK(r.epilogue == (env.splitk_tile ? CGP_SPLITK_TILE : CGP_SPLITK), "%s epilogue", k);
    CHECK(r.stat_rows == ceil_div(NP, env.splitk_tile ? SKT_P : 256) && r.stat_rows == r.ex,
          "%s split rows %lld", k, (long long)r.stat_rows);
  } else {
    CHECK(r.ktiles_per_split >= nkt && r.workspace == 0 && r.epilogue == CGP_NONE, "%s unsplit", k);
    CHECK(r.stat_rows == ceil_div(NP, CG_TILE / BM), "%s rows %lld", k, (long long)r.stat_rows);
  }
  if (r.kernel == CGK_NHWC16_WIDE) {
    CHECK((r.bm == 256 || r.bm == 128 || r.bm == 64) && (r.nw == 4 || (r.nw == 8 && r.bm > 64)) &&
              r.gx == r.tco * r.tpx && r.gy == r.nsplit && r.gz == 1 &&
              r.tco == ceil_div(c.Cout, r.bm) && r.tpx == ceil_div(NP, r.bm == 256 ? 128 : 256),
          "wide tiles");
    // its statistic slots are the BM-channel kernels' pixel tiles (128 or 256
    // pixels): whole slots per wide tile, none past the rows counted above
    const int span = r.bm == 256 ? 128 : 256, slot = CG_TILE / BM;
    CHECK(span % slot == 0 && (r.nsplit > 1 || ceil_div(NP, slot) == r.stat_rows), "wide rows");
  } else {
    CHECK(r.bm == BM && r.gx == ceil_div(NP, CG_TILE / BM) && r.gy == ceil_div(c.Cout, BM) &&
              r.gz == r.nsplit, "%s tiles", k);
    CHECK(r.nsplit > 1 || r.stat_rows == r.gx, "%s rows are not its pixel tiles", k);
  }
  if (r.kernel == CGK_X6)
    CHECK(c.b16 ? (r.planes == 1 && (r.bk == 16 || r.bk == 32 || r.bk == 64) &&
                   (r.bk != 64 || r.nsplit == 1 || r.ktiles_per_split % 2 == 0))
                : (r.planes == 3 && !env.exact && (r.bk == 16 || r.bk == 32)), "x6 loop");
  if (r.kernel == CGK_EXACT) CHECK(env.exact && !c.b16, "exact loop");
  if (n16)
    CHECK(r.y16 == (!(c.y16 && pol.out16) ? CGY_NOBODY : r.nsplit == 1 ? CGY_KERNEL
                    : env.splitk_tile ? CGY_TILE_EPILOGUE : CGY_TRANSPOSE), "%s y16", k);
  else
    CHECK(r.y16 == CGY_NOBODY, "%s y16", k);
  // the queries know channels, kernel and output size only
  const ConvGenRoute q = query_conv_gen(env, c.N, Cin, c.KH, c.KW, c.Cout, c.Ho, c.Wo, true);
  CHECK(q.stat_rows == r.stat_rows && q.workspace == r.workspace && q.nsplit == r.nsplit,
        "%s: the queries answer %lld rows, %lld bytes", k, (long long)q.stat_rows,
        (long long)q.workspace);
}

static void walk(const ConvGenEnv& env, const ConvGenPolicy& pol, const Pair& p, int k, int stride,
                 const Shape& sh) {
  const int pad = (k - 1) / 2;
  for (int up0 : {0, 1})
    for (int opt = 0; opt < 16; ++opt) {
      ConvGenCall c;
      c.N = sh.N; c.C0 = p.C0; c.C1 = p.C1; c.Cout = p.Cout;
      c.up0 = up0;
      c.Ho = sh.Ho; c.Wo = sh.Wo;
      c.Hin = sat_mul(sh.Ho - 1, stride) + k - 2 * pad;
      c.Win = sat_mul(sh.Wo - 1, stride) + k - 2 * pad;
      c.KH = c.KW = k;
      c.b16 = opt & 1; c.stats = opt & 2; c.y16 = opt & 4;
      if (opt & 8) {
        c.crop_h = sh.Ho > 1 ? (int)(sh.Ho < 1000 ? sh.Ho - 1 : 999) : 1;
        c.crop_w = 1;
      }
      check_route(env, pol, c);
    }
}

int main() {
  std::vector<ConvGenEnv> envs;
  // the switches of the NCHW entry's kernels, then those of the channel-last
  // entry's; each with the ones both share
  for (int sw : {0, 512, 768})
    for (int bits = 0; bits < 32; ++bits) {
      ConvGenEnv e;
      e.split_wide = sw;
      e.splitk_tile = !(bits & 1); e.smallcin = !(bits & 2);
      e.cout1_taps = !(bits & 4); e.smallcin_lds16 = !(bits & 8); e.exact = bits & 16;
      envs.push_back(e);
      if (bits >= 16) continue;
      for (int variant = 0; variant < 4; ++variant) {
        e = ConvGenEnv();
        e.split_wide = sw;
        e.splitk_tile = !(bits & 1); e.smallcin = !(bits & 2);
        e.conv16_small_wide = bits & 4; e.wide_pf = !(bits & 8);
        e.conv16_variant = variant;
        envs.push_back(e);
      }
    }
  // the K-tile depths change no grid: walked once each with the default rest
  for (int xbk : {16, 32})
    for (int bbk : {16, 32, 64}) {
      ConvGenEnv e;
      e.x6_bk = xbk; e.b16_bk = bbk;
      envs.push_back(e);
    }
  std::vector<ConvGenPolicy> pols;
  for (int n16 = 0; n16 < 2; ++n16)
    for (int small = 0; small < 3; ++small)
      for (int o = 0; o < 3; ++o) {
        ConvGenPolicy p;
        p.nhwc16 = n16; p.nhwc16_small = small; p.out16 = o > 0; p.out16_direct = o > 1;
        pols.push_back(p);
      }
  for (const ConvGenEnv& env : envs)
    for (const ConvGenPolicy& pol : pols)
      for (const Pair& p : PAIRS)
        for (int k : KERNELS)
          for (int stride : {1, 2}) {
            for (const Shape& sh : GRID) walk(env, pol, p, k, stride, sh);
            walk(env, pol, p, k, stride, OVERSIZED);
          }
  // the oversized shape: refused, with saturated (not wrapped) sizes
  {
    ConvGenCall c;
    c.N = OVERSIZED.N; c.C0 = 512; c.Cout = 512; c.KH = c.KW = 3;
    c.Hin = c.Ho = OVERSIZED.Ho; c.Win = c.Wo = OVERSIZED.Wo;
    const ConvGenRoute r = route_conv_gen(ConvGenEnv(), ConvGenPolicy(), c);
    CHECK(!r.ok() && r.refuse == CGR_SIZE && r.stat_rows > LIM_OFF32, "oversized shape");
    c.Cout = 1;
    const ConvGenRoute r1 = route_conv_gen(ConvGenEnv(), ConvGenPolicy(), c);
    CHECK(!r1.ok() && r1.workspace == INT64_MAX, "oversized Cout = 1 workspace saturates");
  }
  // the launchers' own policies name their entry for every call
  for (const Pair& p : PAIRS) {
    ConvGenCall c;
    c.N = 2; c.C0 = p.C0; c.C1 = p.C1; c.Cout = p.Cout; c.KH = c.KW = 3;
    c.Hin = c.Ho = 9; c.Win = c.Wo = 11;
    c.b16 = true;
    CHECK(route_conv_gen(ConvGenEnv(), conv_gen_policy_nchw(), c).entry == CGE_NCHW, "NCHW policy");
    if (p.Cout > 1)
      CHECK(route_conv_gen(ConvGenEnv(), conv_gen_policy_nhwc16(), c).entry == CGE_NHWC16,
            "channel-last policy");
  }
  if (g_fail) {
    fprintf(stderr, "conv_gen_route_check: %d failures in %lld cells\n", g_fail, g_cells);
    return 1;
  }
  printf("conv_gen_route_check OK (%lld cells, %zu environments, %zu policies)\n", g_cells,
         envs.size(), pols.size());
  return 0;
}
