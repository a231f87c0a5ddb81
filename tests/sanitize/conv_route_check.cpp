// conv_route_check — walks the 3x3 conv routing table (csrc/conv_route.h) on
// the host, built with ASan + UBSan (csrc/Makefile `sanitize`).  For every
// cell of channel pairs x shapes x flags / layouts / optional operands x
// routing environments, the accepted extremes included, it checks that the
// route refuses with a known message or names a kernel, that the grid fits
// `unsigned` and the row / slab counts fit `int` where the launchers cast
// them, that they stay within the stat_parts / workspace bounds, and that
// every host-only query answers what the route says.  Prints the kernels of
// the model's five convs; exits 0 with "conv_route_check OK".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../ml-audio-inpainting_amd/csrc/conv_route.h"

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

struct Shape { int64_t N, H, W; };
static const int PAIRS[][2] = {{1, 16}, {16, 32}, {32, 64}, {32, 16}, {16, 1}, {2, 16}, {16, 2},
                               {64, 32}, {16, 16}, {16, 64}, {64, 64}, {8, 24}, {3, 64}};
static const Shape GRID[] = {{1, 1, 1}, {2, 9, 49}, {4, 257, 334}, {32, 257, 334},
                             {2, 257, 1001}, {1, 23000, 23400}};
static const int64_t I31 = ((int64_t)1 << 31) - 1;
// what ainp_conv3x3_fwd_ex accepts at most; the data gradient bounds neither H nor W
static const Shape FWD_MAX[] = {{65535, 1 << 24, 1 << 24}};
static const Shape DGRAD_MAX[] = {{65535, I31, 7}, {65535, 7, I31}, {65535, I31, I31}};

static bool fits_unsigned(int64_t v) { return v >= 1 && v <= 0xffffffffLL; }

static void check_conv(const ConvEnv& env, const ConvCall& c) {
  ++g_cells;
  const ConvRoute r = route_conv(env, c);
  const char* k = conv_kernel_name(r.kernel);
  if (!r.ok()) {
    CHECK(r.kernel == CK_NONE, "refused with kernel %s", k);
    CHECK(r.refuse >= CR_NO16 && r.refuse <= CR_BNR_ARG && conv_refusal_text(r.refuse)[0],
          "refusal %d", (int)r.refuse);
    CHECK(r.refuse != CR_CFNT || (c.lay & CL_CF), "CFNT refusal without the layout");
    CHECK(r.refuse != CR_BNR_ARG || c.fused, "bnr refusal of a plain call");
    return;
  }
  CHECK(r.kernel > CK_NONE && r.kernel < CK_COUNT, "kernel %d", (int)r.kernel);
  CHECK(fits_unsigned(r.gx) && fits_unsigned(r.gy) && fits_unsigned(r.gz), "%s grid %lld %lld %lld",
        k, (long long)r.gx, (long long)r.gy, (long long)r.gz);
  CHECK(!r.two_pass || c.fused, "two passes of a plain call");
  CHECK(!(c.lay & CL_CF) || r.kernel == CK_X6Q, "[C][H][N][W] dx on %s", k);
  CHECK(!c.nodx || r.kernel == CK_ROWS_1TO16, "partials only on %s", k);
  // the row-strip kernels take their strip count as an int
  if (r.kernel == CK_ROWS_16TO1)
    CHECK(tiles(c.N, c.H, c.W, R1_RS, R1_TW) < LIM_OFF32, "strips");
  if (r.kernel == CK_ROWS_1TO16)
    CHECK(tiles(c.N, c.H, c.W, R16_RS, R16_TW) < LIM_OFF32, "strips");
  if (r.kernel == CK_FWD_B16DMA)
    CHECK(tiles(c.N, c.H, c.W, cdf::TR, cdf::TC) < LIM_OFF32, "tiles");
  if (!c.stats || r.two_pass) return;
  CHECK(r.rows >= 1 && r.rows <= r.rows_pad, "%s rows %lld of %lld", k, (long long)r.rows,
        (long long)r.rows_pad);
  if (c.fused) {
    // summed with an int row count out of ainp_conv3x3_dgrad_bnr_workspace
    CHECK(r.rows < LIM_OFF32 && r.rows == r.rows_pad, "%s fused rows %lld", k, (long long)r.rows);
    CHECK(r.rows <= dgrad_bnr_rows(c.N, c.H, c.W), "%s fused rows %lld > workspace rows %lld", k,
          (long long)r.rows, (long long)dgrad_bnr_rows(c.N, c.H, c.W));
  } else {
    // fp32: ainp_conv3x3_fwd_stat_parts; bf16: the persistent grids times
    // the occupancy multiplier may pass it
    int64_t bound = conv_stat_parts(c.N, c.H, c.W);
    if (c.b16 && bound < X6P_GRID2 * X6_OCC_MAX) bound = X6P_GRID2 * X6_OCC_MAX;
    CHECK(r.rows_pad <= bound, "%s rows %lld > bound %lld", k, (long long)r.rows_pad,
          (long long)bound);
  }
}

static void check_wgrad(const ConvEnv& env, const WgradCall& c) {
  ++g_cells;
  const WgradRoute r = route_wgrad(env, c);
  const char* k = wgrad_kernel_name(r.kernel);
  if (!r.ok()) {
    CHECK(r.kernel == WK_NONE, "refused with kernel %s", k);
    CHECK(r.refuse >= CR_W_ARG && r.refuse <= CR_W_TILES && conv_refusal_text(r.refuse)[0],
          "refusal %d", (int)r.refuse);
    return;
  }
  CHECK(r.kernel > WK_NONE && r.kernel < WK_COUNT, "kernel %d", (int)r.kernel);
  CHECK(fits_unsigned(r.gx) && fits_unsigned(r.gy) && fits_unsigned(r.gz), "%s grid", k);
  CHECK(r.slabs >= 1 && r.slabs < LIM_OFF32, "%s slabs %lld", k, (long long)r.slabs);
  CHECK(r.cp >= 1 && r.cp <= WG_CIMAX && c.ci0 + r.cp <= c.Cin, "%s pass %d", k, r.cp);
  // the slabs and the slab sum's first-stage buffer fit the workspace
  const int64_t ws = (int64_t)wgrad_workspace_bytes(c.N, c.Cin, c.Cout, c.H, c.W);
  int64_t need;
  if (r.kernel <= WK_SMALL_TILE) {
    const int nout = c.Cout * c.Cin * 9 + c.Cout;
    need = sat_mul(r.slabs, nout, 4) + (int64_t)SWG_GROUPS * nout * 8 + 16;
  } else {
    const int ct = wgrad_ct(c.Cout) == 3 ? 4 : wgrad_ct(c.Cout);
    const int64_t per = (int64_t)ct * 16 * (9 * r.cp + 1);
    need = (r.slabs + 2 * WG_GROUPS) * per * 4;
    CHECK(r.slabs % WG_GROUPS == 0, "%s slabs %lld", k, (long long)r.slabs);
  }
  CHECK(need <= ws, "%s needs %lld of %lld workspace bytes", k, (long long)need, (long long)ws);
}

static void check_queries(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H, int64_t W) {
  ++g_cells;
  for (int b16 = 0; b16 < 2; ++b16) {
    ConvCall f = conv_call(false, N, Cin, Cout, H, W, b16 ? AINP_CONV_BF16 : 0);
    f.stats = true;
    const ConvRoute r = route_conv(env, f);
    const int64_t want = r.ok() ? r.rows_pad : tiles(N, H, W, CV_FT, CV_TT);
    CHECK(query_stat_rows(env, N, Cin, Cout, H, W, b16 ? AINP_CONV_BF16 : 0) == want, "stat rows");
    // the fp32 rows are what ainp_conv3x3_fwd_stat_parts bounds
    CHECK(b16 || want <= conv_stat_parts(N, H, W), "stat rows %lld > parts", (long long)want);
  }
  auto wg = [&](int flags) { return wgrad_accepts(env, wgrad_call(N, Cin, Cout, H, W, flags)); };
  auto cv = [&](bool dgrad, int flags, bool stats = false) {
    ConvCall c = conv_call(dgrad, N, Cin, Cout, H, W, flags);
    c.stats = stats;
    return route_conv(env, c).ok();
  };
  const int B = AINP_CONV_BF16, IO = AINP_CONV_XCL | AINP_CONV_YCL;
  CHECK(query_dy16_ok(env, N, Cin, Cout, H, W) ==
            (wg(B | AINP_CONV_DY16) && cv(true, B | AINP_CONV_DY16)), "dy16_ok");
  CHECK(query_io16_ok(env, N, Cin, Cout, H, W) ==
            (wg(B | AINP_CONV_X16) && cv(false, B | AINP_CONV_X16 | AINP_CONV_Y16)), "io16_ok");
  const bool off32 = below(LIM_OFF32, H, W, Cin > Cout ? Cin : Cout, 4);
  CHECK(query_cl_ok(env, N, Cin, Cout, H, W) ==
            (!env.exact && off32 && cv(false, IO, true) && cv(true, IO) &&
             wg(AINP_CONV_XCL | AINP_CONV_GCL)), "cl_ok");
  CHECK(query_dgrad_cfnt_ok(env, N, Cin, Cout, H, W) == cv(true, AINP_CONV_YCFNT), "cfnt_ok");
  for (int dy16 = 0; dy16 < 2; ++dy16)
    for (int y16 = 0; y16 < 2; ++y16) {
      const int fl = AINP_CONV_YCL | (dy16 ? B | AINP_CONV_DY16 : 0), bf = y16 ? AINP_BN_Y16 : 0;
      const bool want = dgrad_bnr_args_ok(N, Cin, Cout, H, W, fl, bf) &&
                        route_conv(env, dgrad_bnr_call(N, Cin, Cout, H, W, fl, bf, true)).ok();
      CHECK(query_dgrad_bnr_nodx_ok(env, N, Cin, Cout, H, W, fl, bf) == want, "nodx_ok");
      // the partials-only form: Conv2d(16, 1) with fp32 dy on the row strips
      CHECK(!want || (Cin == 16 && Cout == 1 && !dy16 && env.small_rows && env.dgrad_bnr),
            "nodx_ok for %d -> %d", Cin, Cout);
    }
}

static void walk(const ConvEnv& env, int Cin, int Cout, const Shape& sh, bool fwd, bool dgrad,
                 bool wgrad) {
  const int64_t N = sh.N, H = sh.H, W = sh.W;
  // forward: arithmetic / storage x layouts x (stats, bias, prologue)
  for (int st = 0; fwd && st < 5; ++st)       // fp32, bf16, +x16, +y16, +x16+y16
    for (int lay = 0; lay < 4; ++lay)
      for (int opt = 0; opt < 8; ++opt) {
        ConvCall c;
        c.N = N; c.Cin = Cin; c.Cout = Cout; c.H = H; c.W = W;
        c.b16 = st > 0; c.x16 = st == 2 || st == 4; c.y16 = st >= 3;
        c.lay = lay;
        c.stats = opt & 1; c.bias = opt & 2; c.pro = opt & 4;
        check_conv(env, c);
      }
  // data gradient of nn.Conv2d(Cin, Cout): runs Cout -> Cin.  Plain, and the
  // fused reduce (stats, Bnr, Bnr::y16, partials only)
  static const int dlay[] = {0, CL_X, CL_Y, CL_X | CL_Y, CL_CF, CL_X | CL_CF};
  for (int st = 0; dgrad && st < 3; ++st)     // fp32, bf16, bf16 + dy16
    for (int lay : dlay)
      for (int fu = 0; fu < 5; ++fu) {        // plain; fused x (y16, nodx)
        ConvCall c;
        c.dgrad = true;
        c.N = N; c.Cin = Cout; c.Cout = Cin; c.H = H; c.W = W;
        c.b16 = st > 0; c.x16 = st == 2;
        c.lay = lay;
        if (fu) {
          if (!(lay & CL_Y)) continue;        // ainp_conv3x3_dgrad_bnr requires it
          c.stats = c.fused = true;
          c.bnr_y16 = (fu - 1) & 1;
          c.nodx = (fu - 1) & 2;
        }
        check_conv(env, c);
      }
  // weight gradient, every pass
  for (int st = 0; wgrad && st < 5; ++st)     // fp32, bf16, +g16, +x16, +g16+x16
    for (int lay : {0, CL_X, CL_G, CL_X | CL_G})
      for (int opt = 0; opt < 4; ++opt)
        for (int ncu : {256, 304, 8})
          for (int ci0 = 0; ci0 < Cin; ci0 += WG_CIMAX) {
            WgradCall c;
            c.N = N; c.Cin = Cin; c.Cout = Cout; c.H = H; c.W = W;
            c.b16 = st > 0; c.g16 = st == 2 || st == 4; c.x16 = st >= 3;
            c.lay = lay;
            c.bna = opt & 1; c.small_tile = opt & 2;
            c.ci0 = ci0; c.ncu = ncu;
            check_wgrad(env, c);
          }
}

static void print_model(const ConvEnv& env) {
  static const int model[][2] = {{1, 16}, {16, 32}, {32, 64}, {32, 16}, {16, 1}};
  const int64_t N = 32, H = 257, W = 334;
  for (int b16 = 0; b16 < 2; ++b16)
    for (auto& p : model) {
      const int Cin = p[0], Cout = p[1];
      // the bf16 configuration: bf16 channel-last source and output where the
      // pair takes them (the 1 <-> 16 convs stay fp32)
      const bool s16 = b16 && !small_pair(Cin, Cout);
      const int B = b16 ? AINP_CONV_BF16 : 0, IO = AINP_CONV_XCL | AINP_CONV_YCL;
      ConvCall f = conv_call(false, N, Cin, Cout, H, W,
                             B | IO | (s16 ? AINP_CONV_X16 | AINP_CONV_Y16 : 0));
      f.stats = Cout > 1;
      f.bias = true;
      const int df = B | IO | (s16 ? AINP_CONV_DY16 : 0);
      // into a BatchNorm+ReLU: the fused reduce (bf16 storage of its y likewise)
      const ConvRoute d = Cin >= 16 ? route_conv(env, dgrad_bnr_call(N, Cin, Cout, H, W, df,
                                                                      s16 ? AINP_BN_Y16 : 0, false))
                                    : route_conv(env, conv_call(true, N, Cin, Cout, H, W, df));
      const WgradRoute g = route_wgrad(
          env, wgrad_call(N, Cin, Cout, H, W, B | AINP_CONV_XCL | AINP_CONV_GCL |
                                                  (s16 ? AINP_CONV_DY16 | AINP_CONV_X16 : 0)));
      printf("model %s %d->%d fwd=%s dgrad=%s%s wgrad=%s\n", b16 ? "bf16" : "fp32", Cin, Cout,
             conv_kernel_name(route_conv(env, f).kernel), conv_kernel_name(d.kernel),
             d.two_pass ? "+reduce" : "", wgrad_kernel_name(g.kernel));
    }
}

int main() {
  std::vector<ConvEnv> envs;
  for (int bits = 0; bits < 128; ++bits)
    for (int occ : {1, 2, X6_OCC_MAX}) {
      ConvEnv e;
      e.exact = bits & 1; e.x6_tiled = bits & 2; e.small_rows = !(bits & 4);
      e.dgrad_bnr = !(bits & 8); e.conv16_dma = !(bits & 16); e.dgrad16_dma = !(bits & 32);
      e.wgrad16_dma = !(bits & 64);
      e.x6_occ16 = occ;
      envs.push_back(e);
    }
  for (const ConvEnv& env : envs)
    for (auto& p : PAIRS) {
      for (const Shape& sh : GRID) {
        walk(env, p[0], p[1], sh, true, true, true);
        check_queries(env, sh.N, p[0], p[1], sh.H, sh.W);
      }
      for (const Shape& sh : FWD_MAX) {
        walk(env, p[0], p[1], sh, true, true, true);
        check_queries(env, sh.N, p[0], p[1], sh.H, sh.W);
      }
      for (const Shape& sh : DGRAD_MAX) walk(env, p[0], p[1], sh, false, true, false);
    }
  // the environment reader's defaults are the struct's
  const ConvEnv d;
  print_model(d);
  if (g_fail) {
    fprintf(stderr, "conv_route_check: %d failures in %lld cells\n", g_fail, g_cells);
    return 1;
  }
  printf("conv_route_check OK (%lld cells, %zu environments)\n", g_cells, envs.size());
  return 0;
}
