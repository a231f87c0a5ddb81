// conv_gen_route.h — which kernel serves which call of the GAN's general
// convolution (ainp_conv_gen_fwd* / ainp_conv_gen_fwd_nhwc16*), host only.
//
// Plain C++17, no HIP: the two launchers of gan.hip call route_conv_gen once
// and switch on the kernel id; ainp_conv_gen_stat_parts / _workspace / _plan
// are the same function's answer, and ops.conv_gen (Python) takes entry point,
// workspace, statistic rows, kernel name and "may I pass y16" from that plan.
// tests/sanitize/conv_gen_route_check.cpp walks the table under ASan + UBSan
// without a GPU.
//
// Size arithmetic saturates (conv_route.h: sat_mul / ceil_div / below).
#pragma once
#include <limits.h>

#include "conv_route.h"

// nhwc16_seg is also called by the kernels
#ifdef __HIP__
#define AINP_HOST_DEVICE __host__ __device__
#else
#define AINP_HOST_DEVICE
#endif

namespace ainp {

// ---------------------------------------------------------------- tilings
constexpr int CG_BK = 32;                 // K tile of the implicit GEMM
constexpr int CG_TILE = 16384;            // outputs per tile: BM channels x CG_TILE / BM pixels
constexpr int SC_K = 160, SC_CO = 64;     // few-input-channel kernel: 40 KB of weights in LDS
constexpr int SC_CIN = 4;                 //   and at most 4 input channels
constexpr int C1_CC = 32;                 // Cout = 1: input channels per chunk
constexpr int C1_KMAX = 64;               // Cout = 1: taps (kernel <= 8 x 8)
constexpr int SKT_P = 64, SKT_C = 64;     // tiled split-K epilogue: pixels x channels
constexpr int IMN_P = 64, IMN_LDS = 4096, IMN_SEG = 256;   // im2col_nhwc16 rows kernel
constexpr int conv_gen_bm(int Cout) { return Cout > 64 ? 128 : 64; }

// k-values one source contributes to the nhwc16 weight rows: whole 32-deep
// tiles (zero weights in the pad) unless its channels are a multiple of 32
AINP_HOST_DEVICE inline int nhwc16_seg(int C, int KK) {
  return (C & 31) ? (KK * C + 31) / 32 * 32 : KK * C;
}

// how a source of Hs x Ws feeds a conv over Hin x Win: 0 same size, 1 exact
// nearest x2, 2 nearest resampling
inline int conv_gen_src_up(int Hs, int Ws, int Hin, int Win) {
  if (Hs == Hin && Ws == Win) return 0;
  return (2 * (int64_t)Hs == Hin && 2 * (int64_t)Ws == Win) ? 1 : 2;
}
inline int64_t conv_gen_out(int64_t in, int k, int stride, int pad) {
  return (in + 2 * (int64_t)pad - k) / stride + 1;
}

// ---------------------------------------------------------------- environment
// Read once per process (conv_gen_env()); route_conv_gen takes it as an
// argument so a test can pass any setting.
struct ConvGenEnv {
  int split_wide = 512;        // split-K target of the wide tiles (0: the old-tile count)
  bool splitk_tile = true;     // tiled split-K epilogue
  bool cout1_taps = true;      // Cout = 1: batched-tap kernel
  bool smallcin = true;        // few-input-channel direct kernel
  bool smallcin_lds16 = true;  //   its bf16 copy staged through LDS
  bool exact = false;          // exact f32 MFMA main loop, no split-bf16
  int x6_bk = 16;              // K-tile depth of the 3-plane split-bf16 loop
  int b16_bk = 32;             // K-tile depth of the 1-plane bf16 loop
  int conv16_variant = 3;      // nhwc16 main loop (ainp_conv16_set_variant overwrites it)
  bool conv16_small_wide = false;   // Cout <= 64 on the wide ring under variant 3
  bool wide_pf = true;         // 8-wave wide ring: prefetch
  bool im2col_rows = true;     // ainp_im2col_nhwc16: row-staged kernel
  bool pconv_mask_unroll = true;    // ainp_pconv_mask: unrolled square kernels
};

inline ConvGenEnv conv_gen_env_read() {
  auto first = [](const char* name) {
    const char* e = getenv(name);
    return e ? e[0] : '\0';
  };
  ConvGenEnv v;
  // =0: the old-tile workgroup count for every Cout; =3: ~768 workgroups
  const char sw = first("AINP_CONV_SPLIT_WIDE");
  v.split_wide = sw == '0' ? 0 : sw == '3' ? 768 : 512;
  v.splitk_tile = first("AINP_SPLITK_TILE") != '0';      // =0: per-channel epilogue blocks
  v.cout1_taps = first("AINP_COUT1_B") != '0';           // =0: the loop kernel (A/B)
  v.smallcin = first("AINP_CONV_SMALLCIN") != '0';
  v.smallcin_lds16 = first("AINP_SMALLCIN_LDS16") != '0';   // =0: each thread stores its own row
  v.exact = conv_env().exact;   // AINP_CONV_EXACT: conv_route.h reads it, for both tables
  v.x6_bk = first("AINP_CONV_GEN_BK") == '3' ? 32 : 16;
  // bf16 operands: 32-deep K tiles (64-deep tiles at 184-212 VGPRs ran the C4
  // step's convs 1.6x slower); = 16 / 64 selects the other depths
  const char bb = first("AINP_CONV_GEN_B16_BK");
  v.b16_bk = bb == '6' ? 64 : bb == '1' ? 16 : 32;
  // 0 register-staged, 1 LDS-DMA ring, 2 wide-tile ring of 4 waves, 3 (default)
  // wide-tile ring of 8 waves for Cout > 64 and the register-staged kernel below
  const char cv = first("AINP_CONV16");
  v.conv16_variant = (cv >= '0' && cv <= '3') ? cv - '0' : first("AINP_CONV16_RING") == '1' ? 1 : 3;
  v.conv16_small_wide = first("AINP_CONV16_SMALLCO") == '2';   // (A/B)
  v.wide_pf = first("AINP_WIDE_PF") != '0';
  v.im2col_rows = first("AINP_IM2COL_NHWC16_ROWS") != '0';     // =0: the per-chunk kernel
  v.pconv_mask_unroll = first("AINP_PCONV_MASK_UNROLL") != '0';   // =0: the loop kernel (A/B)
  return v;
}
inline ConvGenEnv& conv_gen_env() {
  static ConvGenEnv v = conv_gen_env_read();
  return v;
}

// The caller's switches (module attributes of ainp.ops, which tests patch):
// they choose between routes that all exist, so they are arguments, not
// environment.  The launchers pass the policy that names their own entry.
struct ConvGenPolicy {
  bool nhwc16 = true;         // bf16 convs run on channel-last bf16 operands
  int nhwc16_small = 1;       // sources with C % 32 != 0 there: 0 never, 1 unless the
                              // few-input-channel kernel serves the conv, 2 always
  bool out16 = true;          // a conv may write y's bf16 channel-last copy
  bool out16_direct = true;   //   the few-input-channel kernel too
};
inline ConvGenPolicy conv_gen_policy_nchw() {
  ConvGenPolicy p;
  p.nhwc16 = false;
  return p;
}
inline ConvGenPolicy conv_gen_policy_nhwc16() {
  ConvGenPolicy p;
  p.nhwc16_small = 2;
  return p;
}

// ---------------------------------------------------------------- a call, its route
struct ConvGenCall {
  int64_t N = 0;
  int C0 = 0, C1 = 0;        // channels of the two sources (C1 = 0: one source)
  int up0 = 0, up1 = 0;      // conv_gen_src_up of each
  int64_t Hin = 0, Win = 0, Ho = 0, Wo = 0;
  int KH = 0, KW = 0, Cout = 0;
  int crop_h = 0, crop_w = 0;
  bool b16 = false;          // AINP_CONV_BF16 arithmetic
  bool stats = false;        // BatchNorm partials wanted
  bool y16 = false;          // the bf16 channel-last copy of y wanted
};

enum ConvGenEntry { CGE_NCHW = 0, CGE_NHWC16 = 1 };   // fp32 NCHW / bf16 channel-last operands
enum ConvGenKernel {
  CGK_NONE = 0,
  CGK_COUT1_LOOP,     // conv_cout1_partial_kernel
  CGK_COUT1_TAPS,     // conv_cout1_partial_b_kernel<kt, 4>
  CGK_SMALLCIN,       // conv_gen_smallcin_kernel<b16, lds16>
  CGK_X6,             // conv_gen_x6_kernel<bm, bk, planes>
  CGK_EXACT,          // conv_gen_fwd_kernel<bm>
  CGK_NHWC16_TILES,   // conv_gen_nhwc16_kernel<bm, expand>
  CGK_NHWC16_RING,    // conv_gen_nhwc16_ring_kernel<bm, expand>
  CGK_NHWC16_WIDE,    // conv_gen_nhwc16_wide_kernel<bm, nw, expand, pf>
  CGK_COUNT
};
inline const char* conv_gen_kernel_id(ConvGenKernel k) {
  static const char* const ids[CGK_COUNT] = {"none", "cout1_loop", "cout1_taps", "smallcin", "x6",
                                             "exact", "nhwc16_tiles", "nhwc16_ring", "nhwc16_wide"};
  return ids[k];
}
enum ConvGenEpilogue { CGP_NONE = 0, CGP_COUT1_FINISH, CGP_SPLITK, CGP_SPLITK_TILE };
enum ConvGenY16 { CGY_NOBODY = 0, CGY_KERNEL, CGY_TILE_EPILOGUE, CGY_TRANSPOSE };
enum ConvGenRefusal { CGR_OK = 0, CGR_COUT1, CGR_CROP, CGR_Y16, CGR_SIZE, CGR_COUNT };
inline const char* conv_gen_refusal_text(ConvGenRefusal r) {
  switch (r) {
    case CGR_COUT1: return "ainp_conv_gen_fwd: Cout=1 options (workspace, kernel <= 8x8)";
    case CGR_CROP: return "ainp_conv_gen_fwd: crop needs Cout=1";
    case CGR_Y16: return "ainp_conv_gen_fwd: y16 is written by the few-input-channel kernel only";
    case CGR_SIZE: return "ainp_conv_gen_fwd: shape exceeds the launch grid";
    default: return "";
  }
}

struct ConvGenRoute {
  ConvGenEntry entry = CGE_NCHW;
  ConvGenKernel kernel = CGK_NONE;
  ConvGenRefusal refuse = CGR_OK;
  int bm = 0;              // output channels per tile (wide: 256 / 128 / 64)
  int bk = 0;              // CGK_X6: K-tile depth
  int planes = 0;          // CGK_X6: 3 split-bf16 planes (fp32) or 1 (bf16)
  int kt = 0;              // CGK_COUT1_TAPS: 3 or 4
  int nw = 0;              // CGK_NHWC16_WIDE: waves
  bool pf = true;          //   prefetch
  bool b16 = false;        // CGK_SMALLCIN: operands rounded to bf16
  bool lds16 = false;      //   the bf16 copy through LDS
  bool expand = false;     // nhwc16: a source arrives expanded per output pixel
  bool expand0 = false, expand1 = false;   //   which
  int nsplit = 1;
  int ktiles_per_split = 1 << 30;
  int64_t gx = 0, gy = 1, gz = 1;    // grid
  int64_t tco = 0, tpx = 0;          // CGK_NHWC16_WIDE: channel x pixel tiles (gx = tco * tpx)
  ConvGenEpilogue epilogue = CGP_NONE;
  int64_t ex = 0, ey = 1;            // its grid
  ConvGenY16 y16 = CGY_NOBODY;       // who writes the bf16 copy
  int64_t workspace = 0;             // bytes
  int64_t stat_rows = 0;             // BatchNorm partial rows (pixel tiles)
  bool ok() const { return refuse == CGR_OK; }
};

// K splits for a launch: small tile grids with long K (the U-Net bottleneck,
// VGG's last blocks) are split so ~768 workgroups run; >= 8 K tiles per split.
// For Cout > 64 count the workgroups of the bf16 wide-tile kernel (256 x 128 /
// 128 x 256 tiles, two per CU) and split grids under 384 of them to ~512: the
// U-Net decoder's 240-tile layers ran on half the CUs' slots (C4 9.34-9.37 ->
// 9.24-9.25, C5 11.98-12.00 -> 11.78-11.80 ms/step, profiles/r04t_summary.txt).
// The count follows the unpadded K on both entries.
inline int conv_gen_nsplit(const ConvGenEnv& env, int64_t NP, int Cout, int64_t K) {
  if (Cout == 1) return 1;
  const int BM = conv_gen_bm(Cout);
  const int64_t nkt = ceil_div(K, CG_BK);
  const bool wide = env.split_wide && Cout > 64;
  const int64_t blocks = !wide        ? sat_mul(ceil_div(NP, CG_TILE / BM), ceil_div(Cout, BM))
                         : Cout > 128 ? sat_mul(ceil_div(NP, 128), ceil_div(Cout, 256))
                                      : sat_mul(ceil_div(NP, 256), ceil_div(Cout, 128));
  if (blocks >= 384 || nkt < 16) return 1;
  int64_t s = wide ? env.split_wide / blocks : ceil_div(768, blocks);
  if (s > nkt / 8) s = nkt / 8;
  if (s < 1) s = 1;
  return (int)ceil_div(nkt, ceil_div(nkt, s));   // no empty split
}

namespace gen_detail {

inline bool fits_grid(int64_t x, int64_t y = 1, int64_t z = 1) {
  return x >= 1 && x <= INT_MAX && y >= 1 && y <= 65535 && z >= 1 && z <= 65535;
}

// Cout = 1 (the generator's last PartialConv2d, the discriminator's logit
// conv): channel-chunked partial sums, then the finish kernel; the only
// route that crops
inline void cout1_route(const ConvGenEnv& env, const ConvGenCall& c, ConvGenRoute& r) {
  const int64_t Cin = (int64_t)c.C0 + c.C1;
  const int64_t Hc = c.crop_h > 0 ? c.crop_h : c.Ho, Wc = c.crop_w > 0 ? c.crop_w : c.Wo;
  const int64_t np = sat_mul(c.N, Hc, Wc), nchunk = ceil_div(Cin, C1_CC);
  r.workspace = sat_mul(nchunk, np, sizeof(float));
  if (c.stats || Hc > c.Ho || Wc > c.Wo || (int64_t)c.KH * c.KW > C1_KMAX) {
    r.refuse = CGR_COUT1;
    return;
  }
  // one plain source, whole chunks, square 3 / 4 kernels, 32-bit offsets:
  // the batched-tap variant
  const bool plain = c.C1 == 0 && c.up0 == 0 && Cin % C1_CC == 0 && c.KH == c.KW &&
                     below(LIM_OFF32, c.N, Cin, sat_mul(c.Hin, c.Win), 4);
  r.kernel = env.cout1_taps && plain && (c.KH == 3 || c.KH == 4) ? CGK_COUT1_TAPS : CGK_COUT1_LOOP;
  r.kt = r.kernel == CGK_COUT1_TAPS ? c.KH : 0;
  r.gx = r.ex = ceil_div(np, 256);
  r.gy = nchunk;
  r.epilogue = CGP_COUT1_FINISH;
}

// the implicit GEMM's split-K and epilogue, common to both entries (`nkt`: K
// tiles the kernel walks)
inline void gemm_route(const ConvGenEnv& env, const ConvGenCall& c, int64_t NP, int64_t nkt,
                       ConvGenRoute& r) {
  r.nsplit = conv_gen_nsplit(env, NP, c.Cout, sat_mul((int64_t)c.C0 + c.C1, (int64_t)c.KH * c.KW));
  r.gx = ceil_div(NP, CG_TILE / r.bm);
  r.gy = ceil_div(c.Cout, r.bm);
  r.gz = r.nsplit;
  if (r.nsplit == 1) return;
  r.ktiles_per_split = (int)ceil_div(nkt, r.nsplit);
  r.workspace = sat_mul(sat_mul(r.nsplit, c.Cout), NP, sizeof(float));
  r.epilogue = env.splitk_tile ? CGP_SPLITK_TILE : CGP_SPLITK;
  r.ex = ceil_div(NP, env.splitk_tile ? SKT_P : 256);
  r.ey = env.splitk_tile ? ceil_div(c.Cout, SKT_C) : c.Cout;
  r.stat_rows = r.ex;
}

}  // namespace gen_detail

// The entry point and kernel of one call.  stat_rows and workspace are set
// on a refusal too (what a caller sizing its buffers first is told).
inline ConvGenRoute route_conv_gen(const ConvGenEnv& env, const ConvGenPolicy& pol,
                                   const ConvGenCall& c) {
  using namespace gen_detail;
  ConvGenRoute r;
  const int64_t NP = sat_mul(c.N, c.Ho, c.Wo), KK = (int64_t)c.KH * c.KW;
  const int64_t K = sat_mul((int64_t)c.C0 + c.C1, KK);
  r.bm = conv_gen_bm(c.Cout);
  r.stat_rows = ceil_div(NP, CG_TILE / r.bm);
  auto sized = [&]() {
    // the kernels take N, K and pixel indices' tile counts as int
    if (r.ok() && !(c.N <= INT_MAX && K <= INT_MAX && NP < INT64_MAX &&
                    fits_grid(r.gx, r.gy, r.gz) &&
                    (r.epilogue == CGP_NONE || fits_grid(r.ex, r.ey)))) {
      r.kernel = CGK_NONE;
      r.refuse = CGR_SIZE;
    }
    return r;
  };
  if (c.Cout == 1) {
    cout1_route(env, c, r);
    return sized();
  }
  if (c.crop_h > 0 || c.crop_w > 0) {
    r.refuse = CGR_CROP;
    return r;
  }
  // few input channels, one plain source, no BN statistics: the direct kernel
  const bool direct = env.smallcin && c.C1 == 0 && c.up0 == 0 && !c.stats && c.Cout <= SC_CO &&
                      c.C0 * KK <= SC_K && c.C0 <= SC_CIN;
  const bool whole = c.C0 % 32 == 0 && c.C1 % 32 == 0;
  if (pol.nhwc16 && c.b16 &&
      (whole || pol.nhwc16_small == 2 || (pol.nhwc16_small == 1 && !direct))) {
    r.entry = CGE_NHWC16;
    r.expand0 = c.C0 % 32 != 0;
    r.expand1 = c.C1 % 32 != 0;
    r.expand = r.expand0 || r.expand1;
    const int v = env.conv16_variant;
    r.kernel = v == 2 || (v == 3 && (c.Cout > 64 || env.conv16_small_wide)) ? CGK_NHWC16_WIDE
               : v == 1 ? CGK_NHWC16_RING : CGK_NHWC16_TILES;
    // the padded K tiles are spread over the splits of the unpadded K
    gemm_route(env, c, NP, (nhwc16_seg(c.C0, (int)KK) + nhwc16_seg(c.C1, (int)KK)) / CG_BK, r);
    if (r.kernel == CGK_NHWC16_WIDE) {
      // 256 x 128 / 128 x 256 / 64 x 256 (channels x pixels)
      r.bm = c.Cout > 128 ? 256 : (c.Cout > 64 ? 128 : 64);
      r.nw = v == 3 && r.bm > 64 ? 8 : 4;
      r.pf = r.nw == 8 ? env.wide_pf : true;
      r.tco = ceil_div(c.Cout, r.bm);
      r.tpx = ceil_div(NP, r.bm == 256 ? 128 : 256);
      r.gx = sat_mul(r.tco, r.tpx);
      r.gy = r.nsplit;
      r.gz = 1;
    }
    // split-K layers are small: without the tiled epilogue their bf16 copy is
    // the coalesced transpose kernel's
    if (c.y16 && pol.out16)
      r.y16 = r.nsplit == 1 ? CGY_KERNEL : env.splitk_tile ? CGY_TILE_EPILOGUE : CGY_TRANSPOSE;
    return sized();
  }
  if (direct) {
    r.kernel = CGK_SMALLCIN;
    r.b16 = c.b16;
    if (c.y16 && pol.out16 && pol.out16_direct && c.Cout % 8 == 0) r.y16 = CGY_KERNEL;
    r.lds16 = env.smallcin_lds16 && r.y16 == CGY_KERNEL;
    r.gx = ceil_div(NP, 256);
    return sized();
  }
  gemm_route(env, c, NP, ceil_div(K, CG_BK), r);
  if (c.b16) {
    // one plane; the 64-deep tiles need an even count per split
    r.kernel = CGK_X6;
    r.planes = 1;
    r.bk = env.b16_bk == 64 && r.nsplit > 1 && r.ktiles_per_split % 2 ? 32 : env.b16_bk;
  } else if (!env.exact) {
    r.kernel = CGK_X6;   // fp32-accurate split-bf16 main loop
    r.planes = 3;
    r.bk = env.x6_bk;
  } else {
    r.kernel = CGK_EXACT;
  }
  return sized();
}

// The kernel's name as profiler rows carry it, up to the first template
// argument that tells two routes apart (bench.py matches rows by substring;
// "conv_cout1_partial" covers both Cout = 1 kernels).
inline const char* conv_gen_kernel_name(const ConvGenRoute& r) {
  switch (r.kernel) {
    case CGK_COUT1_LOOP:
    case CGK_COUT1_TAPS: return "conv_cout1_partial";
    case CGK_SMALLCIN: return "conv_gen_smallcin_kernel";
    case CGK_X6: return "conv_gen_x6_kernel";
    case CGK_EXACT: return "conv_gen_fwd_kernel";
    case CGK_NHWC16_TILES:
      return r.bm == 128 ? "conv_gen_nhwc16_kernel<128" : "conv_gen_nhwc16_kernel<64";
    case CGK_NHWC16_RING:
      return r.bm == 128 ? "conv_gen_nhwc16_ring_kernel<128" : "conv_gen_nhwc16_ring_kernel<64";
    case CGK_NHWC16_WIDE:
      return r.bm == 256   ? "conv_gen_nhwc16_wide_kernel<256"
             : r.bm == 128 ? "conv_gen_nhwc16_wide_kernel<128"
                           : "conv_gen_nhwc16_wide_kernel<64";
    default: return "";
  }
}

// ---------------------------------------------------------------- queries
// (include/ainp.h: each is what route_conv_gen answers)
inline ConvGenCall conv_gen_call(const AinpConvGenCall& a) {
  ConvGenCall c;
  c.N = a.N;
  c.C0 = a.C0;
  c.C1 = a.C1;
  c.up0 = conv_gen_src_up(a.H0, a.W0, a.Hin, a.Win);
  c.up1 = a.C1 ? conv_gen_src_up(a.H1, a.W1, a.Hin, a.Win) : 0;
  c.Hin = a.Hin;
  c.Win = a.Win;
  c.Ho = conv_gen_out(a.Hin, a.KH, a.stride, a.pad);
  c.Wo = conv_gen_out(a.Win, a.KW, a.stride, a.pad);
  c.KH = a.KH;
  c.KW = a.KW;
  c.Cout = a.Cout;
  c.crop_h = a.crop_h;
  c.crop_w = a.crop_w;
  c.b16 = (a.flags & AINP_CONV_BF16) != 0;
  c.stats = a.want_stats != 0;
  c.y16 = a.want_y16 != 0;
  return c;
}
inline ConvGenPolicy conv_gen_policy(const AinpConvGenCall& a) {
  ConvGenPolicy p;
  p.nhwc16 = a.nhwc16 != 0;
  p.nhwc16_small = a.nhwc16_small;
  p.out16 = a.out16 != 0;
  p.out16_direct = a.out16_direct != 0;
  return p;
}
// ainp_conv_gen_stat_parts / _workspace know channels, kernel and output size
// only: one plain fp32 source on the NCHW entry (both entries answer the same)
inline ConvGenRoute query_conv_gen(const ConvGenEnv& env, int64_t N, int Cin, int KH, int KW,
                                   int Cout, int64_t Ho, int64_t Wo, bool stats) {
  ConvGenCall c;
  c.N = N;
  c.C0 = Cin;
  c.Hin = c.Ho = Ho;
  c.Win = c.Wo = Wo;
  c.KH = KH;
  c.KW = KW;
  c.Cout = Cout;
  c.stats = stats;
  return route_conv_gen(env, conv_gen_policy_nchw(), c);
}

}  // namespace ainp
