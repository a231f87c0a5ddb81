// conv_route.h — which 3x3 conv kernel serves which call (host only).
//
// Plain C++17, no HIP: the launchers of conv.hip / conv_x6.hip call
// route_conv / route_wgrad once and switch on the kernel id, and every
// host-only query of include/ainp.h (stat rows, *_ok) is the same function's
// answer, so the two cannot drift apart.  tests/sanitize/conv_route_check.cpp
// walks the table under ASan + UBSan without a GPU.
//
// All size arithmetic saturates: a product past its limit "does not fit".
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/ainp.h"

namespace ainp {

// ---------------------------------------------------------------- tilings
constexpr int CV_FT = 8;           // exact f32 kernels: rows per tile
constexpr int CV_TT = 48;          // columns per tile (3 MFMA tiles)
constexpr int R1_TW = 14, R1_RS = 16;     // 16 -> 1 row strips: columns per wave, rows
constexpr int R16_TW = 14, R16_RS = 16;   // 1 -> 16 row strips
constexpr int SW_RS = 32;          // small weight gradients: rows per strip
constexpr int SW_TW = 62;          // output columns per wave
constexpr int SW_RB = 8;           // rows loaded per batch
constexpr int SWC_TW = 14;         // channel-last strips: output columns per wave
constexpr int SWG_GROUPS = 128, SWG_GROUPS_MAX = 128;   // small slab sum: first-stage groups
constexpr int WG_BLOCKS = 512;     // weight-gradient persistent grid (slabs)
constexpr int WG_GROUPS = 16;      // stage-1 groups of WG_BLOCKS / WG_GROUPS slabs
constexpr int WG_CIMAX = 32;       // input channels staged per pass
namespace cx6 { constexpr int TR = 16, TC = 32; }   // tiled split-bf16: rows x columns
namespace cdf { constexpr int TR = 8, TC = 32; }    // bf16 LDS-DMA forward tiles
namespace cdd {                                      // bf16 LDS-DMA 64 -> 32 data gradient
constexpr int CI = 64, COP = 32, TR = 8, TC = 32, HR = TR + 2, HC = TC + 2;
constexpr int XROW = HC * 32, XPLANE = HR * XROW;           // 1088, 10880
constexpr int NPIX = HR * HC;                                // 340 halo pixels
constexpr int XBLK = (NPIX * 32 + 1023) / 1024;              // 11 DMA blocks per plane
constexpr int XPP = XBLK * 1024;                             // padded plane
constexpr int NCK = CI / 16;                                 // 4 planes
constexpr int XBUF = NCK * XPP;                              // 45056 per halo buffer
constexpr int WROW = 9 * 32 + 16, WPLANE = COP * WROW;       // 304, 9728
constexpr int NT = 512;
constexpr int YBLK = TR * TC * COP * 2 / 1024;              // 16 blocks: bf16 y of a tile
}  // namespace cdd
namespace wdm { constexpr int TT = 24; }            // bf16 LDS-DMA weight gradient: tile columns
// persistent grids of the split-bf16 forward / data gradient (x6p / x6q):
// one or two workgroups per CU
constexpr int X6P_GRID1 = 256, X6P_GRID2 = 512;
// Upper bound of the persistent-grid multiplier of the bf16 (NP = 1) kernels
// (ConvEnv::x6_occ16): BatchNorm partial rows and weight-gradient slabs are
// sized for it.
constexpr int X6_OCC_MAX = 4;

// activation layouts of a launch (bitmask): input / output / dy channel-last
constexpr int CL_X = 1, CL_Y = 2, CL_G = 4;
// round 6: a data gradient's dx written [C][H][N][W] (AINP_CONV_YCFNT) -- the
// [C*F, N*T] operand of the fp32 output projection's backward GEMMs, so the
// transposing copy of the decoder input gradient disappears (x6q only)
constexpr int CL_CF = 8;

// ---------------------------------------------------------------- sizes
constexpr int64_t LIM_OFF32 = (int64_t)1 << 31;   // 32-bit buffer offsets / int counts
constexpr int64_t LIM_ELEM40 = (int64_t)1 << 40;  // elements of a 16-channel tensor

inline int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }
// product of non-negative factors, INT64_MAX when it does not fit
inline int64_t sat_mul(int64_t a, int64_t b) {
  int64_t r;
  return __builtin_mul_overflow(a, b, &r) ? INT64_MAX : r;
}
inline int64_t sat_mul(int64_t a, int64_t b, int64_t c) { return sat_mul(sat_mul(a, b), c); }
inline bool below(int64_t limit, int64_t a, int64_t b, int64_t c = 1, int64_t d = 1) {
  return sat_mul(sat_mul(a, b), sat_mul(c, d)) < limit;
}
inline int64_t tiles(int64_t N, int64_t H, int64_t W, int tr, int tc) {
  return sat_mul(N, ceil_div(H, tr), ceil_div(W, tc));
}

// ---------------------------------------------------------------- environment
// Read once per process (conv_env()); the route functions take it as an
// argument so a test can pass any setting.
struct ConvEnv {
  bool exact = false;        // AINP_CONV_EXACT=1: the exact f32 kernels, no split-bf16
  bool x6_tiled = false;     // AINP_CONV_X6_TILED set: no persistent x6p / x6q
  bool small_rows = true;    // AINP_SMALL_ROWS=0: the 8 x 48 tile kernel for 1 <-> 16 (A/B)
  bool dgrad_bnr = true;     // AINP_DGRAD_BNR=0: data gradient, then the reduce (two passes)
  bool conv16_dma = true;    // AINP_CONV16_DMA=0: the register-staged x6p forwards (A/B)
  bool dgrad16_dma = true;   // AINP_DGRAD16_DMA=0: register-staged 64 -> 32 data gradient
  bool wgrad16_dma = true;   // AINP_WGRAD16_DMA=0: register-staged 32 -> 64 weight gradient
  // Persistent-grid multiplier of the bf16 (NP = 1) kernels: their LDS (21-50
  // KB) and VGPR (48-80) footprints let 2-4x the fp32 kernels' workgroups stay
  // resident, and they are bound by the loads a CU keeps in flight (SQ passes:
  // MFMA busy 0.05-0.10, waves parked on s_waitcnt 0.5-0.67 of their cycles,
  // profiles/r04e_*).  AINP_X6_OCC16 overrides (1 .. X6_OCC_MAX).
  int x6_occ16 = 1;
};

inline ConvEnv conv_env_read() {
  auto not0 = [](const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
  };
  ConvEnv v;
  const char* e = getenv("AINP_CONV_EXACT");
  v.exact = e && e[0] == '1';
  v.x6_tiled = getenv("AINP_CONV_X6_TILED") != nullptr;
  v.small_rows = not0("AINP_SMALL_ROWS");
  v.dgrad_bnr = not0("AINP_DGRAD_BNR");
  v.conv16_dma = not0("AINP_CONV16_DMA");
  v.dgrad16_dma = not0("AINP_DGRAD16_DMA");
  v.wgrad16_dma = not0("AINP_WGRAD16_DMA");
  e = getenv("AINP_X6_OCC16");
  const int o = e ? atoi(e) : 1;
  v.x6_occ16 = o < 1 ? 1 : (o > X6_OCC_MAX ? X6_OCC_MAX : o);
  return v;
}
inline const ConvEnv& conv_env() {
  static const ConvEnv v = conv_env_read();
  return v;
}

// ---------------------------------------------------------------- ABI flags
// forward: the act(x) source and / or y in bf16 storage (with the bf16
// arithmetic); either may be channel-last
inline bool conv_fwd_flags_ok(int flags) {
  flags &= ~(AINP_CONV_XCL | AINP_CONV_YCL);
  return (flags & ~(AINP_CONV_BF16 | AINP_CONV_X16 | AINP_CONV_Y16)) == 0 &&
         (!(flags & (AINP_CONV_X16 | AINP_CONV_Y16)) || (flags & AINP_CONV_BF16));
}
// data / weight gradients: dy may be bf16 storage (with the bf16 arithmetic);
// data gradient: dy / dx channel-last; weight gradient: x / dy channel-last
inline bool conv_grad_flags_ok(int flags, bool wgrad) {
  // data gradient: dx [C][H][N][W] (AINP_CONV_YCFNT) instead of channel-last
  if ((flags & AINP_CONV_YCFNT) && (wgrad || (flags & AINP_CONV_YCL))) return false;
  if (!wgrad) flags &= ~AINP_CONV_YCFNT;
  flags &= ~(wgrad ? (AINP_CONV_XCL | AINP_CONV_GCL) : (AINP_CONV_XCL | AINP_CONV_YCL));
  const int extra = AINP_CONV_DY16 | (wgrad ? AINP_CONV_X16 : 0);
  return (flags & ~(AINP_CONV_BF16 | extra)) == 0 &&
         (!(flags & extra) || (flags & AINP_CONV_BF16));
}
// ABI layout flags -> the kernels' layout bits
inline int conv_lay(int flags) {
  return ((flags & AINP_CONV_XCL) ? CL_X : 0) | ((flags & AINP_CONV_YCL) ? CL_Y : 0) |
         ((flags & AINP_CONV_GCL) ? CL_G : 0) | ((flags & AINP_CONV_YCFNT) ? CL_CF : 0);
}

// (Cin, Cout) pairs with a dedicated small-channel kernel
inline bool small_pair(int a, int b) {
  return ((a == 1 || a == 2) && b == 16) || ((b == 1 || b == 2) && a == 16);
}

// ---------------------------------------------------------------- refusals
enum ConvRefusal {
  CR_OK = 0,
  CR_NO16, CR_CL16, CR_CL_EXACT, CR_COUT64, CR_NODX, CR_FWD_TILES, CR_CFNT, CR_BNR_ARG,
  CR_W_ARG, CR_W_NO16, CR_W_CL, CR_W_COUT64, CR_W_BNA, CR_W_SMALL_CL, CR_W_TILES,
  CR_COUNT
};
inline const char* conv_refusal_text(ConvRefusal r) {
  switch (r) {
    case CR_NO16: return "conv3x3: bf16 storage (AINP_CONV_DY16 / _X16 / _Y16) needs a split-bf16 kernel for this pair";
    case CR_CL16: return "conv3x3: no channel-last / bf16-storage kernel for this pair";
    case CR_CL_EXACT: return "conv3x3: channel-last activations need a split-bf16 kernel for this pair";
    case CR_COUT64: return "conv3x3: Cout > 64 unsupported";
    case CR_NODX: return "conv3x3: a partials-only data gradient needs the row-strip kernel";
    case CR_FWD_TILES: return "conv3x3_fwd_b16dma: too many tiles";
    case CR_CFNT: return "ainp_conv3x3_dgrad: AINP_CONV_YCFNT serves the 32 -> 16 channel data "
                         "gradient only (see ainp_conv3x3_dgrad_cfnt_ok)";
    case CR_BNR_ARG: return "ainp_conv3x3_dgrad_bnr: bad argument (channel-last dx and y, C in "
                            "{16, 32, 64}, 16-byte aligned dx / y / scale / shift / save)";
    case CR_W_ARG: return "ainp_conv3x3_wgrad: bad argument";
    case CR_W_NO16: return "ainp_conv3x3_wgrad: bf16 storage (AINP_CONV_DY16 / _X16) needs a split-bf16 "
                           "weight-gradient kernel for this pair";
    case CR_W_CL: return "ainp_conv3x3_wgrad: channel-last activations need a split-bf16 kernel";
    case CR_W_COUT64: return "ainp_conv3x3_wgrad: Cout > 64 unsupported";
    case CR_W_BNA: return "conv3x3_wgrad: fused BatchNorm apply: 1 -> 16 only";
    case CR_W_SMALL_CL: return "conv3x3_wgrad: no channel-last small-channel kernel for this pair";
    case CR_W_TILES: return "conv3x3_wgrad_b16dma: too many tiles";
    default: return "";
  }
}

// ---------------------------------------------------------------- forward / data gradient
enum ConvKernel {
  CK_NONE = 0,
  CK_ROWS_16TO1,     // conv3x3_rows_16to1 (row strips, channel-last x)
  CK_ROWS_1TO16,     // conv3x3_rows_1to16 (row strips, channel-last y)
  CK_SMALL_TILE,     // conv3x3_small_fwd (8 x 48 tiles)
  CK_EXACT,          // conv3x3_fwd_mfma (exact f32)
  CK_X6P,            // conv3x3_x6p_kernel (persistent split-bf16)
  CK_X6Q,            // conv3x3_x6q_kernel (persistent 32 -> 16)
  CK_X6_TILED,       // conv3x3_x6_kernel (16- or 8-row tiles)
  CK_FWD_B16DMA,     // conv3x3_fwd_b16dma_kernel (bf16 channel-last, LDS DMA)
  CK_DGRAD_B16DMA,   // conv3x3_dgrad_b16dma_kernel (bf16 64 -> 32, LDS DMA)
  CK_COUNT
};
inline const char* conv_kernel_name(ConvKernel k) {
  static const char* const names[CK_COUNT] = {"none", "rows_16to1", "rows_1to16", "small_tile",
                                              "exact", "x6p", "x6q", "x6_tiled", "fwd_b16dma",
                                              "dgrad_b16dma"};
  return names[k];
}

// One launch as the kernels see it: the conv over `Cin` source channels
// producing `Cout` (a data gradient of nn.Conv2d(a, b) runs b -> a).
struct ConvCall {
  bool dgrad = false;
  int64_t N = 0;
  int Cin = 0, Cout = 0;
  int64_t H = 0, W = 0;
  bool b16 = false;      // AINP_CONV_BF16 arithmetic
  bool x16 = false;      // source (x, or dy of a data gradient) in bf16 storage
  bool y16 = false;      // forward output in bf16 storage
  int lay = 0;           // CL_X | CL_Y | CL_CF
  bool stats = false;    // BatchNorm partials wanted
  bool bias = false;
  bool pro = false;      // in_scale / in_shift prologue
  bool fused = false;    // Bnr: the consuming BatchNorm's backward reduce in the epilogue
  bool bnr_y16 = false;  // Bnr::y16
  bool nodx = false;     // the partials only (dx == NULL)
};

struct ConvRoute {
  ConvKernel kernel = CK_NONE;
  ConvRefusal refuse = CR_OK;
  int64_t gx = 0, gy = 1, gz = 1;   // grid
  int64_t rows = 0;       // BatchNorm partial rows the kernel writes
  int64_t rows_pad = 0;   // rows the entry point defines ([rows, rows_pad) zero-filled)
  bool fast = false;      // CK_EXACT: the specialised staging (channel multiples, 32-bit offsets)
  bool dg8 = false;       // CK_X6_TILED: 8-row tiles (a data gradient without forward statistics)
  bool two_pass = false;  // fused asked, no fused kernel: this data gradient, then the reduce
  bool ok() const { return refuse == CR_OK; }
};

namespace route_detail {

inline ConvRoute refused(ConvRefusal why) {
  ConvRoute r;
  r.refuse = why;
  return r;
}
inline ConvRoute grid1(ConvKernel k, int64_t g, int64_t rows_pad = -1) {
  ConvRoute r;
  r.kernel = k;
  r.gx = g;
  r.rows = g;
  r.rows_pad = rows_pad < 0 ? g : rows_pad;
  return r;
}

// the small-channel pairs (1 / 2 <-> 16): row strips where the call allows,
// the 8 x 48 tile kernel otherwise
inline ConvRoute small_route(const ConvEnv& env, const ConvCall& c) {
  const int64_t parts = tiles(c.N, c.H, c.W, CV_FT, CV_TT);
  const bool e40 = below(LIM_ELEM40, c.N, c.H, c.W, 16);
  if (!c.dgrad && c.Cin == 16 && c.Cout == 1 && (c.lay & CL_X) && env.small_rows && e40) {
    const int64_t ns = tiles(c.N, c.H, c.W, R1_RS, R1_TW), nb = ceil_div(ns, 4);
    if (ns < LIM_OFF32 && nb <= parts) return grid1(CK_ROWS_16TO1, nb, parts);
  }
  if (c.Cin == 1 && c.Cout == 16 && (c.lay & CL_Y) && env.small_rows && e40 &&
      (c.dgrad || !c.fused)) {
    const int64_t ns = tiles(c.N, c.H, c.W, R16_RS, R16_TW), nb = ceil_div(ns, 4);
    if (ns < LIM_OFF32 && nb <= parts) return grid1(CK_ROWS_1TO16, nb, parts);
  }
  if (c.nodx) return refused(CR_NODX);
  ConvRoute r;
  r.kernel = CK_SMALL_TILE;
  r.gx = ceil_div(c.W, CV_TT);
  r.gy = ceil_div(c.H, CV_FT);
  r.gz = c.N;
  r.rows = r.rows_pad = parts;
  return r;
}

// the split-bf16 kernels of conv_x6.hip: true if one serves the call (*r) or
// the call is refused (*r); false if the pair has none
inline bool x6_route(const ConvEnv& env, const ConvCall& c, ConvRoute* r) {
  const ConvRefusal no = c.lay ? CR_CL16 : CR_NO16;
  // the fused reduce: a data gradient writing channel-last dx of at most 32 channels
  if (c.fused && !(c.dgrad && c.stats && (c.lay & CL_Y) && !c.bias && c.Cout <= 32)) {
    *r = refused(no);
    return true;
  }
  if (c.Cout < 16 || c.Cout > 64) return false;
  const int cop = c.Cout <= 32 ? 32 : 64;
  const bool cin_fits = below(LIM_OFF32, c.Cin, c.H, c.W, 4);   // 32-bit buffer offsets
  const bool pers = !env.x6_tiled && below(LIM_OFF32, c.Cin > c.Cout ? c.Cin : c.Cout, c.H, c.W, 4);
  const bool p3264 = c.Cin == 32 && cop == 64, p1632 = c.Cin == 16 && cop == 32;
  const bool p3216 = c.Cin == 32 && c.Cout == 16;
  const bool pers_pair = pers && ((!c.dgrad && p3264) || p1632 || p3216);
  const bool tiled_pair = (p3264 || (c.Cin == 64 && cop == 32)) && cin_fits;
  if (!pers_pair && !tiled_pair) return false;
  // the channel-last stores write four consecutive channels of a pixel: a
  // Cout that is no multiple of 4 would run into the next pixel (and, on the
  // last one, past the tensor)
  if ((c.lay & CL_Y) && c.Cout % 4 != 0) {
    *r = refused(CR_CL16);
    return true;
  }
  const int occ = c.b16 ? env.x6_occ16 : 1;
  if (pers_pair) {
    // bf16 channel-last forward with bf16 source and output: the LDS-DMA
    // kernel, on x6p's grid (the same BatchNorm partial rows, bit-identical)
    if (!c.dgrad && c.b16 && c.x16 && c.y16 && c.lay == (CL_X | CL_Y) && c.Cout % 4 == 0 &&
        env.conv16_dma && (p3264 || p1632)) {
      if (tiles(c.N, c.H, c.W, cdf::TR, cdf::TC) >= LIM_OFF32) *r = refused(CR_FWD_TILES);
      else *r = grid1(CK_FWD_B16DMA, (p3264 ? X6P_GRID1 : X6P_GRID2) * occ);
      return true;
    }
    // two workgroups per CU where the LDS allows it (one 16-channel chunk;
    // x6q: 65 KB of LDS, bf16: more)
    *r = p3216 ? grid1(CK_X6Q, X6P_GRID2 * occ)
               : grid1(CK_X6P, (p3264 ? X6P_GRID1 : X6P_GRID2) * occ);
    return true;
  }
  // tiled.  The data gradient without forward statistics: 8-row tiles
  // (channel-last, bf16 dy, the fused reduce)
  const bool dg8 = c.dgrad && (!c.stats || c.fused);
  if (c.y16 || (c.x16 && !(dg8 && c.b16)) || (c.lay && !dg8)) {
    *r = refused(no);
    return true;
  }
  const int64_t nt8 = tiles(c.N, c.H, c.W, 8, cx6::TC);
  if (dg8 && c.b16 && c.x16 && c.lay == (CL_X | CL_Y) && c.Cin == cdd::CI && c.Cout == cdd::COP &&
      !c.bias && !c.pro && (!c.fused || c.bnr_y16) && env.dgrad16_dma) {
    *r = grid1(CK_DGRAD_B16DMA, nt8 < X6P_GRID1 ? nt8 : X6P_GRID1);   // one workgroup per CU
    return true;
  }
  r->kernel = CK_X6_TILED;
  r->dg8 = dg8;
  r->gx = ceil_div(c.W, cx6::TC);
  r->gy = ceil_div(c.H, dg8 ? 8 : cx6::TR);
  r->gz = c.N;
  r->rows = r->rows_pad = dg8 ? nt8 : tiles(c.N, c.H, c.W, cx6::TR, cx6::TC);
  return true;
}

inline ConvRoute plain_route(const ConvEnv& env, const ConvCall& c) {
  if (small_pair(c.Cin, c.Cout))
    return (c.x16 || c.y16) ? refused(CR_NO16) : small_route(env, c);
  ConvRoute r;
  if (!env.exact && x6_route(env, c, &r)) return r;
  if (c.x16 || c.y16) return refused(CR_NO16);
  if (c.lay) return refused(CR_CL_EXACT);
  if ((c.Cout + 15) / 16 > 4) return refused(CR_COUT64);
  r.kernel = CK_EXACT;
  r.gx = ceil_div(c.W, CV_TT);
  r.gy = ceil_div(c.H, CV_FT);
  r.gz = c.N;
  r.rows = r.rows_pad = tiles(c.N, c.H, c.W, CV_FT, CV_TT);
  r.fast = c.Cin % 8 == 0 && c.Cout % 16 == 0 && below(LIM_OFF32, c.Cin, c.H, c.W, 4);
  return r;
}

}  // namespace route_detail

// The kernel of one forward or data-gradient call.
inline ConvRoute route_conv(const ConvEnv& env, const ConvCall& c) {
  using namespace route_detail;
  // [C][H][N][W] dx: the persistent 32 -> 16 data gradient (x6q) only
  if ((c.lay & CL_CF) &&
      !(c.dgrad && !env.exact && !env.x6_tiled && c.Cin == 32 && c.Cout == 16 && !(c.lay & CL_Y) &&
        below(LIM_ELEM40, c.N, c.H, c.W, 16) && below(LIM_OFF32, c.Cin, c.H, c.W, 4)))
    return refused(CR_CFNT);
  if (!c.fused) return c.nodx ? refused(CR_BNR_ARG) : plain_route(env, c);
  // the fused reduce: the small kernels' channel-last epilogue (1 / 2 -> 16),
  // a split-bf16 data gradient, or the two passes
  const bool small = small_pair(c.Cin, c.Cout);
  ConvRoute r;
  if (env.dgrad_bnr && small && c.Cout % 4 == 0 && !c.x16) r = small_route(env, c);
  else if (c.nodx) return refused(CR_BNR_ARG);
  else if (!(env.dgrad_bnr && !small && !env.exact && x6_route(env, c, &r) && r.ok())) {
    ConvCall p = c;
    p.fused = p.bnr_y16 = p.stats = false;
    r = plain_route(env, p);
    r.two_pass = true;
    return r;
  }
  // the launcher sums `rows` partial rows with an int count, and no others
  if (r.ok() && r.rows >= LIM_OFF32) return refused(CR_BNR_ARG);
  r.rows_pad = r.rows;
  return r;
}

// ---------------------------------------------------------------- weight gradient
enum WgradKernel {
  WK_NONE = 0,
  WK_STRIP_CL,     // conv3x3_strip_wgrad_cl (1 <-> 16, the 16-channel side channel-last)
  WK_STRIP,        // conv3x3_strip_wgrad (row strips)
  WK_SMALL_TILE,   // conv3x3_small_wgrad (8 x 48 tiles)
  WK_X6S,          // conv3x3_wgrad_x6s (split-bf16, 32 -> 16 / 16 -> 32)
  WK_X6,           // conv3x3_wgrad_x6 (split-bf16, 32 -> 64)
  WK_B16DMA,       // conv3x3_wgrad_b16dma_kernel (bf16 channel-last 32 -> 64, LDS DMA)
  WK_T,            // conv3x3_wgrad_t (exact f32, specialised pairs)
  WK_MFMA,         // conv3x3_wgrad_mfma (exact f32, any pair)
  WK_COUNT
};
inline const char* wgrad_kernel_name(WgradKernel k) {
  static const char* const names[WK_COUNT] = {"none", "strip_cl", "strip", "small_tile", "x6s",
                                              "x6", "wgrad_b16dma", "wgrad_t", "wgrad_mfma"};
  return names[k];
}

// One pass (input channels ci0 .. ci0 + WG_CIMAX) of nn.Conv2d(Cin, Cout)'s
// weight gradient; the small pairs have a single pass.
struct WgradCall {
  int64_t N = 0;
  int Cin = 0, Cout = 0;
  int64_t H = 0, W = 0;
  bool b16 = false, g16 = false, x16 = false;   // arithmetic; dy / act(x) source bf16 storage
  int lay = 0;             // CL_X | CL_G
  bool bna = false;        // fused BatchNorm apply (ainp_conv3x3_wgrad_bnapply)
  bool small_tile = false; // AINP_SMALL_WGRAD_TILE=1 (read per call)
  int ci0 = 0;
  int ncu = 256;           // compute units of the device (WK_B16DMA: one workgroup each)
};

struct WgradRoute {
  WgradKernel kernel = WK_NONE;
  ConvRefusal refuse = CR_OK;
  int64_t gx = 0, gy = 1, gz = 1;
  int64_t slabs = 0;   // partial slabs written (the reduce's row count)
  int cp = 0;          // input channels of this pass
  bool ok() const { return refuse == CR_OK; }
};

inline int wgrad_ct(int Cout) { return (Cout + 15) / 16; }
inline int wgrad_pass(int Cin) { return Cin < WG_CIMAX ? Cin : WG_CIMAX; }

inline WgradRoute route_wgrad(const ConvEnv& env, const WgradCall& c) {
  WgradRoute r;
  auto refused = [&](ConvRefusal why) {
    r = WgradRoute{};
    r.refuse = why;
    return r;
  };
  if (small_pair(c.Cin, c.Cout)) {
    if (c.g16 || c.x16) return refused(CR_W_NO16);
    r.cp = c.Cin;
    const bool acl = (c.lay & CL_X) && c.Cin == 16, gcl = (c.lay & CL_G) && c.Cout == 16;
    if (c.bna && !(gcl && c.Cin == 1)) return refused(CR_W_BNA);
    if ((acl && c.Cout == 1) || (gcl && c.Cin == 1)) {
      r.kernel = WK_STRIP_CL;
      r.slabs = tiles(c.N, c.H, c.W, SW_RS, SWC_TW);
      r.gx = ceil_div(r.slabs, 4);
    } else if (acl || gcl) {
      return refused(CR_W_SMALL_CL);
    } else if (!c.small_tile && below(LIM_OFF32, c.H, c.W)) {
      r.kernel = WK_STRIP;
      r.slabs = tiles(c.N, c.H, c.W, SW_RS, SW_TW);
      r.gx = r.slabs;
      r.gy = ceil_div(c.Cin * c.Cout, 4);
    } else {
      r.kernel = WK_SMALL_TILE;
      r.gx = ceil_div(c.W, CV_TT);
      r.gy = ceil_div(c.H, CV_FT);
      r.gz = c.N;
      r.slabs = tiles(c.N, c.H, c.W, CV_FT, CV_TT);
    }
    // the kernels and the slab sum index slabs with an int
    return r.slabs < LIM_OFF32 ? r : refused(CR_W_ARG);
  }
  if (wgrad_ct(c.Cout) > 4) return refused(CR_W_COUT64);
  const int cp = (c.Cin - c.ci0) < WG_CIMAX ? (c.Cin - c.ci0) : WG_CIMAX;
  r.cp = cp;
  r.gx = r.slabs = WG_BLOCKS;
  // specialised kernels: 32-bit buffer offsets must cover a sample's planes
  const bool fits = below(LIM_OFF32, c.H, c.W, 4, c.Cout > WG_CIMAX ? c.Cout : WG_CIMAX);
  // split-bf16 kernel where it is instantiated, unless AINP_CONV_EXACT=1;
  // same slab format
  if (fits && !env.exact) {
    const int grid = c.b16 ? WG_BLOCKS * env.x6_occ16 : WG_BLOCKS;
    // bf16 channel-last 32 -> 64 (the bf16 configuration's encoder conv): the
    // LDS-DMA kernel, one workgroup per CU, a multiple of WG_GROUPS
    if (c.b16 && c.g16 && c.x16 && c.lay == (CL_X | CL_G) && c.Cin == 32 && cp == 32 &&
        c.ci0 == 0 && c.Cout == 64 && env.wgrad16_dma) {
      if (tiles(c.N, c.H, c.W, 4, wdm::TT) >= LIM_OFF32) return refused(CR_W_TILES);
      r.kernel = WK_B16DMA;
      r.gx = r.slabs = c.ncu >= WG_GROUPS ? c.ncu / WG_GROUPS * WG_GROUPS : WG_GROUPS;
      return r;
    }
    if ((cp == 32 && c.Cout == 16) || (cp == 16 && c.Cout == 32)) r.kernel = WK_X6S;
    else if (cp == 32 && c.Cout == 64) r.kernel = WK_X6;
    if (r.kernel != WK_NONE) {
      r.gx = r.slabs = grid;
      return r;
    }
  }
  if (c.g16 || c.x16) return refused(CR_W_NO16);
  if (c.lay) return refused(CR_W_CL);
  r.kernel = fits && (cp == 16 || cp == 32) && (c.Cout == 16 || c.Cout == 32 || c.Cout == 64)
                 ? WK_T : WK_MFMA;
  return r;
}

// every pass of the weight gradient is served
inline bool wgrad_accepts(const ConvEnv& env, WgradCall c) {
  for (c.ci0 = 0; c.ci0 == 0 || c.ci0 < c.Cin; c.ci0 += WG_CIMAX)
    if (!route_wgrad(env, c).ok()) return false;
  return true;
}

// ---------------------------------------------------------------- bounds
// ainp_conv3x3_fwd_stat_parts: bounds rows_pad of every fp32 forward route
// (CK_ROWS_*, CK_SMALL_TILE and CK_EXACT: the 8 x 48 tiles; CK_X6_TILED: 16 x
// 32 tiles; CK_X6P / CK_X6Q: X6P_GRID2).  The bf16 routes multiply the
// persistent grids by ConvEnv::x6_occ16 (<= X6_OCC_MAX).
inline int64_t conv_stat_parts(int64_t N, int64_t H, int64_t W) {
  const int64_t a = tiles(N, H, W, CV_FT, CV_TT), b = tiles(N, H, W, cx6::TR, cx6::TC);
  const int64_t m = a > b ? a : b;
  return m > X6P_GRID2 ? m : X6P_GRID2;
}
// ainp_conv3x3_dgrad_bnr_workspace's partial rows: bounds `rows` of every
// fused route_conv result (CK_X6_TILED / CK_DGRAD_B16DMA: 8-row tiles;
// CK_X6P / CK_X6Q: X6P_GRID2 * X6_OCC_MAX; the small kernels: 8 x 48 tiles)
inline int64_t dgrad_bnr_rows(int64_t N, int64_t H, int64_t W) {
  int64_t rows = tiles(N, H, W, 8, cx6::TC);
  const int64_t pers = X6P_GRID2 * (int64_t)X6_OCC_MAX, small = tiles(N, H, W, CV_FT, CV_TT);
  if (rows < pers) rows = pers;
  return rows < small ? small : rows;
}
// ainp_conv3x3_wgrad_workspace: bounds the slabs of every route_wgrad result
// and the slab sum's first-stage buffer (small pairs: the largest of the
// three tilings; others: WG_BLOCKS * X6_OCC_MAX slabs, WK_B16DMA's one per CU
// included)
inline size_t wgrad_workspace_bytes(int64_t N, int Cin, int Cout, int64_t H, int64_t W) {
  if (small_pair(Cin, Cout)) {
    int64_t nblk = tiles(N, H, W, CV_FT, CV_TT);
    const int64_t ns = tiles(N, H, W, SW_RS, SW_TW), nc = tiles(N, H, W, SW_RS, SWC_TW);
    if (ns > nblk) nblk = ns;
    if (nc > nblk) nblk = nc;
    const int nout = Cout * Cin * 9 + Cout;
    return (size_t)sat_mul(nblk, nout, sizeof(float)) + (size_t)SWG_GROUPS * nout * sizeof(double) +
           16;
  }
  const int cp = wgrad_pass(Cin);
  const int ct = wgrad_ct(Cout) == 3 ? 4 : wgrad_ct(Cout);
  return (size_t)(WG_BLOCKS * X6_OCC_MAX + 2 * WG_GROUPS) * ct * 16 * (9 * cp + 1) * sizeof(float);
}

// ---------------------------------------------------------------- queries
// (include/ainp.h: each is what the route functions above answer)
inline ConvCall conv_call(bool dgrad, int64_t N, int Cin, int Cout, int64_t H, int64_t W,
                          int flags) {
  ConvCall c;
  c.dgrad = dgrad;
  c.N = N;
  // a data gradient of nn.Conv2d(Cin, Cout): the conv over dy (Cout channels)
  // producing Cin
  c.Cin = dgrad ? Cout : Cin;
  c.Cout = dgrad ? Cin : Cout;
  c.H = H;
  c.W = W;
  c.b16 = (flags & AINP_CONV_BF16) != 0;
  c.x16 = (flags & (dgrad ? AINP_CONV_DY16 : AINP_CONV_X16)) != 0;
  c.y16 = !dgrad && (flags & AINP_CONV_Y16) != 0;
  c.lay = conv_lay(flags) & (CL_X | CL_Y | CL_CF);
  return c;
}
inline WgradCall wgrad_call(int64_t N, int Cin, int Cout, int64_t H, int64_t W, int flags) {
  WgradCall c;
  c.N = N;
  c.Cin = Cin;
  c.Cout = Cout;
  c.H = H;
  c.W = W;
  c.b16 = (flags & AINP_CONV_BF16) != 0;
  c.g16 = (flags & AINP_CONV_DY16) != 0;
  c.x16 = (flags & AINP_CONV_X16) != 0;
  c.lay = conv_lay(flags) & (CL_X | CL_G);
  return c;
}
inline bool conv_shape_ok(int64_t N, int Cin, int Cout, int64_t H, int64_t W) {
  return N >= 0 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1;
}

// rows of an NCHW forward with statistics; a shape no kernel serves answers
// the 8 x 48 tiling
inline int64_t query_stat_rows(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H,
                               int64_t W, int flags) {
  ConvCall c = conv_call(false, N, Cin, Cout, H, W, flags & AINP_CONV_BF16);
  c.stats = true;
  const ConvRoute r = route_conv(env, c);
  return r.ok() ? r.rows_pad : tiles(N, H, W, CV_FT, CV_TT);
}
inline bool query_dy16_ok(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H, int64_t W) {
  const int f = AINP_CONV_BF16 | AINP_CONV_DY16;
  return conv_shape_ok(N, Cin, Cout, H, W) && wgrad_accepts(env, wgrad_call(N, Cin, Cout, H, W, f)) &&
         route_conv(env, conv_call(true, N, Cin, Cout, H, W, f)).ok();
}
inline bool query_io16_ok(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H, int64_t W) {
  const int b = AINP_CONV_BF16;
  return conv_shape_ok(N, Cin, Cout, H, W) &&
         wgrad_accepts(env, wgrad_call(N, Cin, Cout, H, W, b | AINP_CONV_X16)) &&
         route_conv(env, conv_call(false, N, Cin, Cout, H, W, b | AINP_CONV_X16 | AINP_CONV_Y16))
             .ok();
}
// Every entry point of nn.Conv2d(Cin, Cout) takes channel-last activations.
// Two conditions are not the launchers': the channel-last kernels index a
// sample with 32-bit offsets (no launcher of the small pairs checks it), and
// AINP_CONV_EXACT answers 0 for the small pairs too (their kernels would
// serve, but the model's channel-last path is all of its convs or none).
inline bool query_cl_ok(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H, int64_t W) {
  if (!conv_shape_ok(N, Cin, Cout, H, W) || env.exact ||
      !below(LIM_OFF32, H, W, Cin > Cout ? Cin : Cout, 4))
    return false;
  const int io = AINP_CONV_XCL | AINP_CONV_YCL;
  ConvCall f = conv_call(false, N, Cin, Cout, H, W, io);
  f.stats = true;
  return route_conv(env, f).ok() && route_conv(env, conv_call(true, N, Cin, Cout, H, W, io)).ok() &&
         wgrad_accepts(env, wgrad_call(N, Cin, Cout, H, W, AINP_CONV_XCL | AINP_CONV_GCL));
}
inline bool query_dgrad_cfnt_ok(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H,
                                int64_t W) {
  return conv_shape_ok(N, Cin, Cout, H, W) &&
         route_conv(env, conv_call(true, N, Cin, Cout, H, W, AINP_CONV_YCFNT)).ok();
}
// the call ainp_conv3x3_dgrad_bnr(flags, bn_flags) makes (dx == NULL: nodx)
inline ConvCall dgrad_bnr_call(int64_t N, int Cin, int Cout, int64_t H, int64_t W, int flags,
                               int bn_flags, bool nodx) {
  ConvCall c = conv_call(true, N, Cin, Cout, H, W, flags);
  c.stats = c.fused = true;
  c.bnr_y16 = (bn_flags & AINP_BN_Y16) != 0;
  c.nodx = nodx;
  return c;
}
// the shape and flag part of ainp_conv3x3_dgrad_bnr's argument check
inline bool dgrad_bnr_args_ok(int64_t N, int Cin, int Cout, int64_t H, int64_t W, int flags,
                              int bn_flags) {
  return N >= 1 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1 && N <= 65535 &&
         conv_grad_flags_ok(flags, false) && (flags & AINP_CONV_YCL) &&
         !(bn_flags & ~AINP_BN_Y16) && (Cin == 16 || Cin == 32 || Cin == 64);
}
inline bool query_dgrad_bnr_nodx_ok(const ConvEnv& env, int64_t N, int Cin, int Cout, int64_t H,
                                    int64_t W, int flags, int bn_flags) {
  return dgrad_bnr_args_ok(N, Cin, Cout, H, W, flags, bn_flags) &&
         route_conv(env, dgrad_bnr_call(N, Cin, Cout, H, W, flags, bn_flags, true)).ok();
}

}  // namespace ainp
