// stoi_plan.h — what the STOI / ESTOI kernels (stoi.hip) fix on the host: the
// constants of the measure, the band table, the frame count of a row, the
// limits, the ragged-batch tables and the workspace of a launch.  Plain C++17,
// no HIP: the launcher, the host queries (ainp_stoi_plan, ainp_stoi_workspace)
// and ainp/stoi.py state the same rule.
//
// A batch is C clean rows of lengths n[c] and R restored rows, row r scored
// against clean row clean_row[r] (any order, repeats allowed) and as long as
// that row.  Four dependent launches share one workspace (every block 16-byte
// aligned), sized by the longest row's frame count K = frames(max n):
//   keep   int32  [C][t_stride]            kept frame indices, ascending
//   env    double [C + R][J][t_stride]     band envelopes of the kept frames:
//                                          rows 0 .. C-1 clean, C .. C+R-1 restored
//   part   double [R][chunks]              a chunk's sum of d_m, m ascending
// with t_stride = K rounded up to 2 and chunks = ceil((K - N + 1) / SEG) (at
// least 1): a chunk is SEG consecutive segments whatever else the batch holds,
// so a row's sums do not depend on the batch.
//
// LDS (static but for the energies): keep holds the frame energies of its row,
// K doubles (64 KB at the row limit), beside 2 x 16 doubles of reduction
// slots; bands holds the window (256 doubles), the quarter wave (129), and per
// wave the split re / im arrays (2 x 264) and the power spectrum (257): 27 KB
// for 4 waves; score holds a chunk's X and Y windows, 2 x J x (SEG + N - 1)
// doubles, the row statistics of 16 segments (16 x 4 x 16) and SEG values
// of d_m: 31 KB.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ainp.h"

namespace ainp {

constexpr int STOI_FS = 10000;
constexpr int STOI_NF = 256;      // frame length
constexpr int STOI_HOP = 128;
constexpr int STOI_NFFT = 512;
constexpr int STOI_J = 15;        // one-third octave bands
constexpr int STOI_N = 30;        // frames per segment
constexpr double STOI_BETA = -15.0;   // dB, the clipping bound of STOI
constexpr double STOI_CLIP = 6.623413251903491;   // 1 + 10^(-BETA / 20)
constexpr double STOI_DYN = 40.0;     // dB, the silent-frame range
constexpr double STOI_EPS = 2.220446049250313e-16;   // 2^-52
constexpr double STOI_SENTINEL = 1e-5;   // the score of a row with fewer than N kept frames

// band j covers the bins [lo[j], lo[j + 1]) of the 512-point transform: the bin
// nearest 150 2^((2j - 1) / 6) Hz (stoi_band_edge states the formula)
constexpr int STOI_BAND[STOI_J + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138,
                                       174, 219};

constexpr int64_t STOI_MAX_LEN = (int64_t)1 << 20;   // samples of a row: 104.8 s at 10 kHz
constexpr int STOI_SEG = 64;          // segments of one score workgroup
constexpr int STOI_BANDS_WAVES = 4;   // frames of one bands workgroup, a wave each
constexpr int STOI_KEEP_THREADS = 1024;
constexpr int STOI_SCORE_THREADS = 256;

constexpr int64_t stoi_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

// the lower edge of band j (j = J: the upper edge of the last band) by the formula
inline int stoi_band_edge(int j) {
  const double f = 150.0 * pow(2.0, (2.0 * j - 1.0) / 6.0), df = (double)STOI_FS / STOI_NFFT;
  int best = 0;
  for (int b = 1; b <= STOI_NFFT / 2; ++b)
    if (fabs(b * df - f) < fabs(best * df - f)) best = b;
  return best;
}

// frames of a row of L samples
constexpr int64_t stoi_frames(int64_t L) { return L < STOI_NF ? 0 : (L - STOI_NF) / STOI_HOP + 1; }

struct StoiPlan {
  int ok;              // 0: refused; nothing else is meaningful
  int64_t frames;      // K of the longest row
  int64_t t_stride;
  int64_t chunks;
  int64_t keep_off, env_off, part_off;   // byte offsets into the workspace
  int64_t bytes;
  int64_t keep_lds;    // dynamic LDS of the keep launch
};

inline StoiPlan stoi_plan(int64_t C, int64_t R, int64_t max_len) {
  StoiPlan p = {};
  if (C < 0 || R < 0 || max_len < 0 || max_len > STOI_MAX_LEN || C > 0x7fffffff ||
      R > 0x7fffffff)
    return p;
  p.frames = stoi_frames(max_len);
  p.t_stride = stoi_up(p.frames > 0 ? p.frames : 1, 2);
  const int64_t segs = p.frames - STOI_N + 1;
  p.chunks = segs > 0 ? (segs + STOI_SEG - 1) / STOI_SEG : 1;
  int64_t o = 0;
  p.keep_off = o;  o += stoi_up(4 * C * p.t_stride, 16);
  p.env_off = o;   o += 8 * (C + R) * STOI_J * p.t_stride;
  p.part_off = o;  o += stoi_up(8 * R * p.chunks, 16);
  p.bytes = o;
  p.keep_lds = 8 * p.t_stride;
  p.ok = 1;
  return p;
}

// The ragged-batch tables as the host holds them: 0 when every length lies in
// [0, min(stride, STOI_MAX_LEN)] and every clean_row in [0, C); else the
// 1-based position of the first offender (rows of n first, then clean_row).
// *max_len receives the longest row.
inline int64_t stoi_check_tables(const int32_t* n, int64_t C, const int32_t* clean_row, int64_t R,
                                 int64_t stride, int64_t* max_len) {
  int64_t longest = 0;
  for (int64_t c = 0; c < C; ++c) {
    if (n[c] < 0 || n[c] > stride || n[c] > STOI_MAX_LEN) return c + 1;
    if (n[c] > longest) longest = n[c];
  }
  for (int64_t r = 0; r < R; ++r)
    if (clean_row[r] < 0 || clean_row[r] >= C) return C + r + 1;
  if (max_len) *max_len = longest;
  return 0;
}

}  // namespace ainp
