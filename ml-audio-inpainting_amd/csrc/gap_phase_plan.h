// gap_phase_plan.h — what the gap-constrained Griffin-Lim kernel (gap_phase.hip)
// decides on the host: which frames of a masked signal are unreliable, the runs
// they form, and for a run of R frames the waves of its workgroup, the LDS
// layout and where the per-frame state (tprev and the target magnitudes) lives.
// Plain C++17, no HIP: the launcher, the host queries (ainp_gap_phase_plan,
// ainp_gap_phase_workspace) and ainp/gap_phase.py state the same rule.
//
// Frames are librosa's (center, zero padding): frame t holds the samples
// [t hop - n_fft/2, t hop + n_fft/2) of the signal, T = 1 + S / hop frames.  The
// periodic Hann window of win_length samples sits at (n_fft - win_length) / 2 of
// the frame, as ainp_stft takes it.  Frame t is unreliable when one of the
// win_length samples under its window is missing (padding is reliable); a
// maximal set of consecutive unreliable frames is a run.
//
// One workgroup of `waves` waves owns a run.  In LDS for the whole iteration
// loop, in this order (every block 16-byte aligned):
//   ct     n_fft/4 + 1 doubles      quarter wave of the twiddles
//   w      n_fft doubles            the window
//   y      L doubles                the run's span, L = (R - 1) hop + n_fft
//   num    L doubles                overlap-add numerator
//   rpart  R doubles                a frame's share of resid^2
//   scr    waves x 2 x P doubles    a wave's split re / im arrays, P = N + N/32
//                                   for N = n_fft/2 (the skew of sp_pad)
//   mk     L bytes                  1: a missing sample this run fills
// and, on AINP_GP_LDS only (else in the run's slice of the global workspace),
//   tp     R x 2 x SL complex doubles   tprev in the lanes' slot order
//   am     R x SL float2                target magnitudes, the same order
//   nyq    R floats                     the Nyquist bin's magnitude
// with SL = 64 max(1, n_fft / 256) slots a frame (slot p: bins p and N - p).
// waves: the largest of 8, 4, 2, 1 whose fixed part fits in 160 KB, halved
// while half of them still take every frame of the run in one round.  A run whose
// fixed part does not fit with one wave is longer than the cap and is refused.
// A launch over several runs takes the plan of its longest one.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/ainp.h"

namespace ainp {

constexpr int GP_WAVES_MAX = 8;
constexpr int64_t GP_LDS_MAX = 160 * 1024;  // gfx950: one workgroup may take the whole CU's LDS
constexpr int GP_ITER_MAX = 1000;

inline int64_t gp_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

struct GpLayout {   // byte offsets into the dynamic LDS (tp, am, nyq: or into a run's workspace)
  int ct, w, y, num, rpart, scr, mk, tp, am, nyq;
  int scr_len;      // doubles of one re (or im) array
};

struct GpPlan {
  int ok;             // 0: refused; nothing else is meaningful
  int waves;
  int residency;      // AINP_GP_LDS / AINP_GP_WORKSPACE
  int slots;          // SL
  int64_t span;       // L
  int64_t lds_bytes;  // dynamic LDS of the workgroup
  int64_t state_bytes;   // tp + am + nyq of one run
  GpLayout lay;
};

// n_fft a power of two in [16, 2048], 1 <= win_length <= n_fft, hop >= 1, and a
// periodic Hann window whose steady-state sum of squares over the frames has no
// zero: sum_j w^2[r + j hop] > 0 for every residue r of hop
inline bool gp_shape_ok(int n_fft, int hop, int win_length) {
  if (n_fft < 16 || n_fft > 2048 || (n_fft & (n_fft - 1))) return false;
  if (win_length < 1 || win_length > n_fft || hop < 1) return false;
  // hann(j) > 0 for 0 < j < win_length.  hop >= win_length: residue 0 has w[0] = 0
  // alone.  hop < win_length: residue 0 has j = hop, every other r has j = r.
  return hop < win_length;
}

inline GpPlan gp_plan(int n_fft, int hop, int64_t R) {
  GpPlan p = {};
  if (n_fft < 16 || n_fft > 2048 || (n_fft & (n_fft - 1)) || hop < 1 || R < 1) return p;
  if ((R - 1) * (int64_t)hop + n_fft > GP_LDS_MAX) return p;
  const int N = n_fft / 2;
  const int64_t L = (R - 1) * (int64_t)hop + n_fft;
  const int64_t P = gp_up(N + (N >> 5), 2);
  p.slots = 64 * (n_fft / 256 > 1 ? n_fft / 256 : 1);
  p.span = L;
  auto fixed = [&](int waves, GpLayout& l) {
    int64_t o = 0;
    l.ct = (int)o;    o += 8 * gp_up(n_fft / 4 + 1, 2);
    l.w = (int)o;     o += 8 * (int64_t)n_fft;
    l.y = (int)o;     o += 8 * gp_up(L, 2);
    l.num = (int)o;   o += 8 * gp_up(L, 2);
    l.rpart = (int)o; o += 8 * gp_up(R, 2);
    l.scr = (int)o;   o += 8 * 2 * P * waves;
    l.mk = (int)o;    o += gp_up(L, 16);
    l.scr_len = (int)P;
    return o;
  };
  int waves = GP_WAVES_MAX;
  int64_t fix = 0;
  for (;; waves >>= 1) {
    fix = fixed(waves, p.lay);
    if (fix <= GP_LDS_MAX) break;
    if (waves == 1) return p;   // longer than the cap
  }
  while (waves > 1 && waves / 2 >= R) waves >>= 1;
  fix = fixed(waves, p.lay);
  const int64_t tp_b = R * 2 * p.slots * 16, am_b = R * p.slots * 8, nyq_b = gp_up(R * 4, 16);
  p.state_bytes = tp_b + am_b + nyq_b;
  p.waves = waves;
  p.residency = fix + p.state_bytes <= GP_LDS_MAX ? AINP_GP_LDS : AINP_GP_WORKSPACE;
  const int64_t base = p.residency == AINP_GP_LDS ? fix : 0;
  p.lay.tp = (int)base;
  p.lay.am = (int)(base + tp_b);
  p.lay.nyq = (int)(base + tp_b + am_b);
  p.lds_bytes = p.residency == AINP_GP_LDS ? fix + p.state_bytes : fix;
  p.ok = 1;
  return p;
}

// the most frames a run may have at (n_fft, hop)
inline int64_t gp_run_cap(int n_fft, int hop) {
  int64_t lo = 0, hi = GP_LDS_MAX;   // gp_plan(lo) ok (or lo == 0), gp_plan(hi) refused
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) / 2;
    if (gp_plan(n_fft, hop, mid).ok) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The runs of unreliable frames of mask[0 .. S) (1 = reliable), ascending.
// Returns their number, or -1 for a refused shape and -2 for a run over the cap;
// at most max_runs are written.
inline int64_t gp_find_runs(const uint8_t* mask, int64_t S, int n_fft, int hop, int win_length,
                            AinpGapPhaseRun* runs, int64_t max_runs) {
  if (!gp_shape_ok(n_fft, hop, win_length) || S < 0 || S > 0x7fffffff || (!mask && S > 0))
    return -1;
  std::vector<int64_t> miss((size_t)S + 1);   // missing samples before s
  miss[0] = 0;
  for (int64_t s = 0; s < S; ++s) miss[s + 1] = miss[s] + (mask[s] ? 0 : 1);
  const int64_t T = 1 + S / hop, off = (n_fft - win_length) / 2 - n_fft / 2;
  int64_t count = 0, first = -1;
  for (int64_t t = 0; t <= T; ++t) {
    bool bad = false;
    if (t < T) {
      int64_t a = t * hop + off, b = a + win_length;
      a = a < 0 ? 0 : a;
      b = b > S ? S : b;
      bad = b > a && miss[b] > miss[a];
    }
    if (bad && first < 0) first = t;
    if (!bad && first >= 0) {
      const GpPlan p = gp_plan(n_fft, hop, t - first);
      if (!p.ok) return -2;
      if (count < max_runs && runs) {
        AinpGapPhaseRun& r = runs[count];
        r.first_frame = first;
        r.n_frames = t - first;
        r.span_start = first * hop - n_fft / 2;
        r.span = p.span;
        r.residency = p.residency;
        r.waves = p.waves;
      }
      ++count;
      first = -1;
    }
  }
  return count;
}

}  // namespace ainp
