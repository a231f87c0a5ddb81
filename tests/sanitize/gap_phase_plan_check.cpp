// gap_phase_plan_check.cpp — csrc/gap_phase_plan.h (host-only C++) walked under
// ASan + UBSan: over every n_fft, a spread of hops and every run length up to
// past the cap, the plan's LDS blocks are 16-byte aligned, do not overlap and
// end inside 160 KB, the workspace slice holds what LDS does not, and the cap
// is where the plan first refuses; the run finder against the definition taken
// sample by sample on masks with gaps at both ends, everywhere and nowhere.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../ml-audio-inpainting_amd/csrc/gap_phase_plan.h"

using namespace ainp;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static void check_plan(int n_fft, int hop, int64_t R) {
  const GpPlan p = gp_plan(n_fft, hop, R);
  if (!p.ok) return;
  const int N = n_fft / 2;
  const int64_t L = (R - 1) * hop + n_fft;
  CHECK(p.span == L && p.slots >= N / 2 && p.slots % 64 == 0);
  CHECK(p.waves >= 1 && p.waves <= GP_WAVES_MAX && (p.waves == 1 || p.waves / 2 < R));
  const GpLayout& l = p.lay;
  CHECK(l.scr_len >= N + (N >> 5));
  // fixed blocks in order, each ending at or before the next one starts
  const int64_t start[] = {l.ct, l.w, l.y, l.num, l.rpart, l.scr, l.mk};
  const int64_t size[] = {8 * (int64_t)(n_fft / 4 + 1), 8 * (int64_t)n_fft, 8 * L, 8 * L, 8 * R,
                          8 * 2 * (int64_t)l.scr_len * p.waves, L};
  int64_t end = 0;
  for (int i = 0; i < 7; ++i) {
    CHECK(start[i] % 16 == 0 && start[i] >= end);
    end = start[i] + size[i];
  }
  const int64_t tp_b = R * 2 * p.slots * 16, am_b = R * p.slots * 8, nyq_b = R * 4;
  CHECK(l.tp % 16 == 0 && l.am >= l.tp + tp_b && l.nyq >= l.am + am_b);
  if (p.residency == AINP_GP_LDS) {
    CHECK(l.tp >= end);
    CHECK(l.nyq + nyq_b <= p.lds_bytes);
  } else {
    CHECK(p.residency == AINP_GP_WORKSPACE && l.tp == 0);
    CHECK(end <= p.lds_bytes && l.nyq + nyq_b <= p.state_bytes && p.state_bytes % 16 == 0);
  }
  CHECK(p.lds_bytes <= GP_LDS_MAX);
}

static void check_runs(const std::vector<uint8_t>& m, int n_fft, int hop, int win) {
  const int64_t S = (int64_t)m.size(), T = 1 + S / hop;
  std::vector<AinpGapPhaseRun> runs((size_t)T + 1);
  const int64_t n = gp_find_runs(m.data(), S, n_fft, hop, win, runs.data(), (int64_t)runs.size());
  CHECK(n >= 0);
  CHECK(gp_find_runs(m.data(), S, n_fft, hop, win, nullptr, 0) == n);
  std::vector<char> bad((size_t)T, 0);
  for (int64_t t = 0; t < T; ++t)
    for (int64_t s = t * hop - n_fft / 2 + (n_fft - win) / 2, e = s + win; s < e; ++s)
      if (s >= 0 && s < S && !m[(size_t)s]) bad[(size_t)t] = 1;
  std::vector<char> got((size_t)T, 0);
  int64_t prev_end = -1;
  for (int64_t i = 0; i < n; ++i) {
    const AinpGapPhaseRun& r = runs[(size_t)i];
    CHECK(r.first_frame > prev_end && r.n_frames >= 1 && r.first_frame + r.n_frames <= T);
    CHECK(r.span_start == r.first_frame * hop - n_fft / 2);
    CHECK(r.span == (r.n_frames - 1) * hop + n_fft);
    for (int64_t t = r.first_frame; t < r.first_frame + r.n_frames; ++t) got[(size_t)t] = 1;
    prev_end = r.first_frame + r.n_frames;   // a reliable frame lies between two runs
  }
  CHECK(got == bad);
}

int main() {
  for (int n_fft = 16; n_fft <= 2048; n_fft *= 2)
    for (int hop : {1, 3, n_fft / 8, n_fft / 4, n_fft / 2, n_fft - 1}) {
      if (hop < 1) continue;
      const int64_t cap = gp_run_cap(n_fft, hop);
      CHECK(cap >= 1 && gp_plan(n_fft, hop, cap).ok && !gp_plan(n_fft, hop, cap + 1).ok);
      for (int64_t R = 1; R <= cap + 2; R = R < 70 ? R + 1 : R + R / 7) check_plan(n_fft, hop, R);
      check_plan(n_fft, hop, cap);
    }
  CHECK(!gp_plan(48, 16, 4).ok && !gp_plan(8, 2, 4).ok && !gp_plan(4096, 512, 4).ok);
  CHECK(!gp_plan(64, 0, 4).ok && !gp_plan(64, 16, 0).ok && !gp_plan(64, 16, (int64_t)1 << 40).ok);
  CHECK(gp_shape_ok(64, 16, 48) && !gp_shape_ok(64, 48, 48) && !gp_shape_ok(64, 16, 65));
  CHECK(!gp_shape_ok(64, 0, 64) && !gp_shape_ok(48, 16, 48) && !gp_shape_ok(64, 16, 0));

  const int S = 1000;   // not a multiple of the hops below
  for (int win : {48, 64})
    for (int hop : {16, 24}) {
      std::vector<uint8_t> m((size_t)S, 1);
      check_runs(m, 64, hop, win);
      auto gap = [&](int a, int b) { for (int s = a; s < b; ++s) m[(size_t)s] = 0; };
      gap(0, 1);
      check_runs(m, 64, hop, win);
      gap(S - 1, S);
      check_runs(m, 64, hop, win);
      gap(300, 420);
      gap(440, 441);
      gap(700, 710);
      check_runs(m, 64, hop, win);
      std::fill(m.begin(), m.end(), 0);
      check_runs(m, 64, hop, win);
    }
  std::vector<uint8_t> empty;
  CHECK(gp_find_runs(empty.data(), 0, 64, 16, 48, nullptr, 0) == 0);
  std::vector<uint8_t> big(16000, 1);
  for (int s = 1000; s < 1000 + 68 * 128; ++s) big[(size_t)s] = 0;
  CHECK(gp_find_runs(big.data(), (int64_t)big.size(), 512, 128, 512, nullptr, 0) == -2);
  CHECK(gp_find_runs(big.data(), (int64_t)big.size(), 512, 512, 512, nullptr, 0) == -1);
  printf("gap_phase_plan_check OK\n");
  return 0;
}
