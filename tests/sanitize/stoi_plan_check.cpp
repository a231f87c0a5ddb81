// stoi_plan_check.cpp — csrc/stoi_plan.h (host-only C++) walked under ASan +
// UBSan: the band table against its formula, the frame count against a direct
// count at every length around the frame and hop boundaries and at the limit,
// the workspace blocks of a spread of batches (aligned, disjoint, large enough
// for what the kernels index), the refusals, and the ragged-table check on
// tables with an offender at either end of either table.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../ml-audio-inpainting_amd/csrc/stoi_plan.h"

using namespace ainp;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static void check_plan(int64_t C, int64_t R, int64_t L) {
  const StoiPlan p = stoi_plan(C, R, L);
  CHECK(p.ok);
  const int64_t K = stoi_frames(L);
  CHECK(p.frames == K && p.t_stride >= K && p.t_stride >= 2 && p.t_stride % 2 == 0);
  const int64_t segs = K - STOI_N + 1;
  CHECK(p.chunks >= 1 && p.chunks * STOI_SEG >= segs && (p.chunks - 1) * STOI_SEG < (segs > 0 ? segs : 1));
  // keep, env, part in order, 16-byte aligned, each as large as its last index needs
  CHECK(p.keep_off == 0 && p.keep_off % 16 == 0 && p.env_off % 16 == 0 && p.part_off % 16 == 0);
  CHECK(p.env_off >= p.keep_off + 4 * C * p.t_stride);
  CHECK(p.part_off >= p.env_off + 8 * (C + R) * STOI_J * p.t_stride);
  CHECK(p.bytes >= p.part_off + 8 * R * p.chunks && p.bytes % 16 == 0);
  CHECK(p.keep_lds == 8 * p.t_stride && p.keep_lds <= 64 * 1024);
}

int main() {
  for (int j = 0; j <= STOI_J; ++j) CHECK(stoi_band_edge(j) == STOI_BAND[j]);
  for (int j = 0; j < STOI_J; ++j) CHECK(STOI_BAND[j] < STOI_BAND[j + 1]);
  CHECK(STOI_BAND[STOI_J] <= STOI_NFFT / 2);
  CHECK(fabs(STOI_CLIP - (1.0 + pow(10.0, -STOI_BETA / 20.0))) < 1e-15);
  CHECK(STOI_EPS == ldexp(1.0, -52) && STOI_NFFT == 2 * STOI_NF && STOI_NF == 2 * STOI_HOP);

  for (int64_t L = 0; L <= 2000; ++L) {
    int64_t k = 0;
    while (k * STOI_HOP + STOI_NF <= L) ++k;
    CHECK(stoi_frames(L) == k);
  }
  CHECK(stoi_frames(255) == 0 && stoi_frames(256) == 1 && stoi_frames(3840) == 29);
  CHECK(stoi_frames(3968) == 30 && stoi_frames(4095) == 30 && stoi_frames(4096) == 31);
  CHECK(stoi_frames(4224) == 32 && stoi_frames(8000) == 61 && stoi_frames(STOI_MAX_LEN) == 8191);
  CHECK(STOI_MAX_LEN >= 60 * STOI_FS);

  const int64_t lens[] = {0, 1, 255, 256, 383, 384, 3840, 3968, 4095, 4096, 4224, 8000, 9000,
                          50000, 600000, STOI_MAX_LEN - 1, STOI_MAX_LEN};
  for (int64_t L : lens)
    for (int64_t C : {0, 1, 3, 9})
      for (int64_t R : {0, 1, 7, 900}) check_plan(C, R, L);
  for (int64_t K = 28; K < 200; ++K) check_plan(2, 5, (K - 1) * STOI_HOP + STOI_NF);
  CHECK(!stoi_plan(-1, 0, 100).ok && !stoi_plan(0, -1, 100).ok && !stoi_plan(1, 1, -1).ok);
  CHECK(!stoi_plan(1, 1, STOI_MAX_LEN + 1).ok && !stoi_plan((int64_t)1 << 31, 1, 100).ok);
  CHECK(!stoi_plan(1, (int64_t)1 << 31, 100).ok);

  std::vector<int32_t> n = {9000, 255, 4096}, row = {2, 0, 0, 1, 2, 2, 0};
  int64_t longest = -1;
  CHECK(stoi_check_tables(n.data(), 3, row.data(), 7, 9000, &longest) == 0 && longest == 9000);
  CHECK(stoi_check_tables(n.data(), 3, row.data(), 7, 8999, nullptr) == 1);   // over the stride
  n[2] = -1;
  CHECK(stoi_check_tables(n.data(), 3, row.data(), 7, 9000, nullptr) == 3);
  n[2] = 4096;
  row[0] = 3;
  CHECK(stoi_check_tables(n.data(), 3, row.data(), 7, 9000, nullptr) == 4);
  row[0] = 2;
  row[6] = -1;
  CHECK(stoi_check_tables(n.data(), 3, row.data(), 7, 9000, nullptr) == 10);
  row[6] = 0;
  n[1] = (int32_t)STOI_MAX_LEN + 1;
  CHECK(stoi_check_tables(n.data(), 3, row.data(), 7, (int64_t)1 << 21, nullptr) == 2);
  std::vector<int32_t> none;
  CHECK(stoi_check_tables(none.data(), 0, none.data(), 0, 0, &longest) == 0 && longest == 0);
  CHECK(stoi_check_tables(none.data(), 0, row.data(), 1, 0, nullptr) == 1);   // no clean row to name
  printf("stoi_plan_check OK\n");
  return 0;
}
