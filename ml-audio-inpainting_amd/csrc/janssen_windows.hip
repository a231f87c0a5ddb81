// janssen_windows.hip — the two streams around a window solver (ainp_janssen_ex,
// ainp_janssen_mask, ainp_spain, ainp_spain_omp) that make the window-wise
// algorithms (utils/segmentation_inp.m as models/AudioReg/train.m:146-172 drives
// it and as it is written, references/spain/spain_segmentation.m): the gather
// that cuts every window with some, not all, samples missing out of its signal,
// and the overlap-add that puts the missing samples of the solved windows back.
// Float64.  One pair of kernels for every plan; the tables are described in
// include/ainp.h.
//
// A support is `sup_len` samples of a signal from `origin` (which may lie
// before the signal: those samples read as zeros; a whole signal is its own
// support, origin 0), zero-padded to the circular length L = S * a.  Window s
// holds the circular indices (s * a - floor(w / 2) + i) mod L, i < w.  Both
// kernels are memory-bound streams: lane i of a workgroup touches element
// base + i, 8 bytes a lane, the per-row table entries are uniform over the
// workgroup (scalar loads).
#include <algorithm>

#include "ar_limits.h"
#include "common.h"

namespace ainp {

constexpr int JW_THREADS = 256;

// row_tab[r]: the window of batch row r
struct JwRow {
  int32_t sig_len;   // samples of its signal
  int32_t origin;    // signal index of support sample 0 (may be negative)
  int32_t sup_len;   // samples of the support; [sup_len, L) is the padding
  int32_t L;         // circular length, a multiple of a
  int32_t win;       // window index s
  int32_t shape;     // row of gana / gsyn
};
// unit_tab[g]: one run of missing samples of one support under one window shape
struct JwUnit {
  int32_t h;         // missing samples
  int32_t c0;        // support index of the first one
  int32_t L;         // circular length of its support
  int32_t tab0;      // win_row[tab0 + s]: the row of window s of its support, -1: none
  int32_t shape;
};

__device__ __forceinline__ int jw_mod(int v, int L) {
  const int r = v % L;
  return r < 0 ? r + L : r;
}

__global__ __launch_bounds__(JW_THREADS) void janssen_windows_kernel(
    const double* __restrict__ signals, const uint8_t* __restrict__ missing, int64_t total,
    const int64_t* __restrict__ sig_off, const JwRow* __restrict__ row_tab, int w, int a,
    const double* __restrict__ gana, int n_shapes, double* __restrict__ sol, int64_t stride) {
  const int64_t r = blockIdx.x;
  const int i = blockIdx.y * JW_THREADS + threadIdx.x;
  if (i >= w) return;
  const JwRow t = row_tab[r];
  const int64_t off = sig_off[r];
  double v = 0.0;
  // a row whose table entries make no sense is written as zeros
  const bool row_ok = t.L >= w && t.sup_len >= 0 && t.sup_len <= t.L && t.win >= 0 &&
                      (int64_t)t.win * a < t.L && t.shape >= 0 && t.shape < n_shapes &&
                      t.sig_len >= 0 && off >= 0 && off + t.sig_len <= total;
  if (row_ok) {
    const int c = jw_mod(t.win * a - w / 2 + i, t.L);
    const int64_t s = (int64_t)t.origin + c;
    if (c < t.sup_len && s >= 0 && s < t.sig_len && !missing[off + s])
      v = signals[off + s] * gana[(int64_t)t.shape * w + i];
  }
  sol[r * stride + i] = v;
}

// The position of window sample i in the missing list of row r, or -1 where it
// is not in it: i - gap_start[r] for a row of one run (gap_len[r] >= 1), else a
// lower-bound search in the row's ascending miss_idx[miss_off[r] .. miss_off[r + 1]).
__device__ __forceinline__ int jw_position(int64_t r, int i, const int32_t* __restrict__ gap_start,
                                           const int32_t* __restrict__ gap_len,
                                           const int32_t* __restrict__ miss_off,
                                           const int32_t* __restrict__ miss_idx, int64_t n_idx) {
  const int gl = gap_len[r];
  if (gl >= 1) {
    const int q = i - gap_start[r];
    return q >= 0 && q < gl && q < JN_HMAX ? q : -1;
  }
  const int64_t b = miss_off[r], e = miss_off[r + 1];
  if (b < 0 || e < b || e > n_idx || e - b > JN_HMAX) return -1;
  int lo = 0, hi = (int)(e - b);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (miss_idx[b + mid] < i) lo = mid + 1; else hi = mid;
  }
  return lo < (int)(e - b) && miss_idx[b + lo] == i ? lo : -1;
}

// grid: (unit, iteration or the final iterate, chunk of the unit)
__global__ __launch_bounds__(JW_THREADS) void janssen_ola_kernel(
    const double* __restrict__ sol, int64_t n_rows, int64_t stride,
    const double* __restrict__ row_history, int maxit, int64_t hist_stride,
    const JwRow* __restrict__ row_tab, const int32_t* __restrict__ gap_start,
    const int32_t* __restrict__ gap_len, const int32_t* __restrict__ miss_off,
    const int32_t* __restrict__ miss_idx, int64_t n_idx, const int32_t* __restrict__ win_row,
    int64_t n_tab, const int64_t* __restrict__ unit_off, const JwUnit* __restrict__ unit_tab,
    int w, int a, const double* __restrict__ gana, const double* __restrict__ gsyn, int n_shapes,
    double* __restrict__ signals, int64_t total, double* __restrict__ history,
    int64_t out_stride) {
  const int64_t g = blockIdx.x;
  const JwUnit t = unit_tab[g];
  const int j = blockIdx.z * JW_THREADS + threadIdx.x;
  // blockIdx.y < maxit: that column of the history; the last one: the final iterate
  const int it = blockIdx.y;
  const bool final_ = !history || it == maxit;
  if (j >= t.h) return;
  const int64_t off = unit_off[g];
  // a unit whose table entries make no sense is skipped
  if (t.L < w || t.L % a || t.h < 0 || t.c0 < 0 || (int64_t)t.c0 + t.h > t.L || t.shape < 0 ||
      t.shape >= n_shapes || t.tab0 < 0 || (int64_t)t.tab0 + t.L / a > n_tab || off < 0 ||
      off + t.h > total || (!final_ && t.h > out_stride))
    return;
  const double* ga = gana + (int64_t)t.shape * w;
  const double* gy = gsyn + (int64_t)t.shape * w;
  const int c = t.c0 + j;
  // the w / a windows that cover the sample are consecutive on the circle from
  // s_lo; those that wrapped past S - 1 are windows 0 .. n_wrap - 1 and come
  // first, so that both sums run in ascending window order
  const int S = t.L / a, nw = w / a;
  const int s_lo = jw_mod((c + w / 2) / a - nw + 1, S);
  const int n_wrap = s_lo + nw > S ? s_lo + nw - S : 0;
  double rescale = 0.0, acc = 0.0;
  for (int e = 0; e < nw; ++e) {
    const int s = e < n_wrap ? e : s_lo + e - n_wrap;
    const int i = jw_mod(c - s * a + w / 2, t.L);
    if (i >= w) continue;
    // every window that covers the sample counts, also those without a row
    // (all of their samples are missing and they add zeros to the sum)
    rescale += ga[i] * gy[i];
    const int64_t r = win_row[t.tab0 + s];
    if (r < 0 || r >= n_rows) continue;
    const JwRow row = row_tab[r];
    if (row.win != s || row.shape != t.shape || row.L != t.L) continue;
    double z;
    if (final_) {
      z = sol[r * stride + i];
    } else {
      const int q = jw_position(r, i, gap_start, gap_len, miss_off, miss_idx, n_idx);
      if (q < 0) continue;
      z = q < hist_stride ? row_history[(r * maxit + it) * hist_stride + q] : 0.0;
    }
    acc += z * gy[i];
  }
  const double v = acc / rescale;
  if (final_)
    signals[off + j] = v;
  else
    history[(g * maxit + it) * out_stride + j] = v;
}

}  // namespace ainp

using namespace ainp;

// the refusals the two entry points share, under the caller's name
static int jw_check(const char* fn, int w, int a, int n_shapes, int64_t stride, int64_t n_rows) {
  if (!(w >= 2 && w <= JN_NMAX && a >= 1 && w % a == 0 && w / a >= 2 && n_shapes >= 1))
    return record_bad_argument(fn, "a divides w, w / a >= 2, 2 <= w <= 16384, n_shapes >= 1");
  if (stride < w) return record_bad_argument(fn, "stride >= w");
  if (n_rows > 0x7fffffff) return record_bad_argument(fn, "at most 2^31 - 1 rows");
  return AINP_OK;
}

extern "C" int ainp_janssen_windows(const double* signals, const uint8_t* missing, int64_t total,
                                    const int64_t* sig_off, const int32_t* row_tab,
                                    int64_t n_rows, int w, int a, const double* gana,
                                    int n_shapes, double* sol, int64_t stride, void* stream) {
  if (!signals || !missing || !sig_off || !row_tab || !gana || !sol || total < 1 || n_rows < 0)
    return record_msg("ainp_janssen_windows: bad argument");
  if (const int rc = jw_check("ainp_janssen_windows", w, a, n_shapes, stride, n_rows)) return rc;
  if (n_rows == 0) return AINP_OK;
  hipLaunchKernelGGL(janssen_windows_kernel,
                     dim3((unsigned)n_rows, (unsigned)cdiv(w, JW_THREADS)), dim3(JW_THREADS), 0,
                     as_stream(stream), signals, missing, total, sig_off,
                     reinterpret_cast<const JwRow*>(row_tab), w, a, gana, n_shapes, sol, stride);
  return check_launch("ainp_janssen_windows");
}

extern "C" int ainp_janssen_ola(const double* sol, int64_t n_rows, int64_t stride,
                                const double* row_history, int maxit, int64_t hist_stride,
                                const int32_t* row_tab, const int32_t* gap_start,
                                const int32_t* gap_len, const int32_t* miss_off,
                                const int32_t* miss_idx, int64_t n_idx, const int32_t* win_row,
                                int64_t n_tab, const int64_t* unit_off, const int32_t* unit_tab,
                                int64_t n_units, int64_t h_max, int w, int a, const double* gana,
                                const double* gsyn, int n_shapes, double* signals, int64_t total,
                                double* history, int64_t out_stride, void* stream) {
  if (!sol || !row_tab || !gap_start || !gap_len || !miss_off || !miss_idx || !win_row ||
      !unit_off || !unit_tab || !gana || !gsyn || !signals || total < 1 || n_rows < 0 ||
      n_units < 0 || n_idx < 0 || n_tab < 0)
    return record_msg("ainp_janssen_ola: bad argument");
  if (const int rc = jw_check("ainp_janssen_ola", w, a, n_shapes, stride, n_rows)) return rc;
  if (h_max < 1 || h_max > total)
    return record_msg("ainp_janssen_ola: bad argument (1 <= h_max <= total)");
  if ((history != nullptr) != (row_history != nullptr))
    return record_msg("ainp_janssen_ola: bad argument (history needs row_history and the "
                      "reverse)");
  if (history && (maxit < 1 || maxit > JN_ITMAX || hist_stride < 1 || out_stride < h_max))
    return record_msg("ainp_janssen_ola: bad argument (1 <= maxit <= 1000, hist_stride >= 1, "
                      "out_stride >= h_max)");
  if (n_units > 0x7fffffff || n_idx > 0x7fffffff || n_tab > 0x7fffffff ||
      cdiv(h_max, (int64_t)JW_THREADS) > 65535)
    return record_msg("ainp_janssen_ola: too many units, list or table entries, or a unit too "
                      "long for the grid");
  if (n_units == 0) return AINP_OK;
  const unsigned ny = history ? (unsigned)maxit + 1u : 1u;
  hipLaunchKernelGGL(janssen_ola_kernel,
                     dim3((unsigned)n_units, ny, (unsigned)cdiv(h_max, (int64_t)JW_THREADS)),
                     dim3(JW_THREADS), 0, as_stream(stream), sol, n_rows, stride, row_history,
                     history ? maxit : 0, hist_stride, reinterpret_cast<const JwRow*>(row_tab),
                     gap_start, gap_len, miss_off, miss_idx, n_idx, win_row, n_tab, unit_off,
                     reinterpret_cast<const JwUnit*>(unit_tab), w, a, gana, gsyn, n_shapes,
                     signals, total, history, out_stride);
  return check_launch("ainp_janssen_ola");
}
