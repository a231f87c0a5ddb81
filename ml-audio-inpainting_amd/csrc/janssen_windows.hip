// janssen_windows.hip — the two streams around ainp_janssen_ex that make the
// window-wise Janssen rows (janssen_hann / janssen_rect / janssen_tukey of
// models/AudioReg/train.m:146-172, utils/segmentation_inp.m): the gather that
// cuts every window with missing samples out of its signal, and the
// overlap-add that puts the gap samples of the solved windows back.  Float64.
//
// The support of a gap is `sup_len` samples of its signal from `origin` (which
// may lie before the signal: those samples read as zeros), zero-padded to the
// circular length L = S * a.  Window s holds the circular indices
// (s * a - floor(w / 2) + i) mod L, i < w.  Both kernels are memory-bound
// streams: lane i of a workgroup touches element base + i, 8 bytes a lane, the
// per-row table entries are uniform over the workgroup (scalar loads).
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
// gap_tab[g]: one gap of one signal under one window shape
struct JwGap {
  int32_t h;         // missing samples
  int32_t c0;        // support index of the first one
  int32_t L;         // circular length of its support
  int32_t row0;      // its windows with a row: row0 .. row0 + n_rows - 1,
  int32_t n_rows;    //   ascending window index
  int32_t shape;
};

__device__ __forceinline__ int jw_mod(int v, int L) {
  const int r = v % L;
  return r < 0 ? r + L : r;
}

__global__ __launch_bounds__(JW_THREADS) void janssen_windows_kernel(
    const double* __restrict__ signals, int64_t total, const int64_t* __restrict__ sig_off,
    const JwRow* __restrict__ row_tab, const int32_t* __restrict__ gap_start,
    const int32_t* __restrict__ gap_len, int w, int a, const double* __restrict__ gana,
    int n_shapes, double* __restrict__ sol, int64_t stride) {
  const int64_t r = blockIdx.x;
  const int i = blockIdx.y * JW_THREADS + threadIdx.x;
  if (i >= w) return;
  const JwRow t = row_tab[r];
  const int64_t off = sig_off[r];
  const int gs = gap_start[r], gl = gap_len[r];
  double v = 0.0;
  // a row whose table entries make no sense is written as zeros
  const bool row_ok = t.L >= w && t.sup_len >= 0 && t.sup_len <= t.L && t.win >= 0 &&
                      (int64_t)t.win * a < t.L && t.shape >= 0 && t.shape < n_shapes &&
                      t.sig_len >= 0 && off >= 0 && off + t.sig_len <= total;
  if (row_ok && !(i >= gs && i - gs < gl)) {
    const int c = jw_mod(t.win * a - w / 2 + i, t.L);
    const int64_t s = (int64_t)t.origin + c;
    if (c < t.sup_len && s >= 0 && s < t.sig_len)
      v = signals[off + s] * gana[(int64_t)t.shape * w + i];
  }
  sol[r * stride + i] = v;
}

// grid: (gap, iteration or the final iterate, chunk of the gap)
__global__ __launch_bounds__(JW_THREADS) void janssen_ola_kernel(
    const double* __restrict__ sol, int64_t n_rows, int64_t stride,
    const double* __restrict__ row_history, int maxit, int64_t hist_stride,
    const JwRow* __restrict__ row_tab, const int32_t* __restrict__ gap_start,
    const int32_t* __restrict__ gap_len, const int64_t* __restrict__ gap_off,
    const JwGap* __restrict__ gap_tab, int w, int a, const double* __restrict__ gana,
    const double* __restrict__ gsyn, int n_shapes, double* __restrict__ signals, int64_t total,
    double* __restrict__ history, int64_t out_stride) {
  const int64_t g = blockIdx.x;
  const JwGap t = gap_tab[g];
  const int j = blockIdx.z * JW_THREADS + threadIdx.x;
  // blockIdx.y < maxit: that column of the history; the last one: the final iterate
  const int it = blockIdx.y;
  const bool final_ = !history || it == maxit;
  if (j >= t.h) return;
  const int64_t off = gap_off[g];
  if (t.L < w || t.L % a || t.c0 < 0 || (int64_t)t.c0 + t.h > t.L || t.shape < 0 ||
      t.shape >= n_shapes || t.row0 < 0 || t.n_rows < 0 || (int64_t)t.row0 + t.n_rows > n_rows ||
      off < 0 || off + t.h > total || (!final_ && t.h > out_stride))
    return;
  const double* ga = gana + (int64_t)t.shape * w;
  const double* gy = gsyn + (int64_t)t.shape * w;
  const int c = t.c0 + j;
  // every window that covers the sample counts, also those without a row
  // (all of their samples are missing and they add zeros to the sum)
  double rescale = 0.0;
  const int S = t.L / a;
  for (int s = 0; s < S; ++s) {
    const int i = jw_mod(c - s * a + w / 2, t.L);
    if (i < w) rescale += ga[i] * gy[i];
  }
  double acc = 0.0;
  for (int k = 0; k < t.n_rows; ++k) {
    const int64_t r = t.row0 + k;
    const int i = jw_mod(c - row_tab[r].win * a + w / 2, t.L);
    const int q = i - gap_start[r];
    if (i >= w || q < 0 || q >= gap_len[r] || q >= JN_HMAX) continue;
    const double z = final_ ? sol[r * stride + i]
                            : (q < hist_stride ? row_history[(r * maxit + it) * hist_stride + q]
                                               : 0.0);
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

static bool jw_shape_ok(int w, int a, int n_shapes) {
  return w >= 2 && w <= JN_NMAX && a >= 1 && w % a == 0 && w / a >= 2 && n_shapes >= 1;
}

extern "C" int ainp_janssen_windows(const double* signals, int64_t total, const int64_t* sig_off,
                                    const int32_t* row_tab, const int32_t* gap_start,
                                    const int32_t* gap_len, int64_t n_rows, int w, int a,
                                    const double* gana, int n_shapes, double* sol, int64_t stride,
                                    void* stream) {
  if (!signals || !sig_off || !row_tab || !gap_start || !gap_len || !gana || !sol || total < 1 ||
      n_rows < 0)
    return record_msg("ainp_janssen_windows: bad argument");
  if (!jw_shape_ok(w, a, n_shapes))
    return record_msg("ainp_janssen_windows: bad argument (a divides w, w / a >= 2, "
                      "2 <= w <= 16384, n_shapes >= 1)");
  if (stride < w) return record_msg("ainp_janssen_windows: bad argument (stride >= w)");
  if (n_rows > 0x7fffffff) return record_msg("ainp_janssen_windows: too many rows");
  if (n_rows == 0) return AINP_OK;
  hipLaunchKernelGGL(janssen_windows_kernel,
                     dim3((unsigned)n_rows, (unsigned)cdiv(w, JW_THREADS)), dim3(JW_THREADS), 0,
                     as_stream(stream), signals, total, sig_off,
                     reinterpret_cast<const JwRow*>(row_tab), gap_start, gap_len, w, a, gana,
                     n_shapes, sol, stride);
  return check_launch("ainp_janssen_windows");
}

extern "C" int ainp_janssen_ola(const double* sol, int64_t n_rows, int64_t stride,
                                const double* row_history, int maxit, int64_t hist_stride,
                                const int32_t* row_tab, const int32_t* gap_start,
                                const int32_t* gap_len, const int64_t* gap_off,
                                const int32_t* gap_tab, int64_t n_gaps, int h_max, int w, int a,
                                const double* gana, const double* gsyn, int n_shapes,
                                double* signals, int64_t total, double* history,
                                int64_t out_stride, void* stream) {
  if (!sol || !row_tab || !gap_start || !gap_len || !gap_off || !gap_tab || !gana || !gsyn ||
      !signals || total < 1 || n_rows < 0 || n_gaps < 0)
    return record_msg("ainp_janssen_ola: bad argument");
  if (!jw_shape_ok(w, a, n_shapes))
    return record_msg("ainp_janssen_ola: bad argument (a divides w, w / a >= 2, "
                      "2 <= w <= 16384, n_shapes >= 1)");
  if (stride < w) return record_msg("ainp_janssen_ola: bad argument (stride >= w)");
  if (h_max < 1 || h_max > JN_HMAX)
    return record_msg("ainp_janssen_ola: bad argument (1 <= h_max <= 2048)");
  if ((history != nullptr) != (row_history != nullptr))
    return record_msg("ainp_janssen_ola: bad argument (history needs row_history and the "
                      "reverse)");
  if (history && (maxit < 1 || maxit > JN_ITMAX || hist_stride < 1 || out_stride < h_max))
    return record_msg("ainp_janssen_ola: bad argument (1 <= maxit <= 1000, hist_stride >= 1, "
                      "out_stride >= h_max)");
  if (n_gaps > 0x7fffffff || n_rows > 0x7fffffff)
    return record_msg("ainp_janssen_ola: too many gaps or rows");
  if (n_gaps == 0) return AINP_OK;
  const unsigned ny = history ? (unsigned)maxit + 1u : 1u;
  hipLaunchKernelGGL(janssen_ola_kernel,
                     dim3((unsigned)n_gaps, ny, (unsigned)cdiv(h_max, JW_THREADS)),
                     dim3(JW_THREADS), 0, as_stream(stream), sol, n_rows, stride, row_history,
                     history ? maxit : 0, hist_stride, reinterpret_cast<const JwRow*>(row_tab),
                     gap_start, gap_len, gap_off, reinterpret_cast<const JwGap*>(gap_tab), w, a,
                     gana, gsyn, n_shapes, signals, total, history, out_stride);
  return check_launch("ainp_janssen_ola");
}

// ---------------------------------------------------------------- any mask
// The same two streams for segmentation_inp.m on a whole signal with any
// pattern of missing samples (ainp.janssen.janssen_windowed_mask): the support
// is the signal itself from its first sample, zero-padded to L, one fixed grid
// of S = L / a windows whatever the mask.  A row is a window with some, not all,
// samples missing, in any number of runs; with the wrap of the last windows to
// the head of the signal the rows of a run are no longer consecutive, so the
// overlap-add finds them through a window-to-row table.
namespace ainp {

// row_tab[r] of the mask entry points
struct JwmRow {
  int32_t sig_len;   // samples of its signal; [sig_len, L) is the padding
  int32_t L;         // circular length, a multiple of a
  int32_t win;       // window index s
  int32_t shape;     // row of gana / gsyn
};
// run_tab[g]: one run of missing samples of one signal under one window shape
struct JwmRun {
  int32_t h;         // missing samples
  int32_t c0;        // signal index of the first one
  int32_t L;         // circular length of its signal
  int32_t tab0;      // win_row[tab0 + s]: the row of window s of its (shape, signal), -1: none
  int32_t shape;
};

__global__ __launch_bounds__(JW_THREADS) void janssen_windows_mask_kernel(
    const double* __restrict__ signals, const uint8_t* __restrict__ missing, int64_t total,
    const int64_t* __restrict__ sig_off, const JwmRow* __restrict__ row_tab, int w, int a,
    const double* __restrict__ gana, int n_shapes, double* __restrict__ sol, int64_t stride) {
  const int64_t r = blockIdx.x;
  const int i = blockIdx.y * JW_THREADS + threadIdx.x;
  if (i >= w) return;
  const JwmRow t = row_tab[r];
  const int64_t off = sig_off[r];
  double v = 0.0;
  // a row whose table entries make no sense is written as zeros
  const bool row_ok = t.L >= w && t.sig_len >= 0 && t.sig_len <= t.L && t.win >= 0 &&
                      (int64_t)t.win * a < t.L && t.shape >= 0 && t.shape < n_shapes &&
                      off >= 0 && off + t.sig_len <= total;
  if (row_ok) {
    const int c = jw_mod(t.win * a - w / 2 + i, t.L);
    if (c < t.sig_len && !missing[off + c])
      v = signals[off + c] * gana[(int64_t)t.shape * w + i];
  }
  sol[r * stride + i] = v;
}

// The position of window sample i in the missing list of row r, or -1 where it
// is not in it: i - gap_start[r] for a row of one run (gap_len[r] >= 1), else a
// lower-bound search in the row's ascending miss_idx[miss_off[r] .. miss_off[r + 1]).
__device__ __forceinline__ int jwm_position(int64_t r, int i, const int32_t* __restrict__ gap_start,
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

// grid: (run, iteration or the final iterate, chunk of the run)
__global__ __launch_bounds__(JW_THREADS) void janssen_ola_mask_kernel(
    const double* __restrict__ sol, int64_t n_rows, int64_t stride,
    const double* __restrict__ row_history, int maxit, int64_t hist_stride,
    const JwmRow* __restrict__ row_tab, const int32_t* __restrict__ gap_start,
    const int32_t* __restrict__ gap_len, const int32_t* __restrict__ miss_off,
    const int32_t* __restrict__ miss_idx, int64_t n_idx, const int32_t* __restrict__ win_row,
    int64_t n_tab, const int64_t* __restrict__ run_off, const JwmRun* __restrict__ run_tab, int w,
    int a, const double* __restrict__ gana, const double* __restrict__ gsyn, int n_shapes,
    double* __restrict__ signals, int64_t total, double* __restrict__ history,
    int64_t out_stride) {
  const int64_t g = blockIdx.x;
  const JwmRun t = run_tab[g];
  const int j = blockIdx.z * JW_THREADS + threadIdx.x;
  // blockIdx.y < maxit: that column of the history; the last one: the final iterate
  const int it = blockIdx.y;
  const bool final_ = !history || it == maxit;
  if (j >= t.h) return;
  const int64_t off = run_off[g];
  // a run whose table entries make no sense is skipped
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
    const JwmRow row = row_tab[r];
    if (row.win != s || row.shape != t.shape || row.L != t.L) continue;
    double z;
    if (final_) {
      z = sol[r * stride + i];
    } else {
      const int q = jwm_position(r, i, gap_start, gap_len, miss_off, miss_idx, n_idx);
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

extern "C" int ainp_janssen_windows_mask(const double* signals, const uint8_t* missing,
                                         int64_t total, const int64_t* sig_off,
                                         const int32_t* row_tab, int64_t n_rows, int w, int a,
                                         const double* gana, int n_shapes, double* sol,
                                         int64_t stride, void* stream) {
  if (!signals || !missing || !sig_off || !row_tab || !gana || !sol || total < 1 || n_rows < 0)
    return record_msg("ainp_janssen_windows_mask: bad argument");
  if (!jw_shape_ok(w, a, n_shapes))
    return record_msg("ainp_janssen_windows_mask: bad argument (a divides w, w / a >= 2, "
                      "2 <= w <= 16384, n_shapes >= 1)");
  if (stride < w) return record_msg("ainp_janssen_windows_mask: bad argument (stride >= w)");
  if (n_rows > 0x7fffffff) return record_msg("ainp_janssen_windows_mask: too many rows");
  if (n_rows == 0) return AINP_OK;
  hipLaunchKernelGGL(janssen_windows_mask_kernel,
                     dim3((unsigned)n_rows, (unsigned)cdiv(w, JW_THREADS)), dim3(JW_THREADS), 0,
                     as_stream(stream), signals, missing, total, sig_off,
                     reinterpret_cast<const JwmRow*>(row_tab), w, a, gana, n_shapes, sol, stride);
  return check_launch("ainp_janssen_windows_mask");
}

extern "C" int ainp_janssen_ola_mask(const double* sol, int64_t n_rows, int64_t stride,
                                     const double* row_history, int maxit, int64_t hist_stride,
                                     const int32_t* row_tab, const int32_t* gap_start,
                                     const int32_t* gap_len, const int32_t* miss_off,
                                     const int32_t* miss_idx, int64_t n_idx,
                                     const int32_t* win_row, int64_t n_tab,
                                     const int64_t* run_off, const int32_t* run_tab,
                                     int64_t n_runs, int64_t h_max, int w, int a,
                                     const double* gana, const double* gsyn, int n_shapes,
                                     double* signals, int64_t total, double* history,
                                     int64_t out_stride, void* stream) {
  if (!sol || !row_tab || !gap_start || !gap_len || !miss_off || !miss_idx || !win_row ||
      !run_off || !run_tab || !gana || !gsyn || !signals || total < 1 || n_rows < 0 ||
      n_runs < 0 || n_idx < 0 || n_tab < 0)
    return record_msg("ainp_janssen_ola_mask: bad argument");
  if (!jw_shape_ok(w, a, n_shapes))
    return record_msg("ainp_janssen_ola_mask: bad argument (a divides w, w / a >= 2, "
                      "2 <= w <= 16384, n_shapes >= 1)");
  if (stride < w) return record_msg("ainp_janssen_ola_mask: bad argument (stride >= w)");
  if (h_max < 1 || h_max > total)
    return record_msg("ainp_janssen_ola_mask: bad argument (1 <= h_max <= total)");
  if ((history != nullptr) != (row_history != nullptr))
    return record_msg("ainp_janssen_ola_mask: bad argument (history needs row_history and the "
                      "reverse)");
  if (history && (maxit < 1 || maxit > JN_ITMAX || hist_stride < 1 || out_stride < h_max))
    return record_msg("ainp_janssen_ola_mask: bad argument (1 <= maxit <= 1000, hist_stride >= "
                      "1, out_stride >= h_max)");
  if (n_runs > 0x7fffffff || n_rows > 0x7fffffff || n_idx > 0x7fffffff || n_tab > 0x7fffffff ||
      cdiv(h_max, (int64_t)JW_THREADS) > 65535)
    return record_msg("ainp_janssen_ola_mask: too many runs, rows, list or table entries, or a "
                      "run too long for the grid");
  if (n_runs == 0) return AINP_OK;
  const unsigned ny = history ? (unsigned)maxit + 1u : 1u;
  hipLaunchKernelGGL(janssen_ola_mask_kernel,
                     dim3((unsigned)n_runs, ny, (unsigned)cdiv(h_max, (int64_t)JW_THREADS)),
                     dim3(JW_THREADS), 0, as_stream(stream), sol, n_rows, stride, row_history,
                     history ? maxit : 0, hist_stride, reinterpret_cast<const JwmRow*>(row_tab),
                     gap_start, gap_len, miss_off, miss_idx, n_idx, win_row, n_tab, run_off,
                     reinterpret_cast<const JwmRun*>(run_tab), w, a, gana, gsyn, n_shapes,
                     signals, total, history, out_stride);
  return check_launch("ainp_janssen_ola_mask");
}
