// spain_window.h — the window loop spain.hip and spain_omp.hip share: the row
// rule and load, record / stop, k schedule and closing; spain.hip's S-SPAIN
// objective and projection; on the host the argument check and the launcher.
#pragma once
#include <cstdio>

#include "ar_limits.h"
#include "common.h"
#include "spain_fft.h"
#include "spain_plan.h"

namespace ainp {

struct SpRow {
  double* xr;      // the iterate x-hat, in LDS
  double* x;       // the row in sol
  double* hrow;    // its objective history, or nullptr
  int32_t* arow;   // OMP: its atoms per pass, or nullptr
  int gs, gl;      // the missing run
};

// spain_omp_kernel keeps its prologue, objective and projection in its own text:
// its 256-lane register allocation is fragile (shared pieces).

// The run lies in the window; a row whose run does not is closed and left alone.
__device__ __forceinline__ bool sp_run_ok(int gs, int gl, int w) {
  return !(gs < 0 || gl < 1 || gl > JN_HMAX || (int64_t)gs + gl > w);
}

// iters and the tails of the histories after `done` passes
template <int NT>
__device__ __forceinline__ void sp_row_close(int32_t* iters, double* hrow, int32_t* arow, int done,
                                             int maxit, int tid) {
  if (tid == 0) iters[blockIdx.x] = done;
  for (int i = done + tid; i < maxit; i += NT) {
    if (hrow) hrow[i] = NAN;
    if (arow) arow[i] = -1;
  }
}

// The quarter wave and the row with the run zeroed; ends on a barrier.
template <int NT>
__device__ __forceinline__ void sp_row_load(const SpRow& R, double* ct, int w, int M, int tid) {
  sp_quarter_wave<NT>(ct, M, tid);
  for (int i = tid; i < w; i += NT) R.xr[i] = (i >= R.gs && i - R.gs < R.gl) ? 0.0 : R.x[i];
  __syncthreads();
}

// A lane's part of |A* z-bar - x-hat|^2, A* z-bar / inv in the transform buffer
template <int NT, int TPL>
__device__ __forceinline__ double sp_residual2(const SpFft& f, const SpRow& R, int w, double inv,
                                               int tid) {
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < TPL; ++e) {
    const int n = tid + e * NT;
    if (n >= f.N || 2 * n >= w) continue;
    const cplx c = f.ld(n);
    const double d0 = c.re * inv - R.xr[2 * n], d1 = c.im * inv - R.xr[2 * n + 1];
    acc += d0 * d0 + d1 * d1;
  }
  return acc;
}

// Pass cnt's objective (and atom count) into the histories; the smallest so far
// records the iterate it was evaluated on.  True: stop.  No barrier.
template <int NT>
__device__ __forceinline__ bool sp_record(const SpRow& R, double obj, int cnt, int na, double& best,
                                          double epsilon, int tid) {
  if (tid == 0) {
    if (R.hrow) R.hrow[cnt - 1] = obj;
    if (R.arow) R.arow[cnt - 1] = na;
  }
  if (obj <= best) {
    best = obj;
    for (int i = tid; i < R.gl; i += NT) R.x[R.gs + i] = R.xr[R.gs + i];
  }
  return obj <= epsilon;
}

// x-hat = proj(x_e + u);  u += x_e - x-hat, a lane on its own sample pairs; barrier
template <int NT, int TPL>
__device__ __forceinline__ void sp_project_dual(const SpFft& f, const SpRow& R, int w, double inv,
                                                double (&ut)[TPL][2], int tid) {
#pragma unroll
  for (int e = 0; e < TPL; ++e) {
    const int n = tid + e * NT;
    if (n >= f.N || 2 * n >= w) continue;
    const cplx c = f.ld(n);
    const double xe[2] = {c.re * inv, c.im * inv};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = 2 * n + h;
      if (t >= R.gs && t - R.gs < R.gl) R.xr[t] = xe[h] + ut[e][h];
      ut[e][h] += xe[h] - R.xr[t];
    }
  }
  __syncthreads();
}

// k grows by s every r passes
__device__ __forceinline__ void sp_next_pass(int& cnt, int& k, int s_step, int r_rate) {
  ++cnt;
  if (cnt % r_rate == 0) k += s_step;
}

// ---- host
// The arguments the window solvers share, in the order they are refused; fn
// names the entry point, pointers_ok: sol, gap_start, gap_len and iters are set.
inline int sp_check_window_args(const char* fn, bool pointers_ok, int64_t n_rows, int64_t stride,
                                int w, int red, bool alg_ok, int s, int r, double epsilon,
                                int maxit) {
  if (!pointers_ok || n_rows < 0) return record_bad_argument(fn);
  if (!alg_ok) return record_bad_argument(fn, "algorithm is AINP_SPAIN_A or AINP_SPAIN_S");
  if (!sp_shape_ok(w, red)) return record_bad_argument(fn, SP_SHAPE_RULE);
  if (stride < w) return record_bad_argument(fn, "stride >= w");
  if (s < 1 || r < 1) return record_bad_argument(fn, "s >= 1, r >= 1");
  if (maxit < 1 || maxit > red * w / 2 + 1)
    return record_bad_argument(fn, "1 <= maxit <= red * w / 2 + 1");
  if (!(epsilon >= 0.0)) return record_bad_argument(fn, "epsilon >= 0");
  return AINP_OK;
}

// One workgroup of NT lanes per row, `lds` bytes of dynamic LDS; the limit is set once.
template <auto Kernel, int NT, typename... Args>
static int sp_launch_rows(const char* fn, size_t lds_max, size_t lds, int64_t n_rows, void* stream,
                          Args... args) {
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_max) == hipSuccess;
  if (!lds_ok) {
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: cannot reserve the transform's LDS", fn);
    return record_msg(msg);
  }
  hipLaunchKernelGGL(Kernel, dim3((unsigned)n_rows), dim3(NT), lds, as_stream(stream), args...);
  return check_launch(fn);
}

}  // namespace ainp
