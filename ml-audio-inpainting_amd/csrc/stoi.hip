// stoi.hip — STOI and ESTOI of a ragged batch (include/ainp.h: ainp_stoi): C
// clean rows, R restored rows each scored against one of them, float64, four
// dependent launches on the caller's stream (stoi_plan.h lays out the
// workspace they share):
//
//   keep    one workgroup of 16 waves per clean row.  A wave takes a frame at a
//           time: windowed energy by a butterfly sum, e[k] into LDS; then the
//           maximum, the threshold and an order-preserving compaction by wave
//           ballots into the keep list, giving T[c].
//   bands   grid (row of x or y, 4 kept frames); one wave per frame.  Frame t
//           of the silence-removed signal is formed straight from the source
//           row through the keep list (the frame itself plus the half of each
//           neighbour that overlaps it), windowed again, transformed by the
//           half-length complex scheme of spain_fft.h (a 256-point transform on
//           split, skewed re / im arrays, wave-level barriers), and its 15 band
//           sums are taken over ascending bins by lanes 0 .. 14.
//   score   grid (restored row, chunk of 64 segments).  The chunk's 15 x 93
//           windows of X and Y sit in LDS; 16 lanes take one segment (lane l:
//           band l, and for ESTOI then columns l and l + 16), 16 segments a
//           round.  d_m by a fixed butterfly over the 16 lanes; the chunk's sum
//           over ascending m by one thread.
//   finish  a thread per restored row: the chunk sums in ascending order over
//           M, or the sentinel for T < N.
//
// No floating-point atomics and no order that depends on the batch: a row's
// score is the same bits alone or in any batch, on every launch.
#include "common.h"
#include "spain_fft.h"
#include "stoi_plan.h"

namespace ainp {

constexpr int ST_P = STOI_NF + (STOI_NF >> 5);        // a skewed re (or im) array of 256 cells
constexpr int ST_W = STOI_SEG + STOI_N - 1;           // frames under a chunk's segments

__device__ __forceinline__ double st_window(int i) {
  return 0.5 * (1.0 - cospi((double)(2 * (i + 1)) / (double)(STOI_NF + 1)));
}
// the length the kernels take for clean row c: the table's, clamped to the row
__device__ __forceinline__ int64_t st_len(const int32_t* n_tab, int64_t c, int64_t stride) {
  int64_t L = n_tab[c];
  L = L < 0 ? 0 : L;
  L = L > stride ? stride : L;
  return L > STOI_MAX_LEN ? STOI_MAX_LEN : L;
}
// sum over the 16 lanes of a group, the same order in every lane
__device__ __forceinline__ double st_sum16(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(STOI_KEEP_THREADS) void stoi_keep_kernel(
    const double* __restrict__ x, const int32_t* __restrict__ n_tab, int64_t stride,
    int64_t kmax, int64_t t_stride, int32_t* __restrict__ keep, int32_t* __restrict__ frames) {
  extern __shared__ __attribute__((aligned(16))) double e[];   // t_stride energies
  __shared__ double w[STOI_NF];
  __shared__ double red[STOI_KEEP_THREADS / 64];
  __shared__ int cnt[STOI_KEEP_THREADS / 64];
  constexpr int NW = STOI_KEEP_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x;
  int64_t K = stoi_frames(st_len(n_tab, c, stride));
  K = K > kmax ? kmax : K;
  if (tid < STOI_NF) w[tid] = st_window(tid);
  __syncthreads();
  const double* __restrict__ xr = x + c * stride;
  for (int64_t k = wave; k < K; k += NW) {
    const double* f = xr + k * STOI_HOP;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < STOI_NF / 64; ++q) {
      const double v = w[lane + 64 * q] * f[lane + 64 * q];
      s += v * v;
    }
    s = wave_sum_d(s);
    if (lane == 0) e[k] = 20.0 * log10(sqrt(s) + STOI_EPS);
  }
  __syncthreads();
  double m = -INFINITY;
  for (int64_t k = tid; k < K; k += STOI_KEEP_THREADS) m = fmax(m, e[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int wv = 1; wv < NW; ++wv) m = fmax(m, red[wv]);
  const double thr = m - STOI_DYN;
  int32_t* __restrict__ kp = keep + c * t_stride;
  int base = 0;
  for (int64_t k0 = 0; k0 < K; k0 += STOI_KEEP_THREADS) {
    const int64_t k = k0 + tid;
    const bool flag = k < K && e[k] > thr;
    const unsigned long long b = __ballot(flag);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) cnt[wave] = __popcll(b);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) {
      const int cv = cnt[wv];
      off += wv < wave ? cv : 0;
      tot += cv;
    }
    if (flag) kp[off + pre] = (int32_t)k;
    base += tot;
    __syncthreads();
  }
  if (tid == 0) frames[c] = base;
}

__global__ __launch_bounds__(64 * STOI_BANDS_WAVES) void stoi_bands_kernel(
    const double* __restrict__ x, const double* __restrict__ y,
    const int32_t* __restrict__ clean_row, int64_t C, int64_t stride, int64_t t_stride,
    const int32_t* __restrict__ keep, const int32_t* __restrict__ frames,
    double* __restrict__ env) {
  __shared__ double w[STOI_NF];
  __shared__ double ct[STOI_NFFT / 4 + 2];
  __shared__ double scr[STOI_BANDS_WAVES][2 * ST_P];
  __shared__ double pw[STOI_BANDS_WAVES][STOI_NF + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rr = blockIdx.x;
  const int64_t c = rr < C ? rr : (int64_t)clean_row[rr - C];
  if (c < 0 || c >= C) return;   // uniform over the workgroup, before any barrier
  const int64_t T = frames[c], t0 = (int64_t)blockIdx.y * STOI_BANDS_WAVES;
  if (t0 >= T) return;
  const double* __restrict__ src = rr < C ? x + rr * stride : y + (rr - C) * stride;
  w[tid] = st_window(tid);
  sp_quarter_wave<64 * STOI_BANDS_WAVES>(ct, STOI_NFFT, tid);
  __syncthreads();
  const int64_t t = t0 + wave;
  if (t >= T) return;   // no workgroup barrier below
  const int32_t* __restrict__ kp = keep + c * t_stride;
  const double* f0 = src + (int64_t)kp[t] * STOI_HOP;
  const double* fp = t > 0 ? src + (int64_t)kp[t - 1] * STOI_HOP : nullptr;
  const double* fn = t + 1 < T ? src + (int64_t)kp[t + 1] * STOI_HOP : nullptr;
  // sample i of frame t of the silence-removed signal: its own windowed frame
  // plus the overlapping half of the neighbour on that side
  auto sample = [&](int i) {
    double v = w[i] * f0[i];
    if (i < STOI_HOP) {
      if (fp) v += w[i + STOI_HOP] * fp[i + STOI_HOP];
    } else if (fn) {
      v += w[i - STOI_HOP] * fn[i - STOI_HOP];
    }
    return w[i] * v;
  };
  const SpFft f = {scr[wave], scr[wave] + ST_P, ct, STOI_NF, 8, STOI_NFFT};
#pragma unroll
  for (int q = 0; q < 2; ++q) {   // c[n] = s[2n] + i s[2n+1]; n >= 128 is the zero padding
    const int n = lane + 64 * q;
    f.st(n, {sample(2 * n), sample(2 * n + 1)});
    f.st(n + STOI_NF / 2, {0.0, 0.0});
  }
  sp_barrier<true>();
  sp_dif<64, true>(f, lane);
  SpSpec<2> X;
  sp_split<64, 2>(f, lane, 1.0, X);
  double* p = pw[wave];
#pragma unroll
  for (int e = 0; e < 2; ++e) {   // slot q: bins q and 256 - q; slot 0: (DC, Nyquist) and bin 128
    const int q = lane + 64 * e;
    if (q == 0) {
      p[0] = X.a[e].re * X.a[e].re;
      p[STOI_NF] = X.a[e].im * X.a[e].im;
      p[STOI_NF / 2] = cabs2(X.b[e]);
    } else {
      p[q] = cabs2(X.a[e]);
      p[STOI_NF - q] = cabs2(X.b[e]);
    }
  }
  sp_barrier<true>();
  if (lane < STOI_J) {
    double s = 0.0;
    for (int b = STOI_BAND[lane]; b < STOI_BAND[lane + 1]; ++b) s += p[b];
    env[(rr * STOI_J + lane) * t_stride + t] = sqrt(s);
  }
}

template <bool EXT>
__global__ __launch_bounds__(STOI_SCORE_THREADS) void stoi_score_kernel(
    const int32_t* __restrict__ clean_row, int64_t C, int64_t t_stride, int64_t chunks,
    const int32_t* __restrict__ frames, const double* __restrict__ env,
    double* __restrict__ part) {
  constexpr int GROUPS = STOI_SCORE_THREADS / 16;   // segments of a round
  __shared__ double sx[STOI_J * ST_W];
  __shared__ double sy[STOI_J * ST_W];
  __shared__ double stat[EXT ? GROUPS : 1][4][16];   // ESTOI: a segment's row means and norms
  __shared__ double dseg[STOI_SEG];
  const int tid = threadIdx.x, l = tid & 15, g = tid >> 4;
  const int64_t r = blockIdx.x, ch = blockIdx.y;
  const int64_t c = clean_row[r];
  if (c < 0 || c >= C) return;
  const int64_t M = (int64_t)frames[c] - STOI_N + 1, s0 = ch * STOI_SEG;
  if (s0 >= M) return;   // uniform; covers T < N
  const int ns = (int)(M - s0 < STOI_SEG ? M - s0 : STOI_SEG), nt = ns + STOI_N - 1;
  const double* __restrict__ ex = env + c * STOI_J * t_stride + s0;
  const double* __restrict__ ey = env + (C + r) * STOI_J * t_stride + s0;
  for (int i = tid; i < STOI_J * nt; i += STOI_SCORE_THREADS) {
    const int j = i / nt, t = i - j * nt;
    sx[j * ST_W + t] = ex[j * t_stride + t];
    sy[j * ST_W + t] = ey[j * t_stride + t];
  }
  __syncthreads();
  for (int g0 = 0; g0 < ns; g0 += GROUPS) {
    const int s = g0 + g;
    const bool live = s < ns;
    double val = 0.0;
    if constexpr (!EXT) {
      if (live && l < STOI_J) {
        const double* px = sx + l * ST_W + s;
        const double* py = sy + l * ST_W + s;
        double sxx = 0.0, syy = 0.0;
        for (int t = 0; t < STOI_N; ++t) {
          sxx += px[t] * px[t];
          syy += py[t] * py[t];
        }
        const double alpha = sqrt(sxx) / (sqrt(syy) + STOI_EPS);
        double mx = 0.0, my = 0.0;
        for (int t = 0; t < STOI_N; ++t) {
          mx += px[t];
          my += fmin(alpha * py[t], STOI_CLIP * px[t]);
        }
        mx /= STOI_N;
        my /= STOI_N;
        double nx = 0.0, ny = 0.0, dot = 0.0;
        for (int t = 0; t < STOI_N; ++t) {
          const double xc = px[t] - mx, yc = fmin(alpha * py[t], STOI_CLIP * px[t]) - my;
          nx += xc * xc;
          ny += yc * yc;
          dot += xc * yc;
        }
        val = dot / ((sqrt(nx) + STOI_EPS) * (sqrt(ny) + STOI_EPS));
      }
      val = st_sum16(val) / STOI_J;
    } else {
      if (live && l < STOI_J) {
        const double* px = sx + l * ST_W + s;
        const double* py = sy + l * ST_W + s;
        double mx = 0.0, my = 0.0;
        for (int t = 0; t < STOI_N; ++t) {
          mx += px[t];
          my += py[t];
        }
        mx /= STOI_N;
        my /= STOI_N;
        double nx = 0.0, ny = 0.0;
        for (int t = 0; t < STOI_N; ++t) {
          const double xc = px[t] - mx, yc = py[t] - my;
          nx += xc * xc;
          ny += yc * yc;
        }
        stat[g][0][l] = mx;
        stat[g][1][l] = sqrt(nx) + STOI_EPS;
        stat[g][2][l] = my;
        stat[g][3][l] = sqrt(ny) + STOI_EPS;
      }
      __syncthreads();   // the round loop is uniform over the workgroup
      if (live) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int t = l + 16 * h;
          if (t >= STOI_N) continue;
          double xr[STOI_J], yr[STOI_J], cx = 0.0, cy = 0.0;
#pragma unroll
          for (int j = 0; j < STOI_J; ++j) {
            xr[j] = (sx[j * ST_W + s + t] - stat[g][0][j]) / stat[g][1][j];
            yr[j] = (sy[j * ST_W + s + t] - stat[g][2][j]) / stat[g][3][j];
            cx += xr[j];
            cy += yr[j];
          }
          cx /= STOI_J;
          cy /= STOI_J;
          double nx = 0.0, ny = 0.0, dot = 0.0;
#pragma unroll
          for (int j = 0; j < STOI_J; ++j) {
            const double xc = xr[j] - cx, yc = yr[j] - cy;
            nx += xc * xc;
            ny += yc * yc;
            dot += xc * yc;
          }
          val += dot / ((sqrt(nx) + STOI_EPS) * (sqrt(ny) + STOI_EPS));
        }
      }
      val = st_sum16(val) / STOI_N;
      __syncthreads();   // stat is free for the next round
    }
    if (live && l == 0) dseg[s] = val;
  }
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int s = 0; s < ns; ++s) acc += dseg[s];
    part[r * chunks + ch] = acc;
  }
}

__global__ void stoi_finish_kernel(const int32_t* __restrict__ clean_row, int64_t C, int64_t R,
                                   int64_t chunks, const int32_t* __restrict__ frames,
                                   const double* __restrict__ part, double* __restrict__ score) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t c = clean_row[r];
  if (c < 0 || c >= C) {   // a table the host check never saw
    score[r] = NAN;
    return;
  }
  const int64_t M = (int64_t)frames[c] - STOI_N + 1;
  if (M <= 0) {
    score[r] = STOI_SENTINEL;
    return;
  }
  const int64_t nch = (M + STOI_SEG - 1) / STOI_SEG;
  double acc = 0.0;
  for (int64_t ch = 0; ch < nch; ++ch) acc += part[r * chunks + ch];
  score[r] = acc / (double)M;
}

static const char ST_RULE[] =
    "n_clean, n_restored, stride >= 0, extended 0 or 1, every n in [0, min(stride, 2^20)], "
    "every clean_row in [0, n_clean)";

}  // namespace ainp

using namespace ainp;

extern "C" int ainp_stoi_plan(int64_t n_clean, int64_t n_restored, int64_t max_len,
                              AinpStoiPlan* plan) {
  if (!plan) return record_bad_argument("ainp_stoi_plan", "plan must not be NULL");
  *plan = AinpStoiPlan{};
  const StoiPlan p = stoi_plan(n_clean, n_restored, max_len);
  if (!p.ok)
    return record_bad_argument("ainp_stoi_plan",
                               "n_clean, n_restored >= 0, max_len in [0, 2^20]");
  plan->max_len = STOI_MAX_LEN;
  plan->frames = p.frames;
  plan->t_stride = p.t_stride;
  plan->chunks = p.chunks;
  plan->keep_off = p.keep_off;
  plan->env_off = p.env_off;
  plan->part_off = p.part_off;
  plan->bytes = p.bytes;
  plan->keep_lds = p.keep_lds;
  return AINP_OK;
}

extern "C" size_t ainp_stoi_workspace(int64_t n_clean, int64_t n_restored, int64_t max_len) {
  const StoiPlan p = stoi_plan(n_clean, n_restored, max_len);
  return p.ok ? (size_t)p.bytes : 0;
}

extern "C" int ainp_stoi(const double* x, const double* y, int64_t stride, const int32_t* n,
                         int64_t n_clean, const int32_t* clean_row, int64_t n_restored,
                         const int32_t* tables, int extended, double* score, int32_t* frames,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (n_clean < 0 || n_restored < 0 || stride < 0 || n_clean > 0x7fffffff ||
      n_restored > 0x7fffffff || (extended != 0 && extended != 1) || (n_clean > 0 && !n) ||
      (n_restored > 0 && !clean_row))
    return record_bad_argument("ainp_stoi", ST_RULE);
  int64_t max_len = 0;
  if (stoi_check_tables(n, n_clean, clean_row, n_restored, stride, &max_len) != 0)
    return record_bad_argument("ainp_stoi", ST_RULE);
  if (n_clean == 0) return AINP_OK;   // and so n_restored == 0
  const StoiPlan p = stoi_plan(n_clean, n_restored, max_len);
  if (!p.ok) return record_bad_argument("ainp_stoi", ST_RULE);
  if (!x || !tables || !frames || !workspace || workspace_bytes < (size_t)p.bytes ||
      (n_restored > 0 && (!y || !score)))
    return record_bad_argument("ainp_stoi");
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)stoi_keep_kernel,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(8 * stoi_up(stoi_frames(STOI_MAX_LEN), 2))) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_stoi: cannot reserve 64 KB of LDS");
  hipStream_t s = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  int32_t* keep = reinterpret_cast<int32_t*>(ws + p.keep_off);
  double* env = reinterpret_cast<double*>(ws + p.env_off);
  double* part = reinterpret_cast<double*>(ws + p.part_off);
  const int32_t* n_dev = tables;
  const int32_t* row_dev = tables + n_clean;
  hipLaunchKernelGGL(stoi_keep_kernel, dim3((unsigned)n_clean), dim3(STOI_KEEP_THREADS),
                     (size_t)p.keep_lds, s, x, n_dev, stride, p.frames, p.t_stride, keep, frames);
  int rc = check_launch("ainp_stoi (keep)");
  if (rc != AINP_OK || n_restored == 0) return rc;
  if (p.frames > 0) {
    const dim3 grid((unsigned)(n_clean + n_restored),
                    (unsigned)cdiv(p.frames, STOI_BANDS_WAVES));
    hipLaunchKernelGGL(stoi_bands_kernel, grid, dim3(64 * STOI_BANDS_WAVES), 0, s, x, y, row_dev,
                       n_clean, stride, p.t_stride, keep, frames, env);
    if ((rc = check_launch("ainp_stoi (bands)")) != AINP_OK) return rc;
  }
  if (p.frames >= STOI_N) {
    const dim3 grid((unsigned)n_restored, (unsigned)p.chunks);
    if (extended)
      hipLaunchKernelGGL(stoi_score_kernel<true>, grid, dim3(STOI_SCORE_THREADS), 0, s, row_dev,
                         n_clean, p.t_stride, p.chunks, frames, env, part);
    else
      hipLaunchKernelGGL(stoi_score_kernel<false>, grid, dim3(STOI_SCORE_THREADS), 0, s, row_dev,
                         n_clean, p.t_stride, p.chunks, frames, env, part);
    if ((rc = check_launch("ainp_stoi (score)")) != AINP_OK) return rc;
  }
  hipLaunchKernelGGL(stoi_finish_kernel, dim3((unsigned)cdiv(n_restored, 256)), dim3(256), 0, s,
                     row_dev, n_clean, n_restored, p.chunks, frames, part, score);
  return check_launch("ainp_stoi (finish)");
}
