// spain_learned.hip — A-SPAIN and S-SPAIN over the whole signal with a Gabor
// frame and an optional unitary sparsity-enhancing basis
// (references/basisopt/a_spain_learned.m, s_spain_learned.m and
// hard_thresholding_dgtreal.m; restated in DESIGN §14.2).  All arithmetic float64.
//
// Unlike spain.hip the frames are coupled through the signal, so one workgroup
// cannot own a problem.  A pass is a short sequence of launches and the
// launches are the barriers; there is no cooperative launch and no spin
// barrier.  With K = M/2 + 1 bins, N = L/a frames a signal and NF = n_signals N:
//   sl_forward   one frame per workgroup: gather x (S: x - u) at (n a - w/2 + i)
//                mod L, times the analysis window, at (i - w/2) mod M of a zero
//                buffer, the LDS real transform of spain_fft.h -> K bins
//   sl_gemm      Z = U C (and Y = U^H B) as one tiled complex product over all
//                NF frames: 32 x 32 outputs a workgroup, 2 x 2 a lane, the
//                reduction in chunks of 16 through LDS, so U is read once per
//                32 frames.  Skipped when basis == NULL.
//   sl_select    one column per workgroup: (A: u = z - B', v = z + u) the radix
//                select of spain_fft.h on |v|^2 (rows 0 and K-1 halved), ties to
//                the lower row; A: the column's part of |z - zb|^2 and
//                B = zb - u in place (next pass u = z - B gives u + z - zb)
//   sl_inverse   one frame per workgroup: imaginary parts of rows 0 and K-1
//                dropped, inverse LDS transform times 2 (= irfft M), entries
//                (i - w/2) mod M times the synthesis window -> F [NF][w]
//   sl_ola_a /   overlap-add as a gather: every sample sums its w/a frames in
//   sl_ola_s     frame order, no atomics.  A: record, then x = sum on the
//                missing samples.  S: xe = sum, a block's part of |xe - x|^2
//   sl_decide    one workgroup per signal adds the parts in a fixed order; one
//                lane writes the objective, iters, `rec` (the pass whose x is
//                the result) and `done`
//   sl_update_s  S: record, x = proj(xe + u), u += xe - x
// Every kernel returns at once for a signal whose `done` is set, so results do
// not depend on how many passes the host goes on issuing: it reads the flags
// every SL_CHUNK passes and stops when all are set.
//
// A pass:  A: select, decide, [U^H], inverse, ola_a, forward, [U]
//          S: forward, [U], select, [U^H], inverse, ola_s, decide, update_s
//
// LDS at M = 2048 (transform kernels): re, im 2 x (1024 + 34) x 8 = 16928, the
// quarter wave 514 x 8 = 4112: 21 KiB.  sl_gemm: 2 x 16 x 33 x 16 = 16.5 KiB.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "spain_fft.h"
#include "spain_plan.h"

namespace ainp {

constexpr int SL_MAXIT = 65536;
constexpr int SL_NT = 256;
constexpr int SL_EPL = SL_MMAX / 4 / SL_NT;               // spectrum slots a lane: 2
constexpr int SL_NK = (SL_MMAX / 2 + 1 + SL_NT - 1) / SL_NT;   // bins a lane ranks: 5
constexpr int SL_CHUNK = 32;                              // passes between two looks at `done`
constexpr int SL_TILE = 32, SL_RED = 16;

struct SlWs {   // byte offsets into the workspace, each a multiple of 16
  size_t g, gd, xc, u, xe, Z, B, T, F, part, best, done, rec, total;
  int64_t nparts;
};
static SlWs sl_layout(int64_t L, int64_t S, int w, int a, int M, bool basis, int alg) {
  SlWs l;
  const int64_t N = L / a, NF = S * N, K = M / 2 + 1;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 15) & ~(size_t)15;
    return o;
  };
  l.nparts = alg == AINP_SPAIN_A ? N : cdiv(L, SL_NT);
  l.g = take(sizeof(double) * w);
  l.gd = take(sizeof(double) * w);
  l.xc = take(sizeof(double) * S * L);
  l.u = take(alg == AINP_SPAIN_S ? sizeof(double) * S * L : 0);
  l.xe = take(alg == AINP_SPAIN_S ? sizeof(double) * S * L : 0);
  l.Z = take(sizeof(cplx) * NF * K);
  l.B = take(sizeof(cplx) * NF * K);
  l.T = take(basis ? sizeof(cplx) * NF * K : 0);
  l.F = take(sizeof(double) * NF * w);
  l.part = take(sizeof(double) * S * l.nparts);
  l.best = take(sizeof(double) * S);
  l.done = take(sizeof(int) * S);
  l.rec = take(sizeof(int) * S);
  l.total = at;
  return l;
}

// g: the periodic Hann window; gd = g / (M sum_j g^2[(i mod a) + j a])
__global__ __launch_bounds__(SL_NT) void sl_windows(double* g, double* gd, int w, int a, int M) {
  for (int i = threadIdx.x; i < w; i += SL_NT) g[i] = 0.5 - 0.5 * cospi(2.0 * i / (double)w);
  __syncthreads();
  for (int i = threadIdx.x; i < w; i += SL_NT) {
    double s = 0.0;
    for (int j = i % a; j < w; j += a) s += g[j] * g[j];
    gd[i] = g[i] / ((double)M * s);
  }
}

__global__ __launch_bounds__(SL_NT) void sl_init(const double* __restrict__ x,
                                                 const uint8_t* __restrict__ obs, int64_t total,
                                                 double* xc, double* u) {
  const int64_t t = (int64_t)blockIdx.x * SL_NT + threadIdx.x;
  if (t >= total) return;
  xc[t] = obs[t] ? x[t] : 0.0;
  if (u) u[t] = 0.0;
}

__global__ __launch_bounds__(SL_NT) void sl_init_state(int64_t S, int maxit, double* best,
                                                       int* done, int* rec, int32_t* iters,
                                                       double* hist) {
  const int64_t i = (int64_t)blockIdx.x * SL_NT + threadIdx.x;
  if (i < S) {
    best[i] = INFINITY;
    done[i] = 0;
    rec[i] = 0;
    iters[i] = 0;
  }
  if (hist && i < S * maxit) hist[i] = NAN;
}

// grid: one workgroup per frame of every signal.  dynamic LDS: re, im, ct.
__global__ __launch_bounds__(SL_NT) void sl_forward(const double* __restrict__ xc,
                                                    const double* __restrict__ u,
                                                    const double* __restrict__ win,
                                                    cplx* __restrict__ C, int64_t L, int N, int w,
                                                    int a, int M, int lgN, int nF,
                                                    const int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t frame = blockIdx.x;
  const int64_t sig = frame / N;
  if (done[sig]) return;
  const int n = (int)(frame - sig * N), tid = threadIdx.x, Nh = M / 2;
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nF;
  double* ct = im + nF;
  sp_quarter_wave<SL_NT>(ct, M, tid);
  const SpFft f = {re, im, ct, Nh, lgN, M};
  const double* xs = xc + sig * L;
  const double* us = u ? u + sig * L : nullptr;
  for (int j = tid; j < Nh; j += SL_NT) {
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = (2 * j + h + w / 2) & (M - 1);
      v[h] = 0.0;
      if (i < w) {
        int64_t t = (int64_t)n * a - w / 2 + i;
        if (t < 0) t += L;
        if (t >= L) t -= L;
        v[h] = (us ? xs[t] - us[t] : xs[t]) * win[i];
      }
    }
    f.st(j, {v[0], v[1]});
  }
  __syncthreads();
  sp_dif<SL_NT>(f, tid);
  SpSpec<SL_EPL> X;
  sp_split<SL_NT, SL_EPL>(f, tid, 1.0, X);
  cplx* c = C + frame * (int64_t)(Nh + 1);
#pragma unroll
  for (int e = 0; e < SL_EPL; ++e) {
    const int p = tid + e * SL_NT;
    if (p >= Nh / 2) continue;
    if (p == 0) {
      c[0] = {X.a[e].re, 0.0};
      c[Nh] = {X.a[e].im, 0.0};
      c[Nh / 2] = X.b[e];
    } else {
      c[p] = X.a[e];
      c[Nh - p] = X.b[e];
    }
  }
}

// grid: one workgroup per frame.  Y [NF][K] -> F [NF][w] = (irfft M)[(i - w/2) mod M] win[i]
__global__ __launch_bounds__(SL_NT) void sl_inverse(const cplx* __restrict__ Y,
                                                    const double* __restrict__ win,
                                                    double* __restrict__ F, int N, int w, int M,
                                                    int lgN, int nF, const int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t frame = blockIdx.x;
  if (done[frame / N]) return;
  const int tid = threadIdx.x, Nh = M / 2;
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nF;
  double* ct = im + nF;
  sp_quarter_wave<SL_NT>(ct, M, tid);
  const SpFft f = {re, im, ct, Nh, lgN, M};
  const cplx* y = Y + frame * (int64_t)(Nh + 1);
  SpSpec<SL_EPL> X;
#pragma unroll
  for (int e = 0; e < SL_EPL; ++e) {
    const int p = tid + e * SL_NT;
    X.a[e] = X.b[e] = {0.0, 0.0};
    if (p >= Nh / 2) continue;
    if (p == 0) {
      X.a[e] = {y[0].re, y[Nh].re};
      X.b[e] = y[Nh / 2];
    } else {
      X.a[e] = y[p];
      X.b[e] = y[Nh - p];
    }
  }
  __syncthreads();   // the quarter wave is complete
  sp_merge<SL_NT, SL_EPL>(f, tid, X);
  __syncthreads();
  sp_dit<SL_NT>(f, tid);
  double* o = F + frame * (int64_t)w;
  for (int i = tid; i < w; i += SL_NT) {
    const int m = (i - w / 2) & (M - 1);
    const cplx c = f.ld(m >> 1);
    o[i] = 2.0 * ((m & 1) ? c.im : c.re) * win[i];
  }
}

// out[n][o] = sum_r in[n][r] U[o][r] (HERM false) or sum_r in[n][r] conj(U[r][o])
// (HERM true), n < NF, o, r < K.  grid: (ceil(NF / 32), ceil(K / 32)), 256 lanes.
template <bool HERM>
__global__ __launch_bounds__(SL_NT) __attribute__((amdgpu_waves_per_eu(1, 4))) void sl_gemm(const cplx* __restrict__ in,
                                                 const cplx* __restrict__ U,
                                                 cplx* __restrict__ out, int K, int64_t NF, int N,
                                                 const int* __restrict__ done) {
  __shared__ __attribute__((aligned(16))) cplx As[SL_RED][SL_TILE + 1];   // [r][n]
  __shared__ __attribute__((aligned(16))) cplx Bs[SL_RED][SL_TILE + 1];   // [r][o]
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * SL_TILE;
  const int o0 = blockIdx.y * SL_TILE;
  {   // nothing to do when every signal this tile touches has stopped
    const int64_t last = n0 + SL_TILE - 1 < NF ? n0 + SL_TILE - 1 : NF - 1;
    const int64_t s0 = n0 / N, s1 = last / N;
    bool live = false;
    for (int64_t s = s0; s <= s1; ++s) live = live || !done[s];
    if (!live) return;
  }
  const int tx = tid & 15, ty = tid >> 4;
  const cplx zero = {0.0, 0.0};
  cplx acc[2][2] = {{zero, zero}, {zero, zero}};
  // the next chunk's operands are fetched into registers while this one is used
  cplx pa0, pa1, pb0, pb1;
  auto fetch = [=](int r0, int h, cplx& pa, cplx& pb) {
    const int64_t n = n0 + ty + 16 * h;
    pa.re = pa.im = pb.re = pb.im = 0.0;
    if (n < NF && r0 + tx < K) pa = in[n * K + r0 + tx];
    if (!HERM) {
      const int oo = ty + 16 * h;
      if (o0 + oo < K && r0 + tx < K) pb = U[(int64_t)(o0 + oo) * K + r0 + tx];
    } else {
      const int oo = tid & 31, r2 = (tid >> 5) + 8 * h;
      if (o0 + oo < K && r0 + r2 < K) pb = U[(int64_t)(r0 + r2) * K + o0 + oo];
      pb.im = -pb.im;
    }
  };
  fetch(0, 0, pa0, pb0);
  fetch(0, 1, pa1, pb1);
  for (int r0 = 0; r0 < K; r0 += SL_RED) {
    As[tx][ty] = pa0;
    As[tx][ty + 16] = pa1;
    if (!HERM) {
      Bs[tx][ty] = pb0;
      Bs[tx][ty + 16] = pb1;
    } else {
      Bs[tid >> 5][tid & 31] = pb0;
      Bs[(tid >> 5) + 8][tid & 31] = pb1;
    }
    __syncthreads();
    if (r0 + SL_RED < K) {
      fetch(r0 + SL_RED, 0, pa0, pb0);
      fetch(r0 + SL_RED, 1, pa1, pb1);
    }
#pragma unroll
    for (int rr = 0; rr < SL_RED; ++rr) {
      const cplx a0 = As[rr][ty], a1 = As[rr][ty + 16], b0 = Bs[rr][tx], b1 = Bs[rr][tx + 16];
      acc[0][0] = cadd(acc[0][0], cmul(a0, b0));
      acc[0][1] = cadd(acc[0][1], cmul(a0, b1));
      acc[1][0] = cadd(acc[1][0], cmul(a1, b0));
      acc[1][1] = cadd(acc[1][1], cmul(a1, b1));
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t n = n0 + ty + 16 * i;
      const int o = o0 + tx + 16 * j;
      if (n < NF && o < K) out[n * K + o] = acc[i][j];
    }
}

// grid: one workgroup per column (frame).  H_k on v; rows 0 and K-1 rank by
// |v| / sqrt 2, ties go to the lower row, k >= K keeps everything.
//   A: u = z - B (0 in the first pass), v = z + u, zb = H_k(v),
//      part[frame] = sum |z - zb|^2, B = zb - u
//   S: B = H_k(z)
template <int ALG>
__global__ __launch_bounds__(SL_NT) __attribute__((amdgpu_waves_per_eu(1, 4))) void sl_select(const cplx* __restrict__ Z, cplx* __restrict__ B,
                                                   int K, int k, int first, int N,
                                                   double* __restrict__ part,
                                                   const int* __restrict__ done) {
  __shared__ uint32_t hist[256];
  __shared__ double psum[SL_NT / 64];
  __shared__ int sel[4];
  const int64_t frame = blockIdx.x;
  if (done[frame / N]) return;
  const int tid = threadIdx.x;
  const cplx* z = Z + frame * (int64_t)K;
  cplx* b = B + frame * (int64_t)K;
  const cplx zero = {0.0, 0.0};
  cplx zv[SL_NK], uv[SL_NK], vv[SL_NK];
  uint64_t key[SL_NK];
  bool member[SL_NK], keep[SL_NK];
  int row[SL_NK];
#pragma unroll
  for (int e = 0; e < SL_NK; ++e) {
    const int bin = row[e] = tid + e * SL_NT;
    member[e] = bin < K;
    zv[e] = uv[e] = vv[e] = zero;
    double m2 = 0.0;
    if (member[e]) {
      zv[e] = z[bin];
      if (ALG == AINP_SPAIN_A) {
        if (!first) uv[e] = csub(zv[e], b[bin]);
        vv[e] = cadd(zv[e], uv[e]);
      } else {
        vv[e] = zv[e];
      }
      m2 = cabs2(vv[e]);
      if (bin == 0 || bin == K - 1) m2 *= 0.5;
    }
    key[e] = (uint64_t)__double_as_longlong(m2);
  }
  sp_keep_largest<SL_NT, SL_NK>(key, member, row, k, K, hist, sel, tid, keep);
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < SL_NK; ++e) {
    if (!member[e]) continue;
    cplx zb = vv[e];
    if (!keep[e]) zb.re = zb.im = 0.0;
    if (ALG == AINP_SPAIN_A) {
      acc += cabs2(csub(zv[e], zb));
      b[tid + e * SL_NT] = csub(zb, uv[e]);
    } else {
      b[tid + e * SL_NT] = zb;
    }
  }
  if (ALG == AINP_SPAIN_A) {
    const double s = sp_sum<SL_NT>(acc, psum, tid);
    if (tid == 0) part[frame] = s;
  }
}

// sample t of a signal: the sum over its w / a frames in frame order
__device__ __forceinline__ double sl_gather(const double* __restrict__ Fs, int64_t t, int N, int w,
                                            int a) {
  const int64_t top = (t + w / 2) / a;   // the last frame that holds t
  double s = 0.0;
  for (int64_t n = top - w / a + 1; n <= top; ++n) {
    const int i = (int)(t + w / 2 - n * a);
    int64_t nn = n % N;
    if (nn < 0) nn += N;
    s += Fs[nn * w + i];
  }
  return s;
}

// grid: ceil(L / 256) workgroups per signal.  A: record, then x = the sum on
// the missing samples (observed ones hold the input throughout).
__global__ __launch_bounds__(SL_NT) void sl_ola_a(const double* __restrict__ F, double* xc,
                                                  double* x, const uint8_t* __restrict__ obs,
                                                  int64_t L, int nblk, int N, int w, int a, int cnt,
                                                  const int* __restrict__ rec,
                                                  const int* __restrict__ done) {
  const int64_t sig = blockIdx.x / nblk;
  const int64_t t = (int64_t)(blockIdx.x - sig * nblk) * SL_NT + threadIdx.x;
  if (t >= L || obs[sig * L + t]) return;
  if (rec[sig] == cnt) x[sig * L + t] = xc[sig * L + t];
  if (done[sig]) return;
  xc[sig * L + t] = sl_gather(F + sig * N * (int64_t)w, t, N, w, a);
}

// S: xe = the sum, part[block] = the block's sum of (xe - x)^2
__global__ __launch_bounds__(SL_NT) void sl_ola_s(const double* __restrict__ F,
                                                  const double* __restrict__ xc,
                                                  double* __restrict__ xe, int64_t L, int nblk,
                                                  int N, int w, int a, double* __restrict__ part,
                                                  const int* __restrict__ done) {
  __shared__ double psum[SL_NT / 64];
  const int64_t sig = blockIdx.x / nblk;
  if (done[sig]) return;
  const int64_t t = (int64_t)(blockIdx.x - sig * nblk) * SL_NT + threadIdx.x;
  double d = 0.0;
  if (t < L) {
    const double v = sl_gather(F + sig * N * (int64_t)w, t, N, w, a);
    xe[sig * L + t] = v;
    d = v - xc[sig * L + t];
  }
  const double s = sp_sum<SL_NT>(d * d, psum, threadIdx.x);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// S: record, then x = proj(xe + u), u += xe - x
__global__ __launch_bounds__(SL_NT) void sl_update_s(const double* __restrict__ xe, double* xc,
                                                     double* u, double* x,
                                                     const uint8_t* __restrict__ obs, int64_t L,
                                                     int nblk, int cnt,
                                                     const int* __restrict__ rec,
                                                     const int* __restrict__ done) {
  const int64_t sig = blockIdx.x / nblk;
  const int64_t t = (int64_t)(blockIdx.x - sig * nblk) * SL_NT + threadIdx.x;
  if (t >= L) return;
  const int64_t at = sig * L + t;
  const bool o = obs[at];
  if (rec[sig] == cnt && !o) x[at] = xc[at];
  if (done[sig]) return;
  const double e = xe[at], un = u[at];
  const double xn = o ? xc[at] : e + un;
  u[at] = un + (e - xn);
  xc[at] = xn;
}

// grid: one workgroup per signal.  The objective from the parts in a fixed
// order; lane 0 takes every decision of the pass, once.
__global__ __launch_bounds__(SL_NT) void sl_decide(const double* __restrict__ part, int64_t nparts,
                                                   int cnt, int maxit, double epsilon, double* best,
                                                   int* done, int* rec, int32_t* iters,
                                                   double* hist) {
  __shared__ double psum[SL_NT / 64];
  const int64_t sig = blockIdx.x;
  if (done[sig]) return;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += SL_NT) acc += part[sig * nparts + i];
  const double s = sp_sum<SL_NT>(acc, psum, threadIdx.x);
  if (threadIdx.x != 0) return;
  const double obj = sqrt(s);
  if (hist) hist[sig * maxit + cnt - 1] = obj;
  iters[sig] = cnt;
  if (obj <= best[sig]) {   // the x the objective was evaluated on becomes the result
    best[sig] = obj;
    rec[sig] = cnt;
  }
  if (obj <= epsilon || cnt == maxit) done[sig] = 1;
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_spain_learned_workspace(int64_t L, int64_t n_signals, int w, int a, int M,
                                               int has_basis, int algorithm) {
  if (sl_shape_rule(L, w, a, M) || n_signals < 1 ||
      (algorithm != AINP_SPAIN_A && algorithm != AINP_SPAIN_S))
    return 0;
  return sl_layout(L, n_signals, w, a, M, has_basis != 0, algorithm).total;
}

extern "C" int ainp_spain_learned(double* x, const uint8_t* observed, int64_t L, int64_t n_signals,
                                  int w, int a, int M, const double* basis, int algorithm, int s,
                                  int r, double epsilon, int maxit, int32_t* iters,
                                  double* obj_history, void* workspace, size_t ws_bytes,
                                  void* stream) {
  const char* fn = "ainp_spain_learned";
  if (!x || !observed || !iters || n_signals < 0) return record_bad_argument(fn);
  if (algorithm != AINP_SPAIN_A && algorithm != AINP_SPAIN_S)
    return record_bad_argument(fn, "algorithm is AINP_SPAIN_A or AINP_SPAIN_S");
  if (const char* rule = sl_shape_rule(L, w, a, M)) return record_bad_argument(fn, rule);
  if (s < 1 || r < 1) return record_bad_argument(fn, "s >= 1, r >= 1");
  if (!(epsilon >= 0.0)) return record_bad_argument(fn, "epsilon >= 0");
  if (maxit < 1 || maxit > SL_MAXIT) return record_bad_argument(fn, "1 <= maxit <= 65536");
  const int64_t N = L / a, nblk = cdiv(L, SL_NT);
  if (n_signals * std::max(N, nblk) > 0x7fffffff)
    return record_msg("ainp_spain_learned: too many signals (n_signals L / a < 2^31)");
  if (n_signals == 0) return AINP_OK;
  const SlWs l = sl_layout(L, n_signals, w, a, M, basis != nullptr, algorithm);
  if (!workspace || ws_bytes < l.total || ((uintptr_t)workspace & 15))
    return record_msg("ainp_spain_learned: workspace too small or not 16-byte aligned");

  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  auto dbl = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
  auto cpx = [&](size_t off) { return reinterpret_cast<cplx*>(ws + off); };
  double *g = dbl(l.g), *gd = dbl(l.gd), *xc = dbl(l.xc), *F = dbl(l.F), *part = dbl(l.part);
  double *best = dbl(l.best), *xe = dbl(l.xe);
  double* u = algorithm == AINP_SPAIN_S ? dbl(l.u) : nullptr;
  cplx *Z = cpx(l.Z), *B = cpx(l.B), *T = cpx(l.T);
  int* done = reinterpret_cast<int*>(ws + l.done);
  int* rec = reinterpret_cast<int*>(ws + l.rec);
  const cplx* U = reinterpret_cast<const cplx*>(basis);
  const int K = M / 2 + 1;
  const int64_t NF = n_signals * N, total = n_signals * L;
  const int lgN = sp_lgN(M), nF = sp_fft_lds(M).nF;
  const size_t lds = sp_fft_lds(M).bytes();
  const dim3 gFrames((unsigned)NF), gSamples((unsigned)(n_signals * nblk)), nt(SL_NT);
  const dim3 gGemm((unsigned)cdiv(NF, SL_TILE), (unsigned)cdiv(K, SL_TILE));
  const bool isA = algorithm == AINP_SPAIN_A;

  hipLaunchKernelGGL(sl_windows, dim3(1), nt, 0, st, g, gd, w, a, M);
  hipLaunchKernelGGL(sl_init, dim3((unsigned)cdiv(total, SL_NT)), nt, 0, st, x, observed, total, xc,
                     u);
  const int64_t nstate = std::max<int64_t>(n_signals, obj_history ? n_signals * maxit : 0);
  hipLaunchKernelGGL(sl_init_state, dim3((unsigned)cdiv(nstate, SL_NT)), nt, 0, st, n_signals,
                     maxit, best, done, rec, iters, obj_history);

  // z = U dgt(x - u, win) into Z
  auto analysis = [&](const double* win) {
    hipLaunchKernelGGL(sl_forward, gFrames, nt, lds, st, xc, u, win, U ? T : Z, L, (int)N, w, a, M,
                       lgN, nF, done);
    if (U) hipLaunchKernelGGL(sl_gemm<false>, gGemm, nt, 0, st, T, U, Z, K, NF, (int)N, done);
  };
  // F = the frames of idgt(U^H B, win) before the overlap-add
  auto synthesis = [&](const double* win) {
    if (U) hipLaunchKernelGGL(sl_gemm<true>, gGemm, nt, 0, st, B, U, T, K, NF, (int)N, done);
    hipLaunchKernelGGL(sl_inverse, gFrames, nt, lds, st, U ? T : B, win, F, (int)N, w, M, lgN, nF,
                       done);
  };
  auto decide = [&](int cnt) {
    hipLaunchKernelGGL(sl_decide, dim3((unsigned)n_signals), nt, 0, st, part, l.nparts, cnt, maxit,
                       epsilon, best, done, rec, iters, obj_history);
  };

  int chunk = SL_CHUNK;
  if (const char* e = getenv("AINP_SPAIN_LEARNED_CHUNK")) chunk = atoi(e);   // 0: never look
  std::vector<int> flags;
  if (isA) analysis(g);
  int64_t k = s;
  for (int cnt = 1; cnt <= maxit; ++cnt) {
    const int kk = (int)std::min<int64_t>(k, K);
    if (isA) {
      hipLaunchKernelGGL(sl_select<AINP_SPAIN_A>, gFrames, nt, 0, st, Z, B, K, kk, cnt == 1, (int)N,
                         part, done);
      decide(cnt);
      synthesis(gd);
      hipLaunchKernelGGL(sl_ola_a, gSamples, nt, 0, st, F, xc, x, observed, L, (int)nblk, (int)N, w,
                         a, cnt, rec, done);
      if (cnt < maxit) analysis(g);
    } else {
      analysis(gd);
      hipLaunchKernelGGL(sl_select<AINP_SPAIN_S>, gFrames, nt, 0, st, Z, B, K, kk, 0, (int)N, part,
                         done);
      synthesis(g);
      hipLaunchKernelGGL(sl_ola_s, gSamples, nt, 0, st, F, xc, xe, L, (int)nblk, (int)N, w, a, part,
                         done);
      decide(cnt);
      hipLaunchKernelGGL(sl_update_s, gSamples, nt, 0, st, xe, xc, u, x, observed, L, (int)nblk,
                         cnt, rec, done);
    }
    if ((cnt + 1) % r == 0) k += s;
    if (int rc = check_launch("ainp_spain_learned")) return rc;
    if (chunk > 0 && cnt % chunk == 0 && cnt < maxit) {
      // the flags were set on the device; the host only stops issuing
      flags.resize((size_t)n_signals);
      hipError_t e = hipMemcpyAsync(flags.data(), done, sizeof(int) * n_signals,
                                    hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return record_error(e, "ainp_spain_learned");
      if (std::all_of(flags.begin(), flags.end(), [](int d) { return d != 0; })) break;
    }
  }
  return check_launch("ainp_spain_learned");
}

// The analysis alone: dgt(x, g) of every signal through sl_windows and
// sl_forward, for callers that need the coefficients themselves (the training
// columns of ainp_basis_learn).  workspace: g, gd and the (clear) stop flags.
static size_t dgt_ws_bytes(int64_t n_signals, int w) {
  return (((size_t)2 * w * sizeof(double) + 15) & ~(size_t)15) + sizeof(int) * (size_t)n_signals;
}

extern "C" size_t ainp_spain_dgt_workspace(int64_t n_signals, int w) {
  if (n_signals < 1 || w < SL_WMIN || w > SL_MMAX) return 0;
  return dgt_ws_bytes(n_signals, w);
}

extern "C" int ainp_spain_dgt(const double* x, int64_t L, int64_t n_signals, int w, int a, int M,
                              double* coef, void* workspace, size_t ws_bytes, void* stream) {
  if (!x || !coef || n_signals < 0) return record_bad_argument("ainp_spain_dgt");
  if (const char* rule = sl_shape_rule(L, w, a, M)) return record_bad_argument("ainp_spain_dgt", rule);
  const int64_t N = L / a, NF = n_signals * N;
  if (NF > 0x7fffffff) return record_msg("ainp_spain_dgt: too many signals (n_signals L / a < 2^31)");
  if (n_signals == 0) return AINP_OK;
  if (!workspace || ws_bytes < dgt_ws_bytes(n_signals, w) || ((uintptr_t)workspace & 15))
    return record_msg("ainp_spain_dgt: workspace too small or not 16-byte aligned");
  hipStream_t st = as_stream(stream);
  double* g = static_cast<double*>(workspace);
  double* gd = g + w;
  int* done = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) +
                                     dgt_ws_bytes(n_signals, w) - sizeof(int) * (size_t)n_signals);
  hipError_t e = hipMemsetAsync(done, 0, sizeof(int) * (size_t)n_signals, st);
  if (e != hipSuccess) return record_error(e, "ainp_spain_dgt");
  const SpLds l = sp_fft_lds(M);
  hipLaunchKernelGGL(sl_windows, dim3(1), dim3(SL_NT), 0, st, g, gd, w, a, M);
  hipLaunchKernelGGL(sl_forward, dim3((unsigned)NF), dim3(SL_NT), l.bytes(), st, x,
                     (const double*)nullptr, g, reinterpret_cast<cplx*>(coef), L, (int)N, w, a, M,
                     sp_lgN(M), l.nF, done);
  return check_launch("ainp_spain_dgt");
}
