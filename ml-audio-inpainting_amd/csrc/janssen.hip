// janssen.hip — gap-wise Janssen autoregressive inpainting, the AR baseline of
// the reference's model comparison (models/AudioReg/utils/janssen_inp.m with
// method = "lpc", driven by models/AudioReg/train.m).  All arithmetic float64.
//
// One workgroup owns one segment for all maxit iterations; segments share
// nothing, so the batch is the parallelism.  Per iteration:
//   1. r[k] = sum_n sol[n] sol[n+k], k = 0..p   (lpc's biased autocorrelation;
//      the signal is staged through LDS in chunks, two adjacent lags per lane)
//   2. Levinson-Durbin on r -> a[0..p]
//   3. b[k] = sum_i a[i] a[i+k]                 (the same lag routine on a)
//   4. g_i = -sum_{j observed, |i-j| <= p} b[|i-j|] x_j for the gap rows i
//      (both contexts staged in LDS; the x operand is wave-uniform)
//   5. T z = g, T = Toeplitz(b[0..h)), by the Levinson recursion
//   6. sol[gap] = z (and history), unless a pivot was non-positive or a value
//      non-finite: then the previous iterate stays (the reference's chol break)
// Steps 2 and 5 are one routine: the order-m predictor a of the sequence t
// (r in step 2, b in step 5) is advanced by
//   k = -(t[m+1] + sum_{j=1..m} a[j] t[m+1-j]) / e_m,  a[j] += k a[m+1-j],
//   a[m+1] = k,  e_{m+1} = e_m (1 - k^2)
// and step 5 extends the solution alongside (Z[j] = z_{j-1}):
//   mu = (g[m] - sum_{j=1..m} t[m+1-j] Z[j]) / e_m,  Z[j] += mu a[m+1-j],
//   Z[m+1] = mu.
// e_m are the pivots of T.  The lane that owns the pair (j, m+1-j) updates
// a and Z at both indices from the old values in place, and folds the new
// values into the NEXT step's two sums right away (both use the weight
// t[m+2-j]), so a step is: wave reduce -> one LDS slot per wave -> one barrier
// -> every lane adds the slots in wave order -> update.  One barrier per
// dependent step, no atomics, the same bits on every call.
//
// The wave reduce stays in registers: four DPP stages sum each row of 16 lanes
// (quad swaps, then the two mirrors; both partners add the same two values, so
// a row ends with one value), v_readlane fetches the four row sums.
//
// LDS (doubles), H = the longest gap the stride allows (<= 2048):
// B[max(p, H) + 2] (r, then b; zero beyond p, so the recursions read t[i]
// unguarded) | A[max(p, H) + 2] | Y[H] (g) | W[S] (signal chunks, then the two
// contexts, then Z).  The signal itself stays in global memory (L2): 16384
// doubles do not fit beside the vectors.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace ainp {

constexpr int JN_THREADS = 256;
constexpr int JN_WAVES = JN_THREADS / 64;
constexpr int JN_PMAX = 3072;
constexpr int JN_NMAX = 16384;
constexpr int JN_HMAX = 2048;
constexpr int JN_ITMAX = 1000;

struct JnLds {
  int nB, nA, nY, S;   // doubles
  size_t bytes() const { return ((size_t)nB + nA + nY + S) * sizeof(double); }
};

// n_max: the longest segment the stride allows.  W's S doubles hold, in turn,
// a signal chunk (S - p >= 1024 samples and the p that follow them, or the
// whole segment), the two contexts (<= 2p samples, never more than the
// segment) and Z (gap + 1).
static JnLds jn_lds(int64_t n_max, int p) {
  JnLds l;
  const int hcap = (int)std::min<int64_t>(JN_HMAX, n_max);
  l.nB = (std::max(p, hcap) + 3) & ~1;
  l.nA = l.nB;
  l.nY = (hcap + 1) & ~1;
  const int64_t want = std::max<int64_t>(2 * (int64_t)p, (int64_t)p + 1024);
  l.S = (int)std::max<int64_t>(l.nY + 2, std::min<int64_t>(n_max, want));
  return l;
}

// sum over the wave, the same bits in every lane: rows of 16 by DPP (lane ^ 1,
// lane ^ 2, then the mirrors of 8 and of 16 lanes, whose halves already agree),
// the four rows by v_readlane in a fixed order
template <int CTRL>
__device__ __forceinline__ double jn_dpp(double v) {
  // every lane has a source lane under these controls, `old` is never kept
  const int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false),
                          __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ double jn_readlane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double jn_wave_sum(double v) {
  v += jn_dpp<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += jn_dpp<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += jn_dpp<0x141>(v);   // row_half_mirror
  v += jn_dpp<0x140>(v);   // row_mirror
  return (jn_readlane(v, 0) + jn_readlane(v, 16)) + (jn_readlane(v, 32) + jn_readlane(v, 48));
}

// 1 / x for a positive normal x: v_rcp_f64 and two Newton steps (within an ulp
// or two of the quotient; the full division sequence is twice as long a chain)
__device__ __forceinline__ double jn_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}

// sum_{t < cnt} u[t] * v[VS * t]: four interleaved chains, added in a fixed order
template <int VS>
__device__ __forceinline__ double jn_dot(const double* __restrict__ u,
                                         const double* __restrict__ v, int cnt) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int t = 0;
  for (; t + 8 <= cnt; t += 8) {
    double a[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a[e] = u[t + e];
      b[e] = v[VS * (t + e)];
    }
    s0 = fma(a[0], b[0], s0);
    s1 = fma(a[1], b[1], s1);
    s2 = fma(a[2], b[2], s2);
    s3 = fma(a[3], b[3], s3);
    s0 = fma(a[4], b[4], s0);
    s1 = fma(a[5], b[5], s1);
    s2 = fma(a[6], b[6], s2);
    s3 = fma(a[7], b[7], s3);
  }
  for (; t < cnt; ++t) s0 = fma(u[t], v[VS * t], s0);
  return (s0 + s1) + (s2 + s3);
}

// out[k] += sum_{n < min(cn, L - k)} xs[n] * xs[n + k], k = 0..p.  A lane owns
// the adjacent lags k, k + 1 (k even): one window of 16-byte LDS reads feeds
// both, eight products each per nine window samples.  xs is 16-byte aligned.
// Each lag is four interleaved chains added in a fixed order, then its tail.
__device__ __forceinline__ void jn_lags(const double* __restrict__ xs, int L, int cn, int p,
                                        double* __restrict__ out) {
  for (int k = 2 * threadIdx.x; k <= p; k += 2 * JN_THREADS) {
    const int c0 = min(cn, L - k);   // products of lag k; lag k + 1 has c1 <= c0
    if (c0 <= 0) continue;
    if (k == p) {
      out[k] += jn_dot<1>(xs, xs + k, c0);
      continue;
    }
    const int c1 = min(cn, L - k - 1);
    const double* __restrict__ v = xs + k;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    int n = 0;
    for (; n + 8 <= c1; n += 8) {
      double u[8], w[9];
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const double2 uu = *reinterpret_cast<const double2*>(xs + n + e);
        const double2 ww = *reinterpret_cast<const double2*>(v + n + e);
        u[e] = uu.x, u[e + 1] = uu.y;
        w[e] = ww.x, w[e + 1] = ww.y;
      }
      w[8] = v[n + 8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e & 3] = fma(u[e], w[e], a[e & 3]);
        b[e & 3] = fma(u[e], w[e + 1], b[e & 3]);
      }
    }
    double s0 = (a[0] + a[1]) + (a[2] + a[3]), s1 = (b[0] + b[1]) + (b[2] + b[3]);
    for (int t = n; t < c0; ++t) s0 = fma(xs[t], v[t], s0);
    for (int t = n; t < c1; ++t) s1 = fma(xs[t], v[t + 1], s1);
    out[k] += s0;
    out[k + 1] += s1;
  }
}

// The recursion of the header comment over t[0..M] (zero beyond p), M steps.
// SOLVE: also T z = g, Z[j] = z_{j-1}.  Returns false (for every lane alike)
// at a non-positive pivot or a non-finite coefficient.
template <bool SOLVE>
__device__ bool jn_levinson(const double* __restrict__ t, int M, double* __restrict__ A,
                            double* __restrict__ Z, const double* __restrict__ g,
                            double (*part)[2][JN_WAVES]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double e = t[0];
  const double t1 = t[1];
  double pa = 0.0, pz = 0.0;   // this lane's share of the step's two sums
  // the pair (j, jp = m + 1 - j): old values in, new values out and into the
  // next step's sums (weights t[m + 2 - j] = t[jp + 1] and t[j + 1])
  struct Pair {
    double aj, ajp, zj, zjp, wj, wjp;
  };
  auto load = [&](int j, int jp) {
    Pair q;
    q.aj = A[j];
    q.ajp = A[jp];
    q.wj = t[jp + 1];
    q.wjp = t[j + 1];
    q.zj = SOLVE ? Z[j] : 0.0;
    q.zjp = SOLVE ? Z[jp] : 0.0;
    return q;
  };
  auto apply = [&](const Pair& q, int j, int jp, double kk, double mu) {
    const double naj = fma(kk, q.ajp, q.aj);
    A[j] = naj;
    pa = fma(naj, q.wj, pa);
    if (SOLVE) {
      const double nzj = fma(mu, q.ajp, q.zj);
      Z[j] = nzj;
      pz = fma(nzj, q.wj, pz);
    }
    if (j != jp) {
      const double najp = fma(kk, q.aj, q.ajp);
      A[jp] = najp;
      pa = fma(najp, q.wjp, pa);
      if (SOLVE) {
        const double nzjp = fma(mu, q.aj, q.zjp);
        Z[jp] = nzjp;
        pz = fma(nzjp, q.wjp, pz);
      }
    }
  };
  for (int m = 0; m < M; ++m) {
    pa = jn_wave_sum(pa);
    if (SOLVE) pz = jn_wave_sum(pz);
    if (lane == 0) {
      part[m & 1][0][wave] = pa;
      if (SOLVE) part[m & 1][1][wave] = pz;
    }
    __syncthreads();
    // the first two pairs of the lane are requested from LDS together with the
    // partial sums, before the coefficients that will update them are known
    const int j = 1 + tid, jp = m + 1 - j, j2 = j + JN_THREADS, jp2 = jp - JN_THREADS;
    const bool one = 2 * j <= m + 1, two = 2 * j2 <= m + 1;
    Pair q, q2;
    if (one) q = load(j, jp);
    if (two) q2 = load(j2, jp2);
    double da = part[m & 1][0][0], dz = SOLVE ? part[m & 1][1][0] : 0.0;
#pragma unroll
    for (int w = 1; w < JN_WAVES; ++w) {
      da += part[m & 1][0][w];
      if (SOLVE) dz += part[m & 1][1][w];
    }
    if (!(e > 0.0) || !isfinite(e)) return false;
    const double inv = jn_rcp(e);
    const double kk = -(t[m + 1] + da) * inv;
    const double mu = SOLVE ? (g[m] - dz) * inv : 0.0;
    if (!isfinite(kk) || !isfinite(mu)) return false;
    pa = 0.0;
    pz = 0.0;
    if (one) apply(q, j, jp, kk, mu);
    if (two) apply(q2, j2, jp2, kk, mu);
    for (int j3 = j2 + JN_THREADS; 2 * j3 <= m + 1; j3 += JN_THREADS)   // m > 1024 only
      apply(load(j3, m + 1 - j3), j3, m + 1 - j3, kk, mu);
    if (tid == 0) {
      A[m + 1] = kk;
      pa = fma(kk, t1, pa);
      if (SOLVE) {
        Z[m + 1] = mu;
        pz = fma(mu, t1, pz);
      }
    }
    e *= 1.0 - kk * kk;
  }
  return true;
}

// grid: one workgroup per segment.  dynamic LDS: JnLds.
__global__ __launch_bounds__(JN_THREADS) void janssen_kernel(
    double* sol, int64_t n_segments, int64_t stride, const int32_t* __restrict__ n_,
    const int32_t* __restrict__ gap_start, const int32_t* __restrict__ gap_len, int p, int maxit,
    double* __restrict__ history, int32_t* __restrict__ iters_done, int nB, int nA, int nY,
    int S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double part[2][2][JN_WAVES];
  __shared__ int s_hmax[JN_WAVES];
  __shared__ int s_bad;
  double* B = reinterpret_cast<double*>(smem);
  double* A = B + nB;
  double* Y = A + nA;
  double* W = Y + nY;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t seg = blockIdx.x;

  // history's row length: the longest gap of the batch
  int hrow = 0;
  if (history) {
    for (int64_t i = tid; i < n_segments; i += JN_THREADS)
      hrow = max(hrow, min(max(gap_len[i], 0), JN_HMAX));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hrow = max(hrow, __shfl_xor(hrow, o, 64));
    if (lane == 0) s_hmax[wave] = hrow;
    __syncthreads();
    hrow = s_hmax[0];
#pragma unroll
    for (int w = 1; w < JN_WAVES; ++w) hrow = max(hrow, s_hmax[w]);
  }

  const int N = n_[seg], s = gap_start[seg], h = gap_len[seg];
  // a segment the tables describe outside the supported range is left alone
  if (N <= p || N > JN_NMAX || (int64_t)N > stride || h < 1 || h > JN_HMAX || h > nY || s < 0 ||
      (int64_t)s + h > N) {
    if (tid == 0) iters_done[seg] = -1;
    return;
  }
  double* x = sol + seg * stride;
  for (int i = tid; i < h; i += JN_THREADS) x[s + i] = 0.0;
  for (int k = p + 1 + tid; k < nB; k += JN_THREADS) B[k] = 0.0;   // stays zero
  __syncthreads();

  // a chunk holds the products that start at C samples and the p samples after
  // them; a segment that fits W whole is one chunk
  const int C = N <= S ? N : S - p;
  int done = 0;
  for (int it = 0; it < maxit; ++it) {
    // 1. autocorrelation of the current solution
    for (int k = tid; k <= p; k += JN_THREADS) B[k] = 0.0;
    if (tid == 0) {
      A[0] = 1.0;
      s_bad = 0;
    }
    for (int c0 = 0; c0 < N; c0 += C) {
      const int L = min(S, N - c0);
      __syncthreads();   // the previous chunk (or Z) is no longer read
      for (int i = tid; i < L; i += JN_THREADS) W[i] = x[c0 + i];
      __syncthreads();
      jn_lags(W, L, min(C, N - c0), p, B);
    }
    __syncthreads();
    const double r0 = B[0];
    if (!(r0 > 0.0) || !isfinite(r0)) break;   // silent (or unusable) context

    // 2. AR coefficients
    if (!jn_levinson<false>(B, p, A, nullptr, nullptr, part)) break;
    __syncthreads();

    // 3. their autocorrelation, over r
    for (int k = tid; k <= p; k += JN_THREADS) B[k] = 0.0;
    __syncthreads();
    jn_lags(A, p + 1, p + 1, p, B);

    // 4. right-hand side from the observed samples within p of the gap
    const int l0 = max(0, s - p), LL = s - l0;
    const int RL = min(N, s + h + p) - (s + h);
    double* WL = W;
    double* WR = W + LL;
    for (int i = tid; i < LL; i += JN_THREADS) WL[i] = x[l0 + i];
    for (int i = tid; i < RL; i += JN_THREADS) WR[i] = x[s + h + i];
    __syncthreads();
    for (int ii = tid; ii < h; ii += JN_THREADS) {
      // left: d = ii + 1 + t, j = s - 1 - t; right: d = h - ii + t, j = s + h + t
      const int cl = min(p - ii, LL), cr = min(p - (h - ii) + 1, RL);
      double acc = 0.0;
      if (cl > 0) acc = jn_dot<-1>(B + ii + 1, WL + LL - 1, cl);
      if (cr > 0) acc += jn_dot<1>(B + (h - ii), WR, cr);
      Y[ii] = -acc;
    }
    __syncthreads();

    // 5. the gap samples
    const bool ok = jn_levinson<true>(B, h, A, W, Y, part);
    __syncthreads();
    if (!ok) break;
    for (int j = 1 + tid; j <= h; j += JN_THREADS)
      if (!isfinite(W[j])) s_bad = 1;
    __syncthreads();
    if (s_bad) break;

    // 6. accept the iterate
    double* hist = history ? history + ((seg * maxit + it) * (int64_t)hrow) : nullptr;
    for (int j = 1 + tid; j <= h; j += JN_THREADS) {
      const double z = W[j];
      x[s + j - 1] = z;
      if (hist) hist[j - 1] = z;
    }
    done = it + 1;
    __syncthreads();
  }
  if (tid == 0) iters_done[seg] = done;
}

static int jn_unsupported(const char* msg) {
  record_msg(msg);
  return AINP_EUNSUPPORTED;
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_janssen_workspace(int64_t n_segments, int n_max, int p, int gap_max) {
  // every recursion vector fits LDS over the whole supported range and the
  // signal is read in place, so no shape needs global scratch
  (void)n_segments;
  (void)n_max;
  (void)p;
  (void)gap_max;
  return 0;
}

extern "C" int ainp_janssen(double* sol, int64_t n_segments, int64_t stride, const int32_t* n,
                            const int32_t* gap_start, const int32_t* gap_len, int p, int maxit,
                            double* history, int32_t* iters_done, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!sol || !n || !gap_start || !gap_len || !iters_done || n_segments < 0 || stride < 1)
    return record_msg("ainp_janssen: bad argument");
  if (p < 1 || maxit < 1) return record_msg("ainp_janssen: bad argument (p >= 1, maxit >= 1)");
  if (p > JN_PMAX || maxit > JN_ITMAX)
    return jn_unsupported("ainp_janssen: unsupported (p <= 3072, maxit <= 1000)");
  if (stride <= p) return record_msg("ainp_janssen: bad argument (p < n <= stride)");
  const int64_t n_max = std::min<int64_t>(stride, JN_NMAX);
  if (workspace_bytes < ainp_janssen_workspace(n_segments, (int)n_max, p, JN_HMAX) ||
      (workspace_bytes && !workspace))
    return record_msg("ainp_janssen: workspace too small");
  if (n_segments > 0x7fffffff)
    return jn_unsupported("ainp_janssen: too many segments");
  if (n_segments == 0) return AINP_OK;
  const JnLds l = jn_lds(n_max, p);
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)janssen_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)jn_lds(JN_NMAX, JN_PMAX).bytes()) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_janssen: cannot reserve the recursion vectors' LDS");
  hipLaunchKernelGGL(janssen_kernel, dim3((unsigned)n_segments), dim3(JN_THREADS), l.bytes(),
                     as_stream(stream), sol, n_segments, stride, n, gap_start, gap_len, p, maxit,
                     history, iters_done, l.nB, l.nA, l.nY, l.S);
  return check_launch("ainp_janssen");
}
