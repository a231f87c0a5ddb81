// ar_fit.h — device routines shared by the autoregressive baselines
// (janssen.hip, ar_extrapolate.hip): the fixed-order wave / workgroup sums, the
// lag sums and the Levinson recursion of the "lpc" estimator, and the Burg
// estimator.  All arithmetic float64.  NT is the workgroup size of the caller;
// the "lpc" Janssen kernel instantiates everything with NT = 256.
#pragma once
#include <math.h>

#include "ar_limits.h"
#include "common.h"

namespace ainp {

constexpr int JN_THREADS = 256;

// The Burg estimator keeps its two error vectors in registers: 512 lanes, 32
// consecutive elements of each vector per lane (2 x 32 doubles = 128 VGPRs of
// the 256 a lane has at 8 waves per CU), which covers JN_NMAX.  At 1024 lanes
// x 16 elements the vectors take 64 of 128 VGPRs and the step itself needs
// some 45 more, which leaves a kernel around it nothing: it spilled.
constexpr int BG_THREADS = 512;
constexpr int BG_WAVES = BG_THREADS / 64;
constexpr int BG_E = JN_NMAX / BG_THREADS;
constexpr int BG_XROW = BG_THREADS + 2;      // one exchange row (doubles)
constexpr int BG_XY = 4 * BG_XROW;           // [step parity][ef | eb][lane + 1]

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

// The sum of the NW per-wave slots of a workgroup, after the barrier that
// published them; the same bits in every lane.  Four waves: added in wave
// order.  Eight (sixteen) waves: lane l reads slot l & 7 (l & 15) and DPP
// stages sum the half row (row) -- one LDS read and a fixed tree.
template <int NW>
__device__ __forceinline__ double jn_slot_sum(const double* slot) {
  static_assert(NW == 16 || NW == 8 || NW <= 4, "a DPP row holds sixteen slots");
  if constexpr (NW >= 8) {
    double v = slot[threadIdx.x & (NW - 1)];
    v += jn_dpp<0xB1>(v);                        // quad_perm [1, 0, 3, 2]
    v += jn_dpp<0x4E>(v);                        // quad_perm [2, 3, 0, 1]
    v += jn_dpp<0x141>(v);                       // row_half_mirror
    if constexpr (NW == 16) v += jn_dpp<0x140>(v);   // row_mirror
    return v;
  } else {
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += slot[w];
    return s;
  }
}

// sum over the workgroup, the same bits in every lane and on every call: wave
// sums, one slot per wave, added in wave order.  Two barriers; slot is free
// again on return.
template <int NT>
__device__ __forceinline__ double jn_block_sum(double v, double* slot) {
  v = jn_wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = jn_slot_sum<NT / 64>(slot);
  __syncthreads();
  return s;
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
template <int NT>
__device__ __forceinline__ void jn_lags(const double* __restrict__ xs, int L, int cn, int p,
                                        double* __restrict__ out) {
  for (int k = 2 * threadIdx.x; k <= p; k += 2 * NT) {
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

// The recursion of janssen.hip's header comment over t[0..M] (zero beyond p),
// M steps.  SOLVE: also T z = g, Z[j] = z_{j-1}.  Returns false (for every lane
// alike) at a non-positive pivot or a non-finite coefficient.
template <bool SOLVE, int NT>
__device__ bool jn_levinson(const double* __restrict__ t, int M, double* __restrict__ A,
                            double* __restrict__ Z, const double* __restrict__ g,
                            double (*part)[2][NT / 64]) {
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
    const int j = 1 + tid, jp = m + 1 - j, j2 = j + NT, jp2 = jp - NT;
    const bool one = 2 * j <= m + 1, two = 2 * j2 <= m + 1;
    Pair q, q2;
    if (one) q = load(j, jp);
    if (two) q2 = load(j2, jp2);
    const double da = jn_slot_sum<NT / 64>(part[m & 1][0]);
    const double dz = SOLVE ? jn_slot_sum<NT / 64>(part[m & 1][1]) : 0.0;
    if (!(e > 0.0) || !isfinite(e)) return false;
    const double inv = jn_rcp(e);
    const double kk = -(t[m + 1] + da) * inv;
    const double mu = SOLVE ? (g[m] - dz) * inv : 0.0;
    if (!isfinite(kk) || !isfinite(mu)) return false;
    pa = 0.0;
    pz = 0.0;
    if (one) apply(q, j, jp, kk, mu);
    if (two) apply(q2, j2, jp2, kk, mu);
    for (int j3 = j2 + NT; 2 * j3 <= m + 1; j3 += NT)   // m > 4 NT only
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

// Burg's estimator (MATLAB arburg, real input) of order p on the N > p samples
// x[i] = c[DIR i] - mean, i < N (DIR = -1 reads a context backwards), for a
// workgroup of BG_THREADS: A[0..p] in LDS.
//   ef = x[1:], eb = x[:-1];  for m = 1..p:
//   k = -2 sum(eb ef) / (sum(ef^2) + sum(eb^2)),  (ef, eb) <- (ef + k eb, eb + k ef),
//   drop ef's first and eb's last element,  a <- [a, 0] + k [0, reverse(a)].
// Lane t keeps elements 32 t .. 32 t + 31 of both vectors in registers, zero
// from the current length on, so the sums need no mask.  Dropping ef's first
// element moves ef down by one: 31 register renames and one element from
// lane t + 1.  That lane's old (ef[0], eb[0]) travel through LDS with the
// partial sums, before k is known, and the receiver forms the same fma -- so
// a step is: lane sums -> wave reduce -> one LDS slot per wave -> one barrier
// -> every lane adds the slots in a fixed order -> update.  A wave whose 2048
// elements lie beyond the current length holds zeros and skips the arithmetic.
// XY: BG_XY doubles of LDS; part: the slots.  Returns false (for every lane
// alike) when the denominator is not positive and finite or k is not finite;
// A then holds the coefficients of the steps completed.
template <int DIR>
__device__ bool burg_fit(const double* __restrict__ c, double mean, int N, int p,
                         double* __restrict__ A, double* __restrict__ XY,
                         double (*part)[2][BG_WAVES]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = BG_E * tid;
  double ef[BG_E], eb[BG_E];
  {
    // DIR is a constant so that the loads share one address register
    const double* __restrict__ q = c + DIR * base;
    double v[BG_E + 1];
#pragma unroll
    for (int j = 0; j <= BG_E; ++j) v[j] = base + j < N ? q[DIR * j] - mean : 0.0;
#pragma unroll
    for (int j = 0; j < BG_E; ++j) {
      const bool in = base + j < N - 1;
      eb[j] = in ? v[j] : 0.0;
      ef[j] = in ? v[j + 1] : 0.0;
    }
  }
  __syncthreads();   // whoever used XY, part or A before is done
  if (tid == 0) {
    A[0] = 1.0;
    // the neighbour of the last lane: nothing, in both parities and vectors
    XY[BG_THREADS] = XY[BG_XROW + BG_THREADS] = 0.0;
    XY[2 * BG_XROW + BG_THREADS] = XY[3 * BG_XROW + BG_THREADS] = 0.0;
  }
  for (int m = 0; m < p; ++m) {
    const int L = N - 1 - m;                        // current length of ef, eb
    const bool active = wave * (64 * BG_E) < L;     // wave-uniform
    double pn = 0.0, pd = 0.0;
    if (active) {
#pragma unroll
      for (int e = 0; e < BG_E; ++e) {
        pn = fma(ef[e], eb[e], pn);
        pd = fma(ef[e], ef[e], pd);
        pd = fma(eb[e], eb[e], pd);
      }
      pn = jn_wave_sum(pn);
      pd = jn_wave_sum(pd);
    }
    double* X = XY + (m & 1) * 2 * BG_XROW;
    double* Y = X + BG_XROW;
    if (lane == 0) {
      part[m & 1][0][wave] = pn;
      part[m & 1][1][wave] = pd;
    }
    X[tid] = ef[0];
    Y[tid] = eb[0];
    __syncthreads();
    const double num = jn_slot_sum<BG_WAVES>(part[m & 1][0]);
    const double den = jn_slot_sum<BG_WAVES>(part[m & 1][1]);
    if (!(den > 0.0) || !isfinite(den)) return false;
    const double k = -2.0 * num * jn_rcp(den);
    if (!isfinite(k)) return false;
    // the lane's pairs (j, m + 1 - j) of a; their LDS round trip hides behind
    // the update of the error vectors below
    for (int j = 1 + tid; 2 * j <= m + 1; j += BG_THREADS) {
      const int jp = m + 1 - j;
      const double aj = A[j], ajp = A[jp];
      A[j] = fma(k, ajp, aj);
      if (j != jp) A[jp] = fma(k, aj, ajp);
    }
    if (tid == 0) A[m + 1] = k;
    if (active) {
#pragma unroll
      for (int e = 0; e < BG_E; ++e) {
        const double f = ef[e], b = eb[e];
        eb[e] = fma(k, f, b);
        if (e > 0) ef[e - 1] = fma(k, b, f);
      }
      ef[BG_E - 1] = fma(k, Y[tid + 1], X[tid + 1]);
      // eb's last element, index L - 1, leaves; ef's there is zero already
      const int jz = L - 1 - base;
      if ((unsigned)jz < (unsigned)BG_E) {
#pragma unroll
        for (int e = 0; e < BG_E; ++e)
          if (e == jz) eb[e] = 0.0;
      }
    }
  }
  return true;
}

}  // namespace ainp
