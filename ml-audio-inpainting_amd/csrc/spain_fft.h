// spain_fft.h — what the SPAIN kernels share (spain.hip, spain_omp.hip,
// spain_learned.hip; basis_learn.hip takes the sum; gap_phase.hip takes the
// transform, one wave per frame with the wave-level barrier): the length-M real
// transform as an M/2-point complex transform on split, skewed re / im arrays
// in LDS with quarter-wave twiddles, the slots a lane holds of a half spectrum,
// the fixed-order workgroup sum and the radix select with its tie rule.
// spain.hip's header describes the scheme; spain_plan.h sizes the arrays.
#pragma once
#include "common.h"

namespace ainp {

struct cplx {
  double re, im;
};
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ cplx cmulc(cplx a, cplx b) {   // a * conj(b)
  return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}
__device__ __forceinline__ double cabs2(cplx a) { return a.re * a.re + a.im * a.im; }
__device__ __forceinline__ int sp_pad(int i) { return i + (i >> 5); }

// The quarter wave ct[j] = cos(2 pi j / M), j <= M/4; no barrier.
template <int NT>
__device__ __forceinline__ void sp_quarter_wave(double* ct, int M, int tid) {
  for (int j = tid; j <= M / 4; j += NT) ct[j] = cospi((double)(2 * j) / (double)M);
}

// exp(-2 pi i idx / M), 0 <= idx < M/2, from the quarter wave ct[0 .. M/4]
__device__ __forceinline__ cplx sp_tw(const double* ct, int idx, int M) {
  const int q = M >> 2;
  if (idx <= q) return {ct[idx], -ct[q - idx]};
  return {-ct[2 * q - idx], -ct[idx - q]};
}

struct SpFft {
  double* re;
  double* im;
  const double* ct;
  int N, lgN, M;
  __device__ __forceinline__ cplx ld(int i) const {
    const int a = sp_pad(i);
    return {re[a], im[a]};
  }
  __device__ __forceinline__ void st(int i, cplx v) const {
    const int a = sp_pad(i);
    re[a] = v.re;
    im[a] = v.im;
  }
  __device__ __forceinline__ int brev(int k) const { return (int)(__brev((unsigned)k) >> (32 - lgN)); }
};

// The transforms' barrier: the workgroup's, or (WAVE) the wave's own, for a
// wave that transforms in arrays of its own with tid = its lane and NT = 64.
template <bool WAVE>
__device__ __forceinline__ void sp_barrier() {
  if (WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// In place, natural order in, bit-reversed order out.  Block size s: a at
// b + j, c at b + j + s/2 become a + c and (a - c) W_s^j.  Ends on a barrier.
template <int NT, bool WAVE = false>
__device__ void sp_dif(const SpFft& f, int tid) {
  const int N = f.N, M = f.M;
  int s = N;
  if (f.lgN & 1) {
    for (int t = tid; t < N / 2; t += NT) {
      const cplx a = f.ld(t), c = f.ld(t + N / 2);
      f.st(t, cadd(a, c));
      f.st(t + N / 2, cmul(csub(a, c), sp_tw(f.ct, 2 * t, M)));   // W_N^t = W_M^2t
    }
    sp_barrier<WAVE>();
    s >>= 1;
  }
  for (; s >= 4; s >>= 2) {
    const int q = s >> 2, step = M / s;   // W_s^j = W_M^(j step)
    for (int t = tid; t < N / 4; t += NT) {
      const int j = t & (q - 1), i0 = ((t - j) << 2) + j;
      const cplx a0 = f.ld(i0), a1 = f.ld(i0 + q), a2 = f.ld(i0 + 2 * q), a3 = f.ld(i0 + 3 * q);
      const cplx w1 = sp_tw(f.ct, j * step, M), w2 = sp_tw(f.ct, 2 * j * step, M);
      const cplx t0 = cadd(a0, a2), t1 = cadd(a1, a3);
      const cplx t2 = cmul(csub(a0, a2), w1);
      const cplx d = cmul(csub(a1, a3), w1);
      const cplx t3 = {d.im, -d.re};   // W_s^(j + s/4) = -i W_s^j
      f.st(i0, cadd(t0, t1));
      f.st(i0 + q, cmul(csub(t0, t1), w2));
      f.st(i0 + 2 * q, cadd(t2, t3));
      f.st(i0 + 3 * q, cmul(csub(t2, t3), w2));
    }
    sp_barrier<WAVE>();
  }
}

// The transpose: bit-reversed in, natural out, conjugate twiddles, no 1 / N.
// a and c conj(W_s^j) become a + c and a - c.  Ends on a barrier.
template <int NT, bool WAVE = false>
__device__ void sp_dit(const SpFft& f, int tid) {
  const int N = f.N, M = f.M;
  const int top = (f.lgN & 1) ? N / 2 : N;
  for (int s = 4; s <= top; s <<= 2) {
    const int q = s >> 2, step = M / s;
    for (int t = tid; t < N / 4; t += NT) {
      const int j = t & (q - 1), i0 = ((t - j) << 2) + j;
      const cplx a0 = f.ld(i0), a1 = f.ld(i0 + q), a2 = f.ld(i0 + 2 * q), a3 = f.ld(i0 + 3 * q);
      const cplx w1 = sp_tw(f.ct, j * step, M), w2 = sp_tw(f.ct, 2 * j * step, M);
      const cplx c1 = cmulc(a1, w2), c3 = cmulc(a3, w2);
      const cplx t0 = cadd(a0, c1), t1 = csub(a0, c1), t2 = cadd(a2, c3), t3 = csub(a2, c3);
      const cplx e2 = cmulc(t2, w1);
      const cplx d = cmulc(t3, w1);
      const cplx e3 = {-d.im, d.re};   // conj(-i W_s^j) = i conj(W_s^j)
      f.st(i0, cadd(t0, e2));
      f.st(i0 + 2 * q, csub(t0, e2));
      f.st(i0 + q, cadd(t1, e3));
      f.st(i0 + 3 * q, csub(t1, e3));
    }
    sp_barrier<WAVE>();
  }
  if (f.lgN & 1) {
    for (int t = tid; t < N / 2; t += NT) {
      const cplx a = f.ld(t), c = cmulc(f.ld(t + N / 2), sp_tw(f.ct, 2 * t, M));
      f.st(t, cadd(a, c));
      f.st(t + N / 2, csub(a, c));
    }
    sp_barrier<WAVE>();
  }
}

// A lane's slots of the half spectrum X[0 .. N]: slot p >= 1 holds a = X[p]
// and b = X[N - p]; slot 0 holds a = (X[0], X[N]) (both real) and b = X[N/2].
template <int EPL>
struct SpSpec {
  cplx a[EPL], b[EPL];
};

// The N-point spectrum C of c[n] = x[2n] + i x[2n+1] (bit-reversed in LDS) ->
// scale * FFT_M(x): with W = exp(-2 pi i p / M),
//   E = (C[p] + conj C[N-p]) / 2,  O = -i (C[p] - conj C[N-p]) / 2,
//   X[p] = E + W O,  X[N-p] = conj(E) - conj(W O).
template <int NT, int EPL>
__device__ void sp_split(const SpFft& f, int tid, double scale, SpSpec<EPL>& X) {
  const int N = f.N;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int p = tid + e * NT;
    if (p >= N / 2) continue;
    if (p == 0) {
      const cplx c0 = f.ld(0), cm = f.ld(f.brev(N / 2));
      X.a[e] = {(c0.re + c0.im) * scale, (c0.re - c0.im) * scale};
      X.b[e] = {cm.re * scale, -cm.im * scale};
    } else {
      const cplx ck = f.ld(f.brev(p)), cn = f.ld(f.brev(N - p));
      const cplx E = {0.5 * (ck.re + cn.re), 0.5 * (ck.im - cn.im)};
      const cplx O = {0.5 * (ck.im + cn.im), -0.5 * (ck.re - cn.re)};
      const cplx wo = cmul(O, sp_tw(f.ct, p, f.M));
      X.a[e] = {(E.re + wo.re) * scale, (E.im + wo.im) * scale};
      X.b[e] = {(E.re - wo.re) * scale, (wo.im - E.im) * scale};
    }
  }
}

// The reverse: a Hermitian half spectrum X -> C (bit-reversed in LDS) with
// IFFT_N(C)[n] = x[2n] + i x[2n+1] for x = IFFT_M(X):
//   E = (X[p] + conj X[N-p]) / 2,  O = conj(W) (X[p] - conj X[N-p]) / 2,
//   C[p] = E + i O,  C[N-p] = conj(E) + i conj(O).
template <int NT, int EPL>
__device__ void sp_merge(const SpFft& f, int tid, const SpSpec<EPL>& X) {
  const int N = f.N;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int p = tid + e * NT;
    if (p >= N / 2) continue;
    if (p == 0) {
      f.st(0, {0.5 * (X.a[e].re + X.a[e].im), 0.5 * (X.a[e].re - X.a[e].im)});
      f.st(f.brev(N / 2), {X.b[e].re, -X.b[e].im});
    } else {
      const cplx A = X.a[e], B = X.b[e];
      const cplx E = {0.5 * (A.re + B.re), 0.5 * (A.im - B.im)};
      const cplx F = {0.5 * (A.re - B.re), 0.5 * (A.im + B.im)};
      const cplx O = cmulc(F, sp_tw(f.ct, p, f.M));
      f.st(f.brev(p), {E.re - O.im, E.im + O.re});
      f.st(f.brev(N - p), {E.re + O.im, O.re - E.im});
    }
  }
}

// Fixed-order sum over the workgroup; every lane gets the same value.
// Barriers: one before the slots are read, one after (the slots are free again).
template <int NT>
__device__ double sp_sum(double v, double* part, int tid) {
  v = wave_sum_d(v);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int wv = 1; wv < NT / 64; ++wv) s += part[wv];
  __syncthreads();
  return s;
}

// The radix select: among the keys with member[i], find the value of the k-th
// largest (1 <= k <= their number), digit by digit from `shift` down.  Returns
// in sel: [0] unused, [1] how many of the keys equal to the result down to the
// returned shift are wanted, [2] how many there are.  prefix / shift: a key is
// above the cut when key >> shift > prefix >> shift, on it when equal.
template <int NT, int NK>
__device__ void sp_select(const uint64_t (&key)[NK], const bool (&member)[NK], int k,
                          int shift, uint32_t* hist, int* sel, int tid, uint64_t& prefix,
                          int& out_shift, int& need, int& have) {
  prefix = 0;
  int remaining = k;
  for (;; shift -= 8) {
    for (int i = tid; i < 256; i += NT) hist[i] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NK; ++i)
      if (member[i] && (shift >= 56 || (key[i] >> (shift + 8)) == (prefix >> (shift + 8))))
        atomicAdd(&hist[(key[i] >> shift) & 255], 1u);
    __syncthreads();
    if (tid < 64) {
      int c[4], tot = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) tot += c[b] = (int)hist[4 * tid + b];
      int v = tot;   // -> the count of this lane's digits and all above
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(v, o, 64);
        if (tid + o < 64) v += t;
      }
      int above = v - tot;
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        if (above < remaining && remaining <= above + c[b]) {
          sel[0] = 4 * tid + b;
          sel[1] = above;
          sel[2] = c[b];
        }
        above += c[b];
      }
    }
    __syncthreads();
    prefix |= (uint64_t)sel[0] << shift;
    remaining -= sel[1];
    have = sel[2];
    if (have == remaining || shift == 0) break;
  }
  out_shift = shift;
  need = remaining;
}

// keep[i]: key[i] is among the k largest of the `count` keys with member[i].
// Equal keys kept only in part go to the lower bin[i], by a second select over
// the bins of the members on the cut.  k >= count keeps all, without a barrier.
template <int NT, int NK>
__device__ __forceinline__ void sp_keep_largest(const uint64_t (&key)[NK], const bool (&member)[NK],
                                                const int (&bin)[NK], int k, int count,
                                                uint32_t* hist, int* sel, int tid,
                                                bool (&keep)[NK]) {
  if (k >= count) {
#pragma unroll
    for (int i = 0; i < NK; ++i) keep[i] = member[i];
    return;
  }
  uint64_t prefix, prefix2 = 0;
  int shift, need, have, shift2 = 0;
  sp_select<NT, NK>(key, member, k, 56, hist, sel, tid, prefix, shift, need, have);
  const bool tie = need < have;
  bool member2[NK];
  uint64_t key2[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    member2[i] = member[i] && (key[i] >> shift) == (prefix >> shift);
    key2[i] = (uint64_t)(0xffff - bin[i]);
  }
  if (tie) {
    int need2, have2;
    sp_select<NT, NK>(key2, member2, need, 8, hist, sel, tid, prefix2, shift2, need2, have2);
  }
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const bool above = member[i] && (key[i] >> shift) > (prefix >> shift);
    keep[i] = above || (member2[i] && (!tie || (key2[i] >> shift2) >= (prefix2 >> shift2)));
  }
}

}  // namespace ainp
