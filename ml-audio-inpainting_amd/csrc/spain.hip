// spain.hip — A-SPAIN and S-SPAIN sparse audio inpainting of one window per
// workgroup (references/spain/aspain.m and sspain.m with f_update = 'H', driven
// by spain_segmentation.m; restated in DESIGN §14).  All arithmetic float64.
//
// A row is one window of w samples with one run of missing samples.  The frame
// is the zero-padded unitary DFT of length M = red * w:
//   A x = FFT_M([x; 0]) / sqrt(M),   A* z = (IFFT_M(z) sqrt(M))[0 .. w).
// Both algorithms are an ADMM loop of: forward transform, keep the k largest
// of the M/2 + 1 half-spectrum coefficients (H_k), inverse transform, put the
// observed samples back; k grows by s every r passes.  The pass with the
// smallest objective so far copies the iterate it was evaluated on into the
// row's gap in `sol`, which is the result.
//
// One workgroup owns one row for all passes; rows stop at different passes and
// share nothing.  What lives where (the transforms, the slots, the sum and the
// select are in spain_fft.h, which spain_learned.hip uses too):
//   * the length-M real transforms are N = M/2 point complex transforms on
//     split re / im arrays in LDS, in place: forward decimation-in-frequency
//     from natural to bit-reversed order, inverse decimation-in-time back, two
//     radix-2 stages fused per barrier (a radix-4 pass), one radix-2 pass first
//     or last when log2 N is odd.  Nothing is ever reordered: the real-transform
//     split that follows (precedes) reads (writes) bin k at brev(k).
//   * element i of an array lies at i + i / 32: with 8-byte accesses the 64
//     banks take one 32-lane group of consecutive doubles per cycle, and the
//     skew keeps the strided passes (strides 2 .. 32 doubles) on distinct banks.
//   * the half spectrum lives in registers.  A lane owns "slots" p = tid +
//     e * NT < N/2, each the bin pair (p, N - p) that the real-transform split
//     produces together; slot 0 holds the three self-paired bins (DC and
//     Nyquist, both real, packed into one complex value, and bin N/2).  A-SPAIN
//     keeps z, u and the thresholded z-bar there (3 x 2 complex values per slot),
//     S-SPAIN its time-domain u (4 samples per slot).
//   * twiddles: one quarter wave cos(2 pi j / M), j <= M/4, built once per
//     workgroup with cospi (exact arguments, M is a power of two); every
//     other angle of the half circle is an index reflection.
//   * H_k is a radix select over the bit patterns of the squared magnitudes
//     (non-negative doubles order as unsigned integers): 8-bit digits from the
//     top, a 256-bin histogram with integer LDS atomics, one wave scans it.  It
//     stops at the first digit whose bin is kept whole.  Equal magnitudes that
//     are kept only in part go to the lower bin index by a second select over
//     the indices.  DC is ranked by half its magnitude, Nyquist is not
//     (hard_thresholding.m's quirk).
//   * sums (the objective) are per-lane in slot order, a butterfly over the
//     wave, one LDS slot per wave, added in wave order by every lane: the same
//     bits on every call, and every lane takes the same branch.
//
// LDS at the largest shape (w 4096, red 2: M 8192, N 4096), bytes:
//   re, im   2 x (4096 + 128) x 8 = 67584     the transform, skewed
//   row      4096 x 8             = 32768     the iterate x-hat (observed
//                                             samples never change; the run is
//                                             known by its bounds, no flags)
//   cos      (2048 + 1) x 8       = 16392     the quarter wave
//   static   histogram 1024 + wave sums and the select's result < 256
// 117 KiB of the 160 KiB: one workgroup per CU there.  N <= 1024 runs 256 lanes
// with 2 slots a lane, longer transforms 512 lanes with up to 4: at 1024 lanes
// and 2 slots the 128 registers a lane has left spill (196 bytes of scratch a
// lane in A-SPAIN), and A-SPAIN measured 6 % (one row) to 16 % (256 rows) slower
// than at 512 lanes, S-SPAIN 5 % faster.
#include <algorithm>
#include <cmath>

#include "ar_limits.h"
#include "common.h"
#include "spain_fft.h"

namespace ainp {

constexpr int SP_WMIN = 8, SP_WMAX = 4096, SP_MMAX = 8192;
// Per lane: EPL spectrum slots, 2 EPL time-domain sample pairs, and NK = 2 EPL
// + 1 half-spectrum bins to rank (template parameters of what follows).
constexpr int SP_NMAX_256 = 1024;   // the longest transform the 256-lane kernel takes (EPL 2)
constexpr int SP_NT_BIG = 512;      // lanes of the kernel for the longer ones, up to N = 4096
constexpr int SP_EPL_BIG = 2048 / SP_NT_BIG;

struct SpLds {
  int nF, nRow, nCos;   // doubles: one of re / im, the row, the quarter wave
  size_t bytes() const { return ((size_t)2 * nF + nRow + nCos) * sizeof(double); }
};
static SpLds sp_lds(int w, int M) {
  SpLds l;
  const int N = M / 2;
  l.nF = N + N / 32 + 2;
  l.nRow = w;
  l.nCos = (M / 4 + 2) & ~1;
  return l;
}

// H_k on a lane's slots: keep[e][0 / 1] for a / b, keepx for the Nyquist half
// of slot 0.  V is the half spectrum to rank, bins 0 .. N.
template <int NT, int EPL>
__device__ void sp_hard_threshold(const SpSpec<EPL>& V, int N, int k, uint32_t* hist, int* sel,
                                  int tid, bool (&keep)[2 * EPL + 1]) {
  constexpr int SP_NK = 2 * EPL + 1;
  uint64_t key[SP_NK];
  bool member[SP_NK];
  int bin[SP_NK];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int p = tid + e * NT;
    const bool ok = p < N / 2;
    member[2 * e] = member[2 * e + 1] = ok;
    double ka = 0.0, kb = 0.0;
    if (ok) {
      // DC ranks by half its magnitude: a quarter of the square
      ka = p == 0 ? 0.25 * V.a[e].re * V.a[e].re : cabs2(V.a[e]);
      kb = cabs2(V.b[e]);
    }
    key[2 * e] = (uint64_t)__double_as_longlong(ka);
    key[2 * e + 1] = (uint64_t)__double_as_longlong(kb);
    bin[2 * e] = p;
    bin[2 * e + 1] = p == 0 ? N / 2 : N - p;
  }
  member[SP_NK - 1] = tid == 0;   // the Nyquist bin, not halved
  key[SP_NK - 1] = tid == 0 ? (uint64_t)__double_as_longlong(V.a[0].im * V.a[0].im) : 0;
  bin[SP_NK - 1] = N;
  if (k >= N + 1) {
#pragma unroll
    for (int i = 0; i < SP_NK; ++i) keep[i] = member[i];
    __syncthreads();
    return;
  }
  uint64_t prefix, prefix2 = 0;
  int shift, need, have, shift2 = 0;
  sp_select<NT, SP_NK>(key, member, k, 56, hist, sel, tid, prefix, shift, need, have);
  const bool tie = need < have;   // equal squared magnitudes, kept in part: lower bins first
  bool member2[SP_NK];
  uint64_t key2[SP_NK];
#pragma unroll
  for (int i = 0; i < SP_NK; ++i) {
    member2[i] = member[i] && (key[i] >> shift) == (prefix >> shift);
    key2[i] = (uint64_t)(0xffff - bin[i]);
  }
  if (tie) {
    int need2, have2;
    sp_select<NT, SP_NK>(key2, member2, need, 8, hist, sel, tid, prefix2, shift2, need2, have2);
  }
#pragma unroll
  for (int i = 0; i < SP_NK; ++i) {
    const bool above = member[i] && (key[i] >> shift) > (prefix >> shift);
    keep[i] = above || (member2[i] && (!tie || (key2[i] >> shift2) >= (prefix2 >> shift2)));
  }
}

template <int EPL>
__device__ __forceinline__ void sp_apply(SpSpec<EPL>& V, const bool (&keep)[2 * EPL + 1], int tid) {
  constexpr int SP_NK = 2 * EPL + 1;
  const cplx zero = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    if (tid == 0 && e == 0) {
      if (!keep[0]) V.a[0].re = 0.0;
      if (!keep[SP_NK - 1]) V.a[0].im = 0.0;
    } else if (!keep[2 * e]) {
      V.a[e] = zero;
    }
    if (!keep[2 * e + 1]) V.b[e] = zero;
  }
}

// grid: one workgroup of NT lanes per row.  dynamic LDS: SpLds.
template <int NT, int ALG, int EPL>
__global__ __launch_bounds__(NT) void spain_kernel(
    double* sol, int64_t stride, const int32_t* __restrict__ gap_start,
    const int32_t* __restrict__ gap_len, int w, int M, int lgN, int s_step, int r_rate,
    double epsilon, int maxit, int32_t* __restrict__ iters, double* __restrict__ obj_history,
    int nF, int nRow) {
  constexpr int SP_TPL = 2 * EPL, SP_NK = 2 * EPL + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t hist[256];
  __shared__ double part[NT / 64];
  __shared__ int sel[4];
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nF;
  double* xr = im + nF;
  double* ct = xr + nRow;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int N = M / 2;
  const int gs = gap_start[row], gl = gap_len[row];
  double* hrow = obj_history ? obj_history + row * maxit : nullptr;
  // a row whose run does not lie in the window is left alone
  if (gs < 0 || gl < 1 || gl > JN_HMAX || (int64_t)gs + gl > w) {
    if (tid == 0) iters[row] = 0;
    if (hrow)
      for (int i = tid; i < maxit; i += NT) hrow[i] = NAN;
    return;
  }
  double* x = sol + row * stride;
  for (int j = tid; j <= M / 4; j += NT) ct[j] = cospi((double)(2 * j) / (double)M);
  for (int i = tid; i < w; i += NT) xr[i] = (i >= gs && i - gs < gl) ? 0.0 : x[i];
  __syncthreads();

  const SpFft f = {re, im, ct, N, lgN, M};
  const double fwd = 1.0 / sqrt((double)M);   // analysis: FFT_M / sqrt(M)
  const double inv = 2.0 / sqrt((double)M);   // synthesis: (N-point sum) sqrt(M) / N
  const cplx zero = {0.0, 0.0};
  SpSpec<EPL> Z, U, ZB;  // A-SPAIN: z, u, z-bar
  double ut[SP_TPL][2];  // S-SPAIN: u
#pragma unroll
  for (int e = 0; e < EPL; ++e) Z.a[e] = Z.b[e] = U.a[e] = U.b[e] = ZB.a[e] = ZB.b[e] = zero;
#pragma unroll
  for (int e = 0; e < SP_TPL; ++e) ut[e][0] = ut[e][1] = 0.0;

  // c[n] = (v[2n], v[2n+1]) of the zero-padded v = x-hat (A) or x-hat - u (S)
  auto pack = [&]() {
#pragma unroll
    for (int e = 0; e < SP_TPL; ++e) {
      const int n = tid + e * NT;
      if (n >= N) continue;
      cplx c = zero;
      if (2 * n < w) {
        c = {xr[2 * n], xr[2 * n + 1]};
        if (ALG == AINP_SPAIN_S) {
          c.re -= ut[e][0];
          c.im -= ut[e][1];
        }
      }
      f.st(n, c);
    }
    __syncthreads();
  };

  if (ALG == AINP_SPAIN_A) {
    pack();
    sp_dif<NT>(f, tid);
    sp_split<NT, EPL>(f, tid, fwd, Z);
    __syncthreads();
  }

  bool keep[SP_NK];
  double best = INFINITY;
  int k = s_step, cnt = 1, done = 0;
  while (cnt <= maxit) {
    double acc = 0.0;
    if (ALG == AINP_SPAIN_A) {
      // z-bar = H_k(z + u);  obj = |z - z-bar| over all M coefficients
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        ZB.a[e] = cadd(Z.a[e], U.a[e]);
        ZB.b[e] = cadd(Z.b[e], U.b[e]);
      }
      sp_hard_threshold<NT, EPL>(ZB, N, k, hist, sel, tid, keep);
      sp_apply(ZB, keep, tid);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int p = tid + e * NT;
        if (p >= N / 2) continue;
        const cplx da = csub(Z.a[e], ZB.a[e]), db = csub(Z.b[e], ZB.b[e]);
        // DC and Nyquist count once, every other bin with its mirror
        acc += p == 0 ? cabs2(da) + 2.0 * cabs2(db) : 2.0 * (cabs2(da) + cabs2(db));
      }
    } else {
      // z-bar = H_k(A (x-hat - u));  obj = |A* z-bar - x-hat|
      pack();
      sp_dif<NT>(f, tid);
      sp_split<NT, EPL>(f, tid, fwd, ZB);
      sp_hard_threshold<NT, EPL>(ZB, N, k, hist, sel, tid, keep);   // barriers: the split's reads are done
      sp_apply(ZB, keep, tid);
      sp_merge<NT, EPL>(f, tid, ZB);
      __syncthreads();
      sp_dit<NT>(f, tid);
#pragma unroll
      for (int e = 0; e < SP_TPL; ++e) {
        const int n = tid + e * NT;
        if (n >= N || 2 * n >= w) continue;
        const cplx c = f.ld(n);
        const double d0 = c.re * inv - xr[2 * n], d1 = c.im * inv - xr[2 * n + 1];
        acc += d0 * d0 + d1 * d1;
      }
    }
    const double obj = sqrt(sp_sum<NT>(acc, part, tid));
    done = cnt;
    if (hrow && tid == 0) hrow[cnt - 1] = obj;
    if (obj <= best) {   // record the iterate the objective was evaluated on
      best = obj;
      for (int i = tid; i < gl; i += NT) x[gs + i] = xr[gs + i];
    }
    if (obj <= epsilon) break;
    __syncthreads();   // the record has read the row

    if (ALG == AINP_SPAIN_A) {
      // x-hat = proj(Re A* (z-bar - u));  z = A x-hat;  u += z - z-bar
      SpSpec<EPL> B;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        B.a[e] = csub(ZB.a[e], U.a[e]);
        B.b[e] = csub(ZB.b[e], U.b[e]);
      }
      sp_merge<NT, EPL>(f, tid, B);
      __syncthreads();
      sp_dit<NT>(f, tid);
      // a lane projects and re-packs its own sample pairs in place
#pragma unroll
      for (int e = 0; e < SP_TPL; ++e) {
        const int n = tid + e * NT;
        if (n >= N) continue;
        cplx c = zero;
        if (2 * n < w) {
          const cplx y = f.ld(n);
          const int t0 = 2 * n, t1 = 2 * n + 1;
          if (t0 >= gs && t0 - gs < gl) xr[t0] = y.re * inv;
          if (t1 >= gs && t1 - gs < gl) xr[t1] = y.im * inv;
          c = {xr[t0], xr[t1]};
        }
        f.st(n, c);
      }
      __syncthreads();
      sp_dif<NT>(f, tid);
      sp_split<NT, EPL>(f, tid, fwd, Z);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        U.a[e] = csub(cadd(U.a[e], Z.a[e]), ZB.a[e]);
        U.b[e] = csub(cadd(U.b[e], Z.b[e]), ZB.b[e]);
      }
      __syncthreads();   // the split's reads are done before the next merge
    } else {
      // x-hat = proj(x_e + u);  u += x_e - x-hat, a lane on its own sample pairs
#pragma unroll
      for (int e = 0; e < SP_TPL; ++e) {
        const int n = tid + e * NT;
        if (n >= N || 2 * n >= w) continue;
        const cplx c = f.ld(n);
        const double xe[2] = {c.re * inv, c.im * inv};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int t = 2 * n + h;
          if (t >= gs && t - gs < gl) xr[t] = xe[h] + ut[e][h];
          ut[e][h] += xe[h] - xr[t];
        }
      }
      __syncthreads();
    }
    ++cnt;
    if (cnt % r_rate == 0) k += s_step;
  }
  if (tid == 0) iters[row] = done;
  if (hrow)
    for (int i = done + tid; i < maxit; i += NT) hrow[i] = NAN;
}

template <int NT, int ALG, int EPL>
static int sp_launch(const SpLds& l, double* sol, int64_t n_rows, int64_t stride,
                     const int32_t* gap_start, const int32_t* gap_len, int w, int M, int lgN, int s,
                     int r, double epsilon, int maxit, int32_t* iters, double* obj_history,
                     void* stream) {
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)spain_kernel<NT, ALG, EPL>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)sp_lds(SP_WMAX, SP_MMAX).bytes()) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_spain: cannot reserve the transform's LDS");
  hipLaunchKernelGGL((spain_kernel<NT, ALG, EPL>), dim3((unsigned)n_rows), dim3(NT), l.bytes(),
                     as_stream(stream), sol, stride, gap_start, gap_len, w, M, lgN, s, r, epsilon,
                     maxit, iters, obj_history, l.nF, l.nRow);
  return check_launch("ainp_spain");
}

static bool sp_shape_ok(int w, int red) {
  return w >= SP_WMIN && w <= SP_WMAX && (w & (w - 1)) == 0 && (red == 1 || red == 2 || red == 4) &&
         (int64_t)red * w <= SP_MMAX;
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_spain_workspace(int64_t n_rows, int w, int red, int algorithm) {
  // the transform, the iterate and the twiddles fit LDS over the whole
  // supported range and the spectra stay in registers: no global scratch
  (void)n_rows;
  (void)w;
  (void)red;
  (void)algorithm;
  return 0;
}

extern "C" int ainp_spain(double* sol, int64_t n_rows, int64_t stride, const int32_t* gap_start,
                          const int32_t* gap_len, int w, int red, int algorithm, int s, int r,
                          double epsilon, int maxit, int32_t* iters, double* obj_history,
                          void* workspace, size_t ws_bytes, void* stream) {
  if (!sol || !gap_start || !gap_len || !iters || n_rows < 0)
    return record_msg("ainp_spain: bad argument");
  if (algorithm != AINP_SPAIN_A && algorithm != AINP_SPAIN_S)
    return record_msg("ainp_spain: bad argument (algorithm is AINP_SPAIN_A or AINP_SPAIN_S)");
  if (!sp_shape_ok(w, red))
    return record_msg("ainp_spain: bad argument (w a power of two, 8 <= w <= 4096, red 1, 2 or 4, "
                      "red * w <= 8192)");
  if (stride < w) return record_msg("ainp_spain: bad argument (stride >= w)");
  const int M = red * w;
  if (s < 1 || r < 1) return record_msg("ainp_spain: bad argument (s >= 1, r >= 1)");
  if (maxit < 1 || maxit > M / 2 + 1)
    return record_msg("ainp_spain: bad argument (1 <= maxit <= red * w / 2 + 1)");
  if (!(epsilon >= 0.0)) return record_msg("ainp_spain: bad argument (epsilon >= 0)");
  if (ws_bytes < ainp_spain_workspace(n_rows, w, red, algorithm) || (ws_bytes && !workspace))
    return record_msg("ainp_spain: workspace too small");
  if (n_rows > 0x7fffffff) return record_msg("ainp_spain: too many rows");
  if (n_rows == 0) return AINP_OK;
  int lgN = 0;
  while ((2 << lgN) < M) ++lgN;   // N = M / 2 = 1 << lgN
  const SpLds l = sp_lds(w, M);
#define SP_GO(NT, ALG, EPL)                                                                  \
  return sp_launch<NT, ALG, EPL>(l, sol, n_rows, stride, gap_start, gap_len, w, M, lgN, s, r,   \
                                 epsilon, maxit, iters, obj_history, stream)
  if (M / 2 <= SP_NMAX_256) {
    if (algorithm == AINP_SPAIN_A) SP_GO(256, AINP_SPAIN_A, 2);
    SP_GO(256, AINP_SPAIN_S, 2);
  }
  if (algorithm == AINP_SPAIN_A) SP_GO(SP_NT_BIG, AINP_SPAIN_A, SP_EPL_BIG);
  SP_GO(SP_NT_BIG, AINP_SPAIN_S, SP_EPL_BIG);
#undef SP_GO
}
