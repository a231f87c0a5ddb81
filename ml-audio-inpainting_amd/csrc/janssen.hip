// janssen.hip — gap-wise Janssen autoregressive inpainting, the AR baseline of
// the reference's model comparison (models/AudioReg/utils/janssen_inp.m with
// method = "lpc" or "arburg", driven by models/AudioReg/train.m).  All
// arithmetic float64.
//
// One workgroup owns one segment for all maxit iterations; segments share
// nothing, so the batch is the parallelism.  Per iteration:
//   1. r[k] = sum_n sol[n] sol[n+k], k = 0..p   (lpc's biased autocorrelation;
//      the signal is staged through LDS in chunks, two adjacent lags per lane)
//   2. Levinson-Durbin on r -> a[0..p]
//      ("arburg": 1 and 2 are Burg's estimator on sol instead, ar_fit.h)
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
// The "lpc" kernel runs 256 lanes.  The "arburg" kernel runs 512, because
// Burg's two error vectors live in registers (32 elements of each per lane);
// its steps 3 to 6 are the same code over 8 waves instead of 4.
//
// LDS (doubles), H = the longest gap the stride allows (<= 2048):
// B[max(p, H) + 2] (r, then b; zero beyond p, so the recursions read t[i]
// unguarded) | A[max(p, H) + 2] | Y[H] (g) | W[S] (signal chunks, then the two
// contexts, then Z) | arburg only: XY[4 x 514], the neighbour exchange of
// burg_fit.  The signal itself stays in global memory (L2): 16384 doubles do
// not fit beside the vectors.
#include <algorithm>

#include "ar_fit.h"

namespace ainp {

struct JnLds {
  int nB, nA, nY, S, nX;   // doubles
  size_t bytes() const { return ((size_t)nB + nA + nY + S + nX) * sizeof(double); }
};

// n_max: the longest segment the stride allows.  W's S doubles hold, in turn,
// a signal chunk (S - p >= 1024 samples and the p that follow them, or the
// whole segment), the two contexts (<= 2p samples, never more than the
// segment) and Z (gap + 1).
static JnLds jn_lds(int64_t n_max, int p, int method) {
  JnLds l;
  const int hcap = (int)std::min<int64_t>(JN_HMAX, n_max);
  l.nB = (std::max(p, hcap) + 3) & ~1;
  l.nA = l.nB;
  l.nY = (hcap + 1) & ~1;
  const int64_t want = std::max<int64_t>(2 * (int64_t)p, (int64_t)p + 1024);
  l.S = (int)std::max<int64_t>(l.nY + 2, std::min<int64_t>(n_max, want));
  l.nX = method == AINP_AR_BURG ? BG_XY : 0;
  return l;
}

// grid: one workgroup of NT lanes per segment.  dynamic LDS: JnLds.
template <int NT, int METHOD>
__global__ __launch_bounds__(NT) void janssen_kernel(
    double* sol, int64_t n_segments, int64_t stride, const int32_t* __restrict__ n_,
    const int32_t* __restrict__ gap_start, const int32_t* __restrict__ gap_len, int p, int maxit,
    double* __restrict__ history, int32_t* __restrict__ iters_done, int nB, int nA, int nY,
    int S) {
  static_assert(METHOD == AINP_AR_LPC || NT == BG_THREADS, "burg_fit needs its 512 lanes");
  constexpr int NW = NT / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double part[2][2][NW];
  __shared__ int s_hmax[NW];
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
    for (int64_t i = tid; i < n_segments; i += NT)
      hrow = max(hrow, min(max(gap_len[i], 0), JN_HMAX));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hrow = max(hrow, __shfl_xor(hrow, o, 64));
    if (lane == 0) s_hmax[wave] = hrow;
    __syncthreads();
    hrow = s_hmax[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) hrow = max(hrow, s_hmax[w]);
  }

  const int N = n_[seg], s = gap_start[seg], h = gap_len[seg];
  // a segment the tables describe outside the supported range is left alone
  if (N <= p || N > JN_NMAX || (int64_t)N > stride || h < 1 || h > JN_HMAX || h > nY || s < 0 ||
      (int64_t)s + h > N) {
    if (tid == 0) iters_done[seg] = -1;
    return;
  }
  double* x = sol + seg * stride;
  for (int i = tid; i < h; i += NT) x[s + i] = 0.0;
  for (int k = p + 1 + tid; k < nB; k += NT) B[k] = 0.0;   // stays zero
  __syncthreads();

  // a chunk holds the products that start at C samples and the p samples after
  // them; a segment that fits W whole is one chunk
  const int C = N <= S ? N : S - p;
  int done = 0;
  for (int it = 0; it < maxit; ++it) {
    if (tid == 0) s_bad = 0;
    if constexpr (METHOD == AINP_AR_LPC) {
      // 1. autocorrelation of the current solution
      for (int k = tid; k <= p; k += NT) B[k] = 0.0;
      if (tid == 0) A[0] = 1.0;
      for (int c0 = 0; c0 < N; c0 += C) {
        const int L = min(S, N - c0);
        __syncthreads();   // the previous chunk (or Z) is no longer read
        for (int i = tid; i < L; i += NT) W[i] = x[c0 + i];
        __syncthreads();
        jn_lags<NT>(W, L, min(C, N - c0), p, B);
      }
      __syncthreads();
      const double r0 = B[0];
      if (!(r0 > 0.0) || !isfinite(r0)) break;   // silent (or unusable) context

      // 2. AR coefficients
      if (!jn_levinson<false, NT>(B, p, A, nullptr, nullptr, part)) break;
    } else {
      // 1 + 2. AR coefficients by Burg's estimator, the solution read into
      // registers; a silent context stops at its first denominator
      if (!burg_fit<1>(x, 0.0, N, p, A, W + S, part)) break;
    }
    __syncthreads();

    // 3. their autocorrelation, over r
    for (int k = tid; k <= p; k += NT) B[k] = 0.0;
    __syncthreads();
    jn_lags<NT>(A, p + 1, p + 1, p, B);

    // 4. right-hand side from the observed samples within p of the gap
    const int l0 = max(0, s - p), LL = s - l0;
    const int RL = min(N, s + h + p) - (s + h);
    double* WL = W;
    double* WR = W + LL;
    for (int i = tid; i < LL; i += NT) WL[i] = x[l0 + i];
    for (int i = tid; i < RL; i += NT) WR[i] = x[s + h + i];
    __syncthreads();
    for (int ii = tid; ii < h; ii += NT) {
      // left: d = ii + 1 + t, j = s - 1 - t; right: d = h - ii + t, j = s + h + t
      const int cl = min(p - ii, LL), cr = min(p - (h - ii) + 1, RL);
      double acc = 0.0;
      if (cl > 0) acc = jn_dot<-1>(B + ii + 1, WL + LL - 1, cl);
      if (cr > 0) acc += jn_dot<1>(B + (h - ii), WR, cr);
      Y[ii] = -acc;
    }
    __syncthreads();

    // 5. the gap samples
    const bool ok = jn_levinson<true, NT>(B, h, A, W, Y, part);
    __syncthreads();
    if (!ok) break;
    for (int j = 1 + tid; j <= h; j += NT)
      if (!isfinite(W[j])) s_bad = 1;
    __syncthreads();
    if (s_bad) break;

    // 6. accept the iterate
    double* hist = history ? history + ((seg * maxit + it) * (int64_t)hrow) : nullptr;
    for (int j = 1 + tid; j <= h; j += NT) {
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

template <int NT, int METHOD>
static int jn_launch(const JnLds& l, double* sol, int64_t n_segments, int64_t stride,
                     const int32_t* n, const int32_t* gap_start, const int32_t* gap_len, int p,
                     int maxit, double* history, int32_t* iters_done, void* stream) {
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)janssen_kernel<NT, METHOD>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)jn_lds(JN_NMAX, JN_PMAX, METHOD).bytes()) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_janssen_ex: cannot reserve the recursion vectors' LDS");
  hipLaunchKernelGGL((janssen_kernel<NT, METHOD>), dim3((unsigned)n_segments), dim3(NT),
                     l.bytes(), as_stream(stream), sol, n_segments, stride, n, gap_start, gap_len,
                     p, maxit, history, iters_done, l.nB, l.nA, l.nY, l.S);
  return check_launch("ainp_janssen_ex");
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_janssen_workspace(int64_t n_segments, int n_max, int p, int gap_max) {
  return ainp_janssen_ex_workspace(n_segments, n_max, p, gap_max, AINP_AR_LPC);
}

extern "C" size_t ainp_janssen_ex_workspace(int64_t n_segments, int n_max, int p, int gap_max,
                                            int method) {
  // every recursion vector fits LDS over the whole supported range, Burg's
  // error vectors stay in registers and the signal is read in place, so no
  // shape needs global scratch with either estimator
  (void)n_segments;
  (void)n_max;
  (void)p;
  (void)gap_max;
  (void)method;
  return 0;
}

extern "C" int ainp_janssen(double* sol, int64_t n_segments, int64_t stride, const int32_t* n,
                            const int32_t* gap_start, const int32_t* gap_len, int p, int maxit,
                            double* history, int32_t* iters_done, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return ainp_janssen_ex(sol, n_segments, stride, n, gap_start, gap_len, p, maxit, history,
                         iters_done, workspace, workspace_bytes, AINP_AR_LPC, stream);
}

extern "C" int ainp_janssen_ex(double* sol, int64_t n_segments, int64_t stride, const int32_t* n,
                               const int32_t* gap_start, const int32_t* gap_len, int p, int maxit,
                               double* history, int32_t* iters_done, void* workspace,
                               size_t workspace_bytes, int method, void* stream) {
  if (!sol || !n || !gap_start || !gap_len || !iters_done || n_segments < 0 || stride < 1)
    return record_msg("ainp_janssen_ex: bad argument");
  if (method != AINP_AR_LPC && method != AINP_AR_BURG)
    return record_msg("ainp_janssen_ex: bad argument (method is AINP_AR_LPC or AINP_AR_BURG)");
  if (p < 1 || maxit < 1) return record_msg("ainp_janssen_ex: bad argument (p >= 1, maxit >= 1)");
  if (p > JN_PMAX || maxit > JN_ITMAX)
    return jn_unsupported("ainp_janssen_ex: unsupported (p <= 3072, maxit <= 1000)");
  if (stride <= p) return record_msg("ainp_janssen_ex: bad argument (p < n <= stride)");
  const int64_t n_max = std::min<int64_t>(stride, JN_NMAX);
  if (workspace_bytes < ainp_janssen_ex_workspace(n_segments, (int)n_max, p, JN_HMAX, method) ||
      (workspace_bytes && !workspace))
    return record_msg("ainp_janssen_ex: workspace too small");
  if (n_segments > 0x7fffffff)
    return jn_unsupported("ainp_janssen_ex: too many segments");
  if (n_segments == 0) return AINP_OK;
  const JnLds l = jn_lds(n_max, p, method);
  if (method == AINP_AR_BURG)
    return jn_launch<BG_THREADS, AINP_AR_BURG>(l, sol, n_segments, stride, n, gap_start, gap_len,
                                               p, maxit, history, iters_done, stream);
  return jn_launch<JN_THREADS, AINP_AR_LPC>(l, sol, n_segments, stride, n, gap_start, gap_len, p,
                                            maxit, history, iters_done, stream);
}
