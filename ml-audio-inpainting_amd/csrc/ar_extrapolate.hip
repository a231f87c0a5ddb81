// ar_extrapolate.hip — forward/backward autoregressive extrapolation of a gap,
// the `extrapolation` row of the reference's AR comparison
// (models/AudioReg/utils/arinpaint.m as models/AudioReg/train.m drives it, with
// method = "lpc" or "arburg").  All arithmetic float64.
//
// One workgroup of 512 lanes owns one side of one segment -- the context before
// the gap, or the time-reversed context after it (grid: segments x 2):
//   1. mean of the context (at most w samples), removed from it on the fly
//   2. AR coefficients a[0..p] of the mean-removed context: "lpc" (the lag sums
//      and the Levinson recursion of janssen.hip, context staged through LDS in
//      chunks) or "arburg" (burg_fit, context read into registers)
//   3. y[t] = -sum_{k=1..p} a[k] y[t-k], t = 0..h-1, with the last p context
//      samples as the past (filtic + filter(1, a, zeros(h, 1))): lane k - 1
//      keeps a[k], a[k + 512], ... (six at most) in registers and reads its y
//      from the LDS window; a step is lane terms -> wave reduce -> one LDS slot
//      per wave -> one barrier -> every lane adds the slots in wave order
//   4. the mean is added back and the side's h samples go to the workspace
// A second launch blends them: gap = wts * prediction + (1 - wts) *
// reverse(postdiction) with wts = cos^2(linspace(0, pi/2, h)); for h = 1
// MATLAB's linspace gives pi/2, so the gap sample is the postdiction.  A side
// whose context is constant (zero after the mean is removed) or whose fit
// stops predicts its mean; the segment is then filled and reported with status
// 0.  No atomics, every sum in a fixed order: the same bits on every call.
// (Both sides in one workgroup, in turn, would halve the parallelism of a
// small batch, and the values such a kernel keeps live across burg_fit's 128
// vector registers spilled.)
//
// LDS (doubles): B[p + 2] (r; zero beyond p) | A[p + 2] | W[S] (context chunks,
// then the window of step 3: p past samples and h predictions) | XY[4 x 514]
// (burg_fit's neighbour exchange).
// Workspace: double side[n_segments][2][hp] (hp = the longest gap the stride
// allows), then int32 ok[n_segments][2].
#include <algorithm>

#include "ar_fit.h"

namespace ainp {

struct ArLds {
  int nA, S;   // doubles
  size_t bytes() const { return ((size_t)2 * nA + S + BG_XY) * sizeof(double); }
};

// n_max: the longest segment the stride allows.  W holds a context chunk
// (S - p >= 2048 samples and the p that follow them, or the whole context) and
// later p + h <= p + 2048 samples, never more than the segment.
static ArLds ar_lds(int64_t n_max, int p) {
  ArLds l;
  l.nA = (p + 3) & ~1;
  l.S = (int)std::min<int64_t>((n_max + 1) & ~(int64_t)1,
                               (int64_t)p + std::max(p, JN_HMAX));
  return l;
}

// the context lengths of a segment; false when its table entries are outside
// the supported range (both kernels leave such a segment alone)
__device__ __forceinline__ bool ar_contexts(int N, int s, int h, int64_t stride, int p, int w,
                                            int hp, int (&len)[2]) {
  if (N < 1 || N > JN_NMAX || (int64_t)N > stride || h < 1 || h > hp || s < 0 ||
      (int64_t)s + h > N)
    return false;
  len[0] = min(s, w);
  len[1] = (int)min((int64_t)N, (int64_t)s + h + w) - (s + h);
  return len[0] > p && len[1] > p;
}

// grid: (segments, 2 sides), one workgroup each.  dynamic LDS: ArLds.
__global__ __launch_bounds__(BG_THREADS) void ar_predict_kernel(
    const double* __restrict__ sol, int64_t stride, const int32_t* __restrict__ n_,
    const int32_t* __restrict__ gap_start, const int32_t* __restrict__ gap_len, int p, int w,
    int method, double* __restrict__ pred, int32_t* __restrict__ side_ok, int hp, int nA, int S) {
  constexpr int NT = BG_THREADS;
  constexpr int KPL = JN_PMAX / NT;   // coefficients a lane keeps for step 3
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double part[2][2][BG_WAVES];
  double* B = reinterpret_cast<double*>(smem);
  double* A = B + nA;
  double* W = A + nA;
  double* XY = W + S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t seg = blockIdx.x;
  const int side = blockIdx.y;

  const int N = n_[seg], s = gap_start[seg], h = gap_len[seg];
  int len[2] = {0, 0};
  if (!ar_contexts(N, s, h, stride, p, w, hp, len)) return;
  const double* __restrict__ x = sol + seg * stride;
  double* __restrict__ out = pred + (seg * 2 + side) * (int64_t)hp;
  for (int k = p + 1 + tid; k < nA; k += NT) B[k] = 0.0;   // stays zero

  // the context in prediction order: c(i) = x[o + d i], i < Lc
  const int Lc = len[side];
  const int o = side == 0 ? s - Lc : s + h + Lc - 1, d = side == 0 ? 1 : -1;
  const double* __restrict__ xc = x + o;

  // 1. the mean, then the energy of what is left
  double acc = 0.0;
  for (int i = tid; i < Lc; i += NT) acc += xc[d * i];
  const double mean = jn_block_sum<NT>(acc, part[0][0]) / (double)Lc;
  acc = 0.0;
  for (int i = tid; i < Lc; i += NT) {
    const double v = xc[d * i] - mean;
    acc = fma(v, v, acc);
  }
  const double energy = jn_block_sum<NT>(acc, part[0][0]);
  bool ok = energy > 0.0 && isfinite(energy);

  // 2. AR coefficients of the mean-removed context
  if (ok && method == AINP_AR_LPC) {
    for (int k = tid; k <= p; k += NT) B[k] = 0.0;
    if (tid == 0) A[0] = 1.0;
    const int C = Lc <= S ? Lc : S - p;
    for (int c0 = 0; c0 < Lc; c0 += C) {
      const int L = min(S, Lc - c0);
      __syncthreads();   // the previous chunk is no longer read
      for (int i = tid; i < L; i += NT) W[i] = xc[d * (c0 + i)] - mean;
      __syncthreads();
      jn_lags<NT>(W, L, min(C, Lc - c0), p, B);
    }
    __syncthreads();
    const double r0 = B[0];
    ok = r0 > 0.0 && isfinite(r0);
    if (ok) ok = jn_levinson<false, NT>(B, p, A, nullptr, nullptr, part);
  } else if (ok) {
    ok = side == 0 ? burg_fit<1>(xc, mean, Lc, p, A, XY, part)
                   : burg_fit<-1>(xc, mean, Lc, p, A, XY, part);
  }
  __syncthreads();

  // 3. h prediction steps; W[0..p) is the past, W[p + t] = y[t]
  if (ok) {
    for (int i = tid; i < p; i += NT) W[i] = xc[d * (Lc - p + i)] - mean;
    double a[KPL];   // a[k], k = 1 + tid + q NT
#pragma unroll
    for (int q = 0; q < KPL; ++q) a[q] = 1 + tid + q * NT <= p ? A[1 + tid + q * NT] : 0.0;
    double last = 0.0;   // y[t - 1], every lane has it
    __syncthreads();
    for (int t = 0; t < h; ++t) {
      double v = 0.0;
      if (tid < p) v = a[0] * (tid == 0 && t > 0 ? last : W[p + t - 1 - tid]);
#pragma unroll
      for (int q = 1; q < KPL; ++q)
        if (tid + q * NT < p) v = fma(a[q], W[p + t - 1 - tid - q * NT], v);
      v = jn_wave_sum(v);
      if (lane == 0) part[t & 1][0][wave] = v;
      __syncthreads();
      last = -jn_slot_sum<BG_WAVES>(part[t & 1][0]);
      if (tid == 0) W[p + t] = last;
    }
    __syncthreads();
  }

  // 4. the side's samples, in its own prediction order
  for (int i = tid; i < h; i += NT) out[i] = (ok ? W[p + i] : 0.0) + mean;
  if (tid == 0) side_ok[seg * 2 + side] = ok ? 1 : 0;
}

// grid: one workgroup of 256 per segment
__global__ __launch_bounds__(256) void ar_crossfade_kernel(
    double* __restrict__ sol, int64_t stride, const int32_t* __restrict__ n_,
    const int32_t* __restrict__ gap_start, const int32_t* __restrict__ gap_len, int p, int w,
    const double* __restrict__ pred, const int32_t* __restrict__ side_ok, int hp,
    int32_t* __restrict__ status) {
  const int64_t seg = blockIdx.x;
  const int N = n_[seg], s = gap_start[seg], h = gap_len[seg];
  int len[2] = {0, 0};
  if (!ar_contexts(N, s, h, stride, p, w, hp, len)) {
    if (threadIdx.x == 0) status[seg] = -1;
    return;
  }
  double* __restrict__ gap = sol + seg * stride + s;
  const double* __restrict__ fwd = pred + seg * 2 * (int64_t)hp;
  const double* __restrict__ bwd = fwd + hp;
  const double half_pi = 1.5707963267948966;
  const double step = h > 1 ? half_pi / (h - 1) : 0.0;
  for (int i = threadIdx.x; i < h; i += 256) {
    const double c = cos(h == 1 || i == h - 1 ? half_pi : i * step);
    const double wt = c * c;
    gap[i] = wt * fwd[i] + (1.0 - wt) * bwd[h - 1 - i];
  }
  if (threadIdx.x == 0) status[seg] = side_ok[seg * 2] && side_ok[seg * 2 + 1] ? 1 : 0;
}

static int ar_unsupported(const char* msg) {
  record_msg(msg);
  return AINP_EUNSUPPORTED;
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_ar_extrapolate_workspace(int64_t n_segments, int n_max, int p, int gap_max,
                                                int method) {
  // the two sides of a segment meet in global memory: 2 x hp doubles and two
  // flags per segment, hp = the longest gap the shape allows
  (void)p;
  (void)method;
  if (n_segments <= 0) return 0;
  const int64_t hp = std::max<int64_t>(1, std::min<int64_t>({(int64_t)gap_max, (int64_t)n_max,
                                                             (int64_t)JN_HMAX}));
  return (size_t)n_segments * 2 * ((size_t)hp * sizeof(double) + sizeof(int32_t));
}

extern "C" int ainp_ar_extrapolate(double* sol, int64_t n_segments, int64_t stride,
                                   const int32_t* n, const int32_t* gap_start,
                                   const int32_t* gap_len, int p, int w, int method,
                                   int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (!sol || !n || !gap_start || !gap_len || !status || n_segments < 0 || stride < 1)
    return record_msg("ainp_ar_extrapolate: bad argument");
  if (method != AINP_AR_LPC && method != AINP_AR_BURG)
    return record_msg("ainp_ar_extrapolate: bad argument (method is AINP_AR_LPC or AINP_AR_BURG)");
  if (p < 1 || w < 1) return record_msg("ainp_ar_extrapolate: bad argument (p >= 1, w >= 1)");
  if (p > JN_PMAX) return ar_unsupported("ainp_ar_extrapolate: unsupported (p <= 3072)");
  if (stride <= p) return record_msg("ainp_ar_extrapolate: bad argument (p < n <= stride)");
  if (n_segments > 0x7fffffff) return ar_unsupported("ainp_ar_extrapolate: too many segments");
  const int64_t n_max = std::min<int64_t>(stride, JN_NMAX);
  const int hp = (int)std::min<int64_t>(JN_HMAX, n_max);
  if (workspace_bytes <
          ainp_ar_extrapolate_workspace(n_segments, (int)n_max, p, JN_HMAX, method) ||
      (workspace_bytes && !workspace))
    return record_msg("ainp_ar_extrapolate: workspace too small");
  if (n_segments == 0) return AINP_OK;
  double* pred = static_cast<double*>(workspace);
  int32_t* side_ok = reinterpret_cast<int32_t*>(pred + n_segments * 2 * (int64_t)hp);
  const ArLds l = ar_lds(n_max, p);
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)ar_predict_kernel,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)ar_lds(JN_NMAX, JN_PMAX).bytes()) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_ar_extrapolate: cannot reserve the recursion vectors' LDS");
  hipLaunchKernelGGL(ar_predict_kernel, dim3((unsigned)n_segments, 2), dim3(BG_THREADS),
                     l.bytes(), as_stream(stream), sol, stride, n, gap_start, gap_len, p, w, method,
                     pred, side_ok, hp, l.nA, l.S);
  int rc = check_launch("ainp_ar_extrapolate");
  if (rc != AINP_OK) return rc;
  hipLaunchKernelGGL(ar_crossfade_kernel, dim3((unsigned)n_segments), dim3(256), 0,
                     as_stream(stream), sol, stride, n, gap_start, gap_len, p, w, pred, side_ok, hp,
                     status);
  return check_launch("ainp_ar_extrapolate");
}
