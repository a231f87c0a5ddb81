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
// share nothing.  What lives where (spain_fft.h: the transforms, the slots, the
// quarter wave, the sum and the select with its tie rule; spain_window.h: the
// steps of the window loop that spain_omp.hip shares; spain_plan.h: the limits,
// the LDS plan and the lane route, on the host):
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
//   static   histogram 1024 + wave sums and the select's result < 256; 40 of padding
// 117 KiB of the 160 KiB: one workgroup per CU there.  N <= 1024 runs 256 lanes
// with 2 slots a lane, longer transforms 512 lanes with up to 4: at 1024 lanes
// and 2 slots the 128 registers a lane has left spill (196 bytes of scratch a
// lane in A-SPAIN), and A-SPAIN measured 6 % (one row) to 16 % (256 rows) slower
// than at 512 lanes, S-SPAIN 5 % faster.
#include <cmath>

#include "spain_window.h"

namespace ainp {

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
  const int count = N + 1;   // the half spectrum's bins, all members
  sp_keep_largest<NT, SP_NK>(key, member, bin, k, count, hist, sel, tid, keep);
  // sp_keep_largest's k >= count path has no barrier; S-SPAIN's caller needs one
  if (k >= count) __syncthreads();
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

template <int NT>
__device__ __forceinline__ bool sp_open(SpRow& R, double* ct, double* sol, int64_t stride,
                                        const int32_t* gap_start, const int32_t* gap_len, int w,
                                        int M, int maxit, int32_t* iters, double* obj_history,
                                        int tid) {
  const int64_t row = blockIdx.x;
  R.gs = gap_start[row];
  R.gl = gap_len[row];
  R.hrow = obj_history ? obj_history + row * maxit : nullptr;
  R.arow = nullptr;
  if (!sp_run_ok(R.gs, R.gl, w)) {
    sp_row_close<NT>(iters, R.hrow, R.arow, 0, maxit, tid);
    return false;
  }
  R.x = sol + row * stride;
  sp_row_load<NT>(R, ct, w, M, tid);
  return true;
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
  const int tid = threadIdx.x;
  const int N = M / 2;
  const int64_t row = blockIdx.x;
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nF;
  double* xr = im + nF;
  double* ct = xr + nRow;
  SpRow R;
  R.xr = xr;
  if (!sp_open<NT>(R, ct, sol, stride, gap_start, gap_len, w, M, maxit, iters, obj_history, tid))
    return;
  const int gs = R.gs, gl = R.gl;
  double* hrow = R.hrow;

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
      acc = sp_residual2<NT, SP_TPL>(f, R, w, inv, tid);
    }
    const double obj = sqrt(sp_sum<NT>(acc, part, tid));
    done = cnt;
    if (sp_record<NT>(R, obj, cnt, 0, best, epsilon, tid)) break;
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
      sp_project_dual<NT, SP_TPL>(f, R, w, inv, ut, tid);   // x-hat = proj(x_e + u); u += x_e - x-hat
    }
    sp_next_pass(cnt, k, s_step, r_rate);
  }
  sp_row_close<NT>(iters, hrow, nullptr, done, maxit, tid);
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_spain_workspace(int64_t, int, int, int) {
  // the transform, the iterate and the twiddles fit LDS over the whole
  // supported range and the spectra stay in registers: no global scratch
  return 0;
}

extern "C" int ainp_spain(double* sol, int64_t n_rows, int64_t stride, const int32_t* gap_start,
                          const int32_t* gap_len, int w, int red, int algorithm, int s, int r,
                          double epsilon, int maxit, int32_t* iters, double* obj_history,
                          void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = sp_check_window_args(
          "ainp_spain", sol && gap_start && gap_len && iters, n_rows, stride, w, red,
          algorithm == AINP_SPAIN_A || algorithm == AINP_SPAIN_S, s, r, epsilon, maxit))
    return rc;
  if (ws_bytes < ainp_spain_workspace(n_rows, w, red, algorithm) || (ws_bytes && !workspace))
    return record_msg("ainp_spain: workspace too small");
  if (n_rows > 0x7fffffff) return record_msg("ainp_spain: too many rows");
  if (n_rows == 0) return AINP_OK;
  const int M = red * w;
  const SpLds l = sp_window_lds(w, M, false);
#define SP_GO(NT, ALG, EPL)                                                                     \
  return sp_launch_rows<spain_kernel<NT, ALG, EPL>, NT>(                                        \
      "ainp_spain", sp_window_lds(SP_WMAX, SP_MMAX, false).bytes(), l.bytes(), n_rows, stream,  \
      sol, stride, gap_start, gap_len, w, M, sp_lgN(M), s, r, epsilon, maxit, iters,            \
      obj_history, l.nF, l.nRow)
  if (sp_lanes_256(M)) {
    if (algorithm == AINP_SPAIN_A) SP_GO(256, AINP_SPAIN_A, 2);
    SP_GO(256, AINP_SPAIN_S, 2);
  }
  if (algorithm == AINP_SPAIN_A) SP_GO(SP_NT_BIG, AINP_SPAIN_A, SP_EPL_BIG);
  SP_GO(SP_NT_BIG, AINP_SPAIN_S, SP_EPL_BIG);
#undef SP_GO
}
