// mel.hip — the mel layer between the STFT and Griffin-Lim kernels:
// utils.extract_mel_spectrogram (utils.py:236-277 -> librosa.feature.
// melspectrogram) and utils.mel_spectrogram_to_audio (utils.py:335-393).
//
// ainp_mel_fwd: out[m][t] = sum_f w[m][f] * |X[f][t]|^power.  The Slaney
// filterbank is banded (row m is non-zero on one run of bins, a bin feeds at
// most two rows), so the host hands it over compressed: band_lo[m] = first bin
// of row m, band_off[m] .. band_off[m+1] = its run in the packed weights.
// A workgroup owns 64 columns of the flat [signal][frame] axis (the lane axis:
// loads and stores run along T) and a group of consecutive bands.  It walks
// the bins that group covers in chunks: each spectrum element is loaded once,
// its power computed once and staged in LDS, and the (at most two) bands a bin
// feeds read it from there.  The power spectrogram never reaches memory.  A
// band's weights within a chunk sit one per lane and are broadcast by
// v_readlane, the next chunk's loads fly meanwhile.  A band that straddles a
// chunk boundary keeps its running sum in an LDS accumulator owned by one
// (wave, lane), so every output is one fma chain over ascending bins -- no
// atomics, the same bits on every call.  With all bands in one group every
// element is fetched exactly once; when the frame tiles alone would leave most
// CUs idle the host splits the bands into groups, and two neighbouring groups
// both read the one mel step of bins between them.
//
// ainp_mel_inverse: L[f][t] = sum_k P[f][k] * M[k][t] (P = pinv of the
// filterbank, K = n_mels), exact f32 on v_mfma_f32_32x32x2_f32 -- a k-ordered
// fmaf chain, the arithmetic of gemm.hip's exact path -- with the reference's
// sqrt (and this port's clamp) applied to the accumulators before the only
// store.  The signals' frames are one flat column axis, so a short T does not
// waste lanes.  K is small: per 128 k a workgroup stages its 64 columns of M
// in LDS (loads along T) and each wave holds its 32 rows of P in registers.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace ainp {

// ------------------------------------------------------------------ forward
constexpr int MEL_TT = 64;       // frames per workgroup (one per lane)
constexpr int MEL_THREADS = 256;
constexpr int MEL_WAVES = MEL_THREADS / 64;

template <typename R>
struct alignas(2 * sizeof(R)) Cplx {   // one 8- / 16-byte load per element
  R re, im;
};

enum { MEL_POW_GENERAL = 0, MEL_POW_ONE = 1, MEL_POW_TWO = 2 };

template <typename R, int PM>
__device__ __forceinline__ R mel_power(R re, R im, R half_power) {
  const R s = fma(re, re, im * im);
  if (PM == MEL_POW_TWO) return s;
  if (PM == MEL_POW_ONE) return sqrt(s);
  return pow(s, half_power);
}

// run [lo, hi) of band m and the offset of its first weight; a band the
// tables describe inconsistently is treated as empty (never read)
__device__ __forceinline__ void mel_band(const int32_t* __restrict__ band_lo,
                                         const int32_t* __restrict__ band_off, int m, int F,
                                         int64_t n_weights, int& lo, int& hi, int64_t& off) {
  lo = band_lo[m];
  off = band_off[m];
  const int64_t len = (int64_t)band_off[m + 1] - off;
  if (lo < 0 || len <= 0 || off < 0 || off + len > n_weights || (int64_t)lo + len > F) {
    lo = 0;
    hi = 0;
  } else {
    hi = lo + (int)len;
  }
}

__device__ __forceinline__ float mel_readlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// grid: x = 64 columns of the flat [signal][frame] axis (a short T wastes no
// lanes), y = band group of G bands.  dynamic LDS: R powers[BT][64],
// R acc[G][64], int band[3][G] (first bin, end bin, offset of the first weight),
// float w[wcap] (WLDS: the packed weights fit in LDS, wcap >= n_weights, and a
// group's span is staged there; otherwise they are read from global memory)
template <typename R, int BT, int PM, bool WLDS>
__global__ __launch_bounds__(MEL_THREADS) void mel_fwd_kernel(
    const Cplx<R>* __restrict__ spec, int64_t ncols, int F, int64_t T,
    const int32_t* __restrict__ band_lo, const int32_t* __restrict__ band_off,
    const float* __restrict__ weights, int64_t n_weights, int n_mels, int G, int wcap,
    R half_power, R* __restrict__ out) {
  constexpr int NR = BT / MEL_WAVES;   // chunk rows per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int s_lo[MEL_WAVES], s_hi[MEL_WAVES], s_w0[MEL_WAVES], s_w1[MEL_WAVES];
  R* Ps = reinterpret_cast<R*>(smem);
  R* Acc = Ps + BT * MEL_TT;
  int* binfo = reinterpret_cast<int*>(Acc + G * MEL_TT);
  float* Wl = reinterpret_cast<float*>(binfo + 3 * G);   // [wcap] the group's weights
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t col = (int64_t)blockIdx.x * MEL_TT + lane;
  const bool cok = col < ncols;
  const int64_t sig = cok ? col / T : 0;
  const int64_t t = cok ? col - sig * T : 0;
  const int m0 = blockIdx.y * G;
  const int nb = min(n_mels, m0 + G) - m0;

  // the group's band table, and the bins it covers
  int mn = F, mx = 0, wmn = 0x7fffffff, wmx = 0;
  for (int i = threadIdx.x; i < nb; i += MEL_THREADS) {
    int lo, hi;
    int64_t off;
    mel_band(band_lo, band_off, m0 + i, F, n_weights, lo, hi, off);
    binfo[i] = lo;
    binfo[G + i] = hi;
    binfo[2 * G + i] = (int)off;
    if (hi > lo) {
      mn = min(mn, lo);
      mx = max(mx, hi);
      wmn = min(wmn, (int)off);
      wmx = max(wmx, (int)off + (hi - lo));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, 64));
    mx = max(mx, __shfl_xor(mx, o, 64));
    wmn = min(wmn, __shfl_xor(wmn, o, 64));
    wmx = max(wmx, __shfl_xor(wmx, o, 64));
  }
  if (lane == 0) {
    s_lo[wave] = mn;
    s_hi[wave] = mx;
    s_w0[wave] = wmn;
    s_w1[wave] = wmx;
  }
  for (int i = threadIdx.x; i < nb * MEL_TT; i += MEL_THREADS) Acc[i] = (R)0;
  __syncthreads();
  int gb0 = s_lo[0], gb1 = s_hi[0], w0 = s_w0[0], w1 = s_w1[0];
#pragma unroll
  for (int w = 1; w < MEL_WAVES; ++w) {
    gb0 = min(gb0, s_lo[w]);
    gb1 = max(gb1, s_hi[w]);
    w0 = min(w0, s_w0[w]);
    w1 = max(w1, s_w1[w]);
  }
  // the group's weights [w0, w1) into LDS (visible after the first chunk's barrier)
  if (WLDS)
    for (int i = threadIdx.x; i < min(w1 - w0, wcap); i += MEL_THREADS) Wl[i] = weights[w0 + i];

  // rows wave, wave + 4, ... of the chunk at c0 (zeros past the group's bins)
  const Cplx<R>* xs = spec + (sig * F) * T + t;
  Cplx<R> x[NR];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int f = c0 + wave + MEL_WAVES * i;
      x[i] = (cok && f < gb1) ? xs[(int64_t)f * T] : Cplx<R>{(R)0, (R)0};
    }
  };
  fetch(gb0);
  for (int c0 = gb0; c0 < gb1; c0 += BT) {
    // stage |X|^power of bins [c0, c0 + BT) x 64 columns; the next chunk's
    // loads fly while this one is consumed
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int f = c0 + wave + MEL_WAVES * i;
      Ps[(wave + MEL_WAVES * i) * MEL_TT + lane] =
          f < gb1 ? mel_power<R, PM>(x[i].re, x[i].im, half_power) : (R)0;
    }
    __syncthreads();
    fetch(c0 + BT);
    // every band of this wave that meets the chunk continues its fma chain;
    // its <= BT weights come in by one vector load and are read lane by lane
    for (int i = wave; i < nb; i += MEL_WAVES) {
      const int lo = __builtin_amdgcn_readfirstlane(binfo[i]);
      const int hi = __builtin_amdgcn_readfirstlane(binfo[G + i]);
      const int a = max(lo, c0), n = min(hi, c0 + BT) - a;
      if (n <= 0) continue;
      const int off = __builtin_amdgcn_readfirstlane(binfo[2 * G + i]);
      const int wi = off + (a - lo) + lane;
      const float wv = lane >= n ? 0.f : WLDS ? Wl[wi - w0] : weights[wi];
      const R* __restrict__ p = Ps + (a - c0) * MEL_TT + lane;
      R s = Acc[i * MEL_TT + lane];
      int k = 0;
      for (; k + 8 <= n; k += 8) {      // 8 LDS reads in flight, the chain in order
        R v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[(k + e) * MEL_TT];
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fma((R)mel_readlane(wv, k + e), v[e], s);
      }
      for (; k < n; ++k) s = fma((R)mel_readlane(wv, k), p[k * MEL_TT], s);
      Acc[i * MEL_TT + lane] = s;
    }
    __syncthreads();
  }
  if (cok)
    for (int i = wave; i < nb; i += MEL_WAVES)
      out[(sig * n_mels + m0 + i) * T + t] = Acc[i * MEL_TT + lane];
}

template <typename R, int BT>
static int mel_fwd_launch(const void* spec, int64_t n_signals, int F, int64_t T,
                          const int32_t* band_lo, const int32_t* band_off, const float* weights,
                          int64_t n_weights, int n_mels, double power, void* out, hipStream_t s) {
  static_assert(BT <= 64, "a band's weights within a chunk are held one per lane");
  constexpr int GMAX = 32768 / (MEL_TT * (int)sizeof(R));   // 32 KiB of accumulators
  const int64_t ncols = n_signals * T;
  const int64_t tiles = cdiv(ncols, MEL_TT);
  if (tiles > 0x7fffffff) return record_msg("ainp_mel_fwd: too many frames");
  // all bands in one workgroup when the column tiles fill the machine (each
  // element fetched once); otherwise groups of >= 8 bands, for ~2 workgroups
  // per CU
  int64_t groups = cdiv(n_mels, GMAX);
  groups = std::max<int64_t>(groups, std::min<int64_t>(cdiv(512, tiles), cdiv(n_mels, 8)));
  const int G = (int)cdiv(n_mels, groups);
  groups = cdiv(n_mels, G);
  if (groups > 65535) return record_msg("ainp_mel_fwd: too many mel bands");
  const bool wlds = n_weights <= 4096;   // 16 KiB; a mel bank has <= 2 weights per bin
  const int wcap = wlds ? (int)n_weights : 0;
  const size_t lds = ((size_t)BT + G) * MEL_TT * sizeof(R) + 3 * (size_t)G * sizeof(int) +
                     (size_t)wcap * sizeof(float);
  const dim3 grid((unsigned)tiles, (unsigned)groups);
  const Cplx<R>* x = reinterpret_cast<const Cplx<R>*>(spec);
#define AINP_MEL_FWD_W(PM, W)                                                                    \
  hipLaunchKernelGGL((mel_fwd_kernel<R, BT, PM, W>), grid, dim3(MEL_THREADS), lds, s, x, ncols, \
                     F, T, band_lo, band_off, weights, n_weights, n_mels, G, wcap,              \
                     (R)(0.5 * power), (R*)out)
#define AINP_MEL_FWD(PM)         \
  do {                           \
    if (wlds) AINP_MEL_FWD_W(PM, true); \
    else AINP_MEL_FWD_W(PM, false);     \
  } while (0)
  if (power == 2.0) AINP_MEL_FWD(MEL_POW_TWO);
  else if (power == 1.0) AINP_MEL_FWD(MEL_POW_ONE);
  else AINP_MEL_FWD(MEL_POW_GENERAL);
#undef AINP_MEL_FWD_W
#undef AINP_MEL_FWD
  return check_launch("ainp_mel_fwd");
}

// ------------------------------------------------------------------ inverse
typedef float mel_f32x16 __attribute__((ext_vector_type(16)));
constexpr int MEL_KC = 128;   // k per staged chunk (the usual n_mels in one)

// grid: x = 64 columns of the flat [signal][frame] axis, y = 128 bins (a wave
// per 32).  Operand maps of the 32x32x2 MFMA (as gemm.hip): lane (li, lh)
// holds A[row li][k = lh], B[k = lh][col li]; D[row (r&3)+8(r>>2)+4lh][col li].
// Within a group of 8 k the half lh takes k = 4lh + e in step e, for A and B
// alike, so the chain runs over a fixed permutation of k.
// Per chunk of 128 k every load is issued up front -- the workgroup's
// [128 k][64 columns] of M into LDS (loads along T), each wave's 32 rows of P
// into registers -- so the 128 MFMAs of a wave run without waiting on memory.
template <bool VEC>
__global__ __launch_bounds__(MEL_THREADS, 2) void mel_inverse_kernel(
    const float* __restrict__ P, const float* __restrict__ M, int64_t ncols, int64_t T, int F,
    int K, int flags, float* __restrict__ L) {
  __shared__ float Ms[MEL_KC * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int f0 = blockIdx.y * 128 + wave * 32;
  const bool wave_on = f0 < F;          // a wave past F still helps stage M
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  const bool fok = f0 + li < F;
  const float* pa = P + (int64_t)(fok ? f0 + li : 0) * K;
  // staging column (lane) and the two MFMA columns (li, li + 32)
  const int64_t scol = c0 + lane;
  const bool sok = scol < ncols;
  const int64_t ssig = sok ? scol / T : 0;
  const float* ps = M + ssig * K * T + (sok ? scol - ssig * T : 0);
  bool cok[2];
  float* po[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t col = c0 + 32 * j + li;
    cok[j] = col < ncols;
    const int64_t sig = cok[j] ? col / T : 0;
    po[j] = L + sig * F * T + (cok[j] ? col - sig * T : 0);
  }
  mel_f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  for (int kb = 0; kb < K; kb += MEL_KC) {
    const int kn = min(MEL_KC, K - kb);
    // rows wave, wave + 4, ... of M's chunk (zeros past K and past the last column)
    float mv[MEL_KC / MEL_WAVES];
#pragma unroll
    for (int i = 0; i < MEL_KC / MEL_WAVES; ++i) {
      const int k = wave + MEL_WAVES * i;
      mv[i] = (sok && k < kn) ? ps[(int64_t)(kb + k) * T] : 0.f;
    }
    // this lane's k = 8 kg + 4 lh + e of its row of P (zeros past K and past F)
    float a[MEL_KC / 8][4];
#pragma unroll
    for (int kg = 0; kg < MEL_KC / 8; ++kg) {
      const int k = 8 * kg + 4 * lh;
      if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (wave_on && fok && k < kn) v = *reinterpret_cast<const float4*>(pa + kb + k);
        a[kg][0] = v.x, a[kg][1] = v.y, a[kg][2] = v.z, a[kg][3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a[kg][e] = (wave_on && fok && k + e < kn) ? pa[kb + k + e] : 0.f;
      }
    }
    if (kb) __syncthreads();   // the previous chunk's reads of Ms are done
#pragma unroll
    for (int i = 0; i < MEL_KC / MEL_WAVES; ++i) Ms[(wave + MEL_WAVES * i) * 64 + lane] = mv[i];
    __syncthreads();
    if (wave_on) {
#pragma unroll
      for (int kg = 0; kg < MEL_KC / 8; ++kg) {
        if (8 * kg >= kn) break;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* row = Ms + (8 * kg + 4 * lh + e) * 64 + li;
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kg][e], row[32 * j], acc[j], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_on) return;

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!cok[j]) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = f0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (f >= F) continue;
      float v = acc[j][r];
      if (flags & AINP_MEL_CLAMP) v = fmaxf(v, 0.f);
      if (flags & AINP_MEL_SQRT) v = sqrtf(v);
      po[j][(int64_t)f * T] = v;
    }
  }
}

}  // namespace ainp

using namespace ainp;

extern "C" int ainp_mel_fwd(const void* spec, int dtype, int64_t n_signals, int n_bins,
                            int64_t n_frames, const int32_t* band_lo, const int32_t* band_off,
                            const float* weights, int64_t n_weights, int n_mels, double power,
                            void* out, void* stream) {
  if (!spec || !band_lo || !band_off || !weights || !out || n_signals < 0 || n_weights < 0)
    return record_msg("ainp_mel_fwd: bad argument");
  if (n_mels < 1 || n_bins < 2 || n_frames < 1)
    return record_msg("ainp_mel_fwd: bad argument (n_mels >= 1, n_bins >= 2, n_frames >= 1)");
  if (!(power >= 0.0) || !isfinite(power))
    return record_msg("ainp_mel_fwd: power must be finite and non-negative");
  if (dtype != 0 && dtype != 1)
    return record_msg("ainp_mel_fwd: dtype must be 0 (complex64) or 1 (complex128)");
  if (n_signals == 0) return AINP_OK;
  hipStream_t s = as_stream(stream);
  if (dtype == 0)
    return mel_fwd_launch<float, 64>(spec, n_signals, n_bins, n_frames, band_lo, band_off,
                                     weights, n_weights, n_mels, power, out, s);
  return mel_fwd_launch<double, 32>(spec, n_signals, n_bins, n_frames, band_lo, band_off, weights,
                                    n_weights, n_mels, power, out, s);
}

extern "C" int ainp_mel_inverse(const float* pinv, const float* mel, int64_t n_signals,
                                int n_bins, int n_mels, int64_t n_frames, int flags, float* out,
                                void* stream) {
  if (!pinv || !mel || !out || n_signals < 0)
    return record_msg("ainp_mel_inverse: bad argument");
  if (n_mels < 1 || n_bins < 2 || n_frames < 1)
    return record_msg("ainp_mel_inverse: bad argument (n_mels >= 1, n_bins >= 2, n_frames >= 1)");
  if (flags & ~(AINP_MEL_SQRT | AINP_MEL_CLAMP))
    return record_msg("ainp_mel_inverse: unknown flag bits");
  if (n_signals == 0) return AINP_OK;
  const int64_t ncols = n_signals * n_frames;
  const int64_t gx = cdiv(ncols, 64), gy = cdiv(n_bins, 128);
  if (gx > 0x7fffffff || gy > 65535) return record_msg("ainp_mel_inverse: problem too large");
  const dim3 grid((unsigned)gx, (unsigned)gy);
  hipStream_t s = as_stream(stream);
  // 16-byte loads of P's rows: every row start and k = 4 * i is aligned
  if (n_mels % 4 == 0 && (reinterpret_cast<uintptr_t>(pinv) & 15) == 0)
    hipLaunchKernelGGL(mel_inverse_kernel<true>, grid, dim3(MEL_THREADS), 0, s, pinv, mel, ncols,
                       n_frames, n_bins, n_mels, flags, out);
  else
    hipLaunchKernelGGL(mel_inverse_kernel<false>, grid, dim3(MEL_THREADS), 0, s, pinv, mel, ncols,
                       n_frames, n_bins, n_mels, flags, out);
  return check_launch("ainp_mel_inverse");
}
