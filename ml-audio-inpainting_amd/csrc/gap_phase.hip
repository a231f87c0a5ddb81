// gap_phase.hip — gap-constrained Griffin-Lim (include/ainp.h: ainp_gap_phase):
// a phase for the frames whose window touches a missing sample and new values
// for the missing samples only, every reliable sample and frame left alone.
//
// grid: one workgroup per run of unreliable frames (gap_phase_plan.h finds the
// runs and sizes the workgroup), one launch for the whole batch and all
// iterations.  The run's span y, (R - 1) hop + n_fft doubles, and the
// overlap-add numerator stay in LDS from the first iteration to the last; the
// signal makes no trip to memory in between.  Waves take the frames
// round-robin, `waves` at a time: a wave windows its frame out of y into its
// own split re / im arrays (the half-length complex scheme of spain_fft.h,
// skewed by sp_pad, wave-level barriers), transforms, and holds the half
// spectrum in registers (slot p of a lane: bins p and N - p) for the residual,
// the momentum step against tprev, the normalisation and the product with the
// target magnitudes, then transforms back.  After each round the workgroup adds
// the round's frames into the numerator, a thread per sample over ascending t,
// so the sum over all frames runs in ascending t whatever the wave count.
// resid^2 is a wave's fixed butterfly sum per frame, then one thread's sum over
// ascending frames.  No atomics: two launches give the same bits.
//
// tprev and the magnitudes are read and written once per frame and iteration
// by the lane that owns the slot, 16 and 8 bytes a lane, contiguous over the
// lanes: in LDS where the plan says they fit, else in the run's slice of the
// workspace (it stays in L2: about 60 KB for 15 frames of n_fft 512).
#include <string>

#include "common.h"
#include "gap_phase_plan.h"
#include "spain_fft.h"

namespace ainp {

struct GpArgs {
  int64_t rows, S, T;
  int n_fft, lgN, hop, n_iter, max_frames, slots;
  double mom;            // momentum / (1 + momentum)
  int64_t state_bytes;   // a run's slice of the workspace
  GpLayout lay;
};

__device__ __forceinline__ double gp_abs(cplx a) { return sqrt(cabs2(a)); }
// A a / (|a| + tiny): the unit phase of a (0 for a == 0) at magnitude A
__device__ __forceinline__ cplx gp_project(cplx a, double A) {
  const double d = gp_abs(a) + 2.2250738585072014e-308;
  return {A * (a.re / d), A * (a.im / d)};
}

template <typename Tio, int EPL, bool SLDS>
__global__ __launch_bounds__(64 * GP_WAVES_MAX) void gap_phase_kernel(
    const Tio* __restrict__ x, Tio* __restrict__ out, const uint8_t* __restrict__ mask,
    const float* __restrict__ mag, const int32_t* __restrict__ run_row,
    const int32_t* __restrict__ run_first, const int32_t* __restrict__ run_frames,
    const double* __restrict__ window, double* __restrict__ resid,
    unsigned char* __restrict__ ws, GpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = blockDim.x, NW = NT >> 6;
  const int run = blockIdx.x;
  const int64_t row = run_row[run], t0 = run_first[run];
  const int R = run_frames[run];
  // a run the tables misstate is skipped whole (uniform over the workgroup)
  if (row < 0 || row >= a.rows || t0 < 0 || R < 1 || R > a.max_frames || t0 + R > a.T) return;
  const int M = a.n_fft, N = M >> 1, hop = a.hop, SL = a.slots;
  const int L = (R - 1) * hop + M;
  const int64_t s0 = t0 * hop - N;   // the span's first sample (may be < 0: padding)

  double* ct = reinterpret_cast<double*>(smem + a.lay.ct);
  double* w = reinterpret_cast<double*>(smem + a.lay.w);
  double* y = reinterpret_cast<double*>(smem + a.lay.y);
  double* num = reinterpret_cast<double*>(smem + a.lay.num);
  double* rpart = reinterpret_cast<double*>(smem + a.lay.rpart);
  double* scr = reinterpret_cast<double*>(smem + a.lay.scr);
  uint8_t* mk = smem + a.lay.mk;
  cplx* tp;
  float2* am;
  float* nyq;
  if constexpr (SLDS) {
    tp = reinterpret_cast<cplx*>(smem + a.lay.tp);
    am = reinterpret_cast<float2*>(smem + a.lay.am);
    nyq = reinterpret_cast<float*>(smem + a.lay.nyq);
  } else {
    unsigned char* base = ws + (int64_t)run * a.state_bytes;
    tp = reinterpret_cast<cplx*>(base + a.lay.tp);
    am = reinterpret_cast<float2*>(base + a.lay.am);
    nyq = reinterpret_cast<float*>(base + a.lay.nyq);
  }

  for (int j = tid; j <= M / 4; j += NT) ct[j] = cospi((double)(2 * j) / (double)M);
  for (int n = tid; n < M; n += NT) w[n] = window[n];
  const Tio* __restrict__ xr = x + row * a.S;
  const uint8_t* __restrict__ mr = mask + row * a.S;
  for (int j = tid; j < L; j += NT) {
    const int64_t s = s0 + j;
    const bool in = s >= 0 && s < a.S;
    const bool miss = in && mr[s] == 0;
    double v = in ? (double)xr[s] : 0.0;
    if (miss && v != v) v = 0.0;
    y[j] = v;
    mk[j] = miss;
  }
  // the magnitudes in slot order: slot p holds A[p] and A[N - p]; slot 0 A[0]
  // and A[N/2], the Nyquist bin A[N] beside them
  const float* __restrict__ mg = mag + row * (int64_t)(N + 1) * a.T + t0;
  for (int i = tid; i < R * SL; i += NT) {
    const int t = i / SL, p = i - t * SL;
    float2 v = make_float2(0.f, 0.f);
    if (p < N / 2) {
      v.x = mg[(int64_t)p * a.T + t];
      v.y = mg[(int64_t)(p ? N - p : N / 2) * a.T + t];
      if (p == 0) nyq[t] = mg[(int64_t)N * a.T + t];
    }
    am[i] = v;
  }
  __syncthreads();

  // the frames over sample j of the span, clipped to the run
  auto frames_over = [&](int j, int& ta, int& tb) {
    ta = j < M ? 0 : (j - M) / hop + 1;
    tb = min(R - 1, j / hop);
  };
  // window sum-square over ascending frames
  auto wss = [&](int j) {
    int ta, tb;
    frames_over(j, ta, tb);
    double den = 0.0;
    for (int t = ta; t <= tb; ++t) {
      const double wv = w[j - t * hop];
      den += wv * wv;
    }
    return den;
  };
  // a missing sample under no window of the run is not this run's: it keeps its value
  for (int j = tid; j < L; j += NT)
    if (mk[j] && !(wss(j) > 0.0)) mk[j] = 0;
  __syncthreads();

  const int P = a.lay.scr_len;
  const SpFft f = {scr + (size_t)wave * 2 * P, scr + (size_t)wave * 2 * P + P, ct, N, a.lgN, M};
  const double inv = 1.0 / (double)N;   // the N-point sum -> irfft, a power of two

  for (int k = 0; k < a.n_iter; ++k) {
    for (int j = tid; j < L; j += NT) num[j] = 0.0;
    for (int r0 = 0; r0 < R; r0 += NW) {
      const int t = r0 + wave;
      if (t < R) {
        const double* yf = y + t * hop;
        for (int n = lane; n < N; n += 64)
          f.st(n, {yf[2 * n] * w[2 * n], yf[2 * n + 1] * w[2 * n + 1]});
        sp_barrier<true>();
        sp_dif<64, true>(f, lane);
        SpSpec<EPL> X;
        sp_split<64, EPL>(f, lane, 1.0, X);
        double r2 = 0.0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int p = lane + e * 64;
          if (p >= N / 2) continue;
          const float2 af = am[t * SL + p];
          const double Aa = (double)af.x, Ab = (double)af.y;
          cplx* tpa = tp + (size_t)(2 * t) * SL + p;
          cplx* tpb = tpa + SL;
          cplx ga = X.a[e], gb = X.b[e];
          if (k > 0) {
            const cplx pa = *tpa, pb = *tpb;
            ga = {ga.re - a.mom * pa.re, ga.im - a.mom * pa.im};
            gb = {gb.re - a.mom * pb.re, gb.im - a.mom * pb.im};
          }
          *tpa = X.a[e];
          *tpb = X.b[e];
          const double db = gp_abs(X.b[e]) - Ab;
          if (p == 0) {   // a = (X[0], X[N]), both real; b = X[N/2]
            const double An = (double)nyq[t];
            const double d0 = fabs(X.a[e].re) - Aa, dn = fabs(X.a[e].im) - An;
            r2 += d0 * d0 + dn * dn + 2.0 * (db * db);
            const cplx z0 = gp_project({ga.re, 0.0}, Aa), zn = gp_project({ga.im, 0.0}, An);
            X.a[e] = {z0.re, zn.re};
          } else {
            const double da = gp_abs(X.a[e]) - Aa;
            r2 += 2.0 * (da * da + db * db);
            X.a[e] = gp_project(ga, Aa);
          }
          X.b[e] = gp_project(gb, Ab);
        }
        r2 = wave_sum_d(r2);
        if (lane == 0) rpart[t] = r2;
        // a lane's merge writes the cells its split read: no barrier in between
        sp_merge<64, EPL>(f, lane, X);
        sp_barrier<true>();
        sp_dit<64, true>(f, lane);
      }
      __syncthreads();
      // num += the round's frames x window, ascending t
      const int r1 = min(R, r0 + NW);
      const int hi = (r1 - 1) * hop + M;
      for (int j = r0 * hop + tid; j < hi; j += NT) {
        if (!mk[j]) continue;
        int ta, tb;
        frames_over(j, ta, tb);
        ta = max(ta, r0);
        tb = min(tb, r1 - 1);
        double acc = num[j];
        for (int t = ta; t <= tb; ++t) {
          const int o = j - t * hop;
          const double* re = scr + (size_t)(t - r0) * 2 * P;
          const double v = (o & 1) ? re[P + sp_pad(o >> 1)] : re[sp_pad(o >> 1)];
          acc += (v * inv) * w[o];
        }
        num[j] = acc;
      }
      __syncthreads();
    }
    for (int j = tid; j < L; j += NT)
      if (mk[j]) y[j] = num[j] / wss(j);
    if (tid == 0 && resid) {
      double s = 0.0;
      for (int t = 0; t < R; ++t) s += rpart[t];
      resid[(int64_t)run * a.n_iter + k] = sqrt(s);
    }
    __syncthreads();
  }

  Tio* __restrict__ orow = out + row * a.S;
  for (int j = tid; j < L; j += NT)
    if (mk[j]) orow[s0 + j] = (Tio)y[j];
}

template <typename Tio, int EPL>
static int gap_phase_launch(const void* x, void* out, const uint8_t* mask, const float* mag,
                            const int32_t* run_row, const int32_t* run_first,
                            const int32_t* run_frames, int64_t n_runs, const double* window,
                            double* resid, void* ws, const GpArgs& a, const GpPlan& p,
                            hipStream_t s) {
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)gap_phase_kernel<Tio, EPL, true>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)GP_LDS_MAX) == hipSuccess &&
      hipFuncSetAttribute((const void*)gap_phase_kernel<Tio, EPL, false>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)GP_LDS_MAX) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_gap_phase: cannot reserve 160 KB of LDS");
  const dim3 grid((unsigned)n_runs), block(64 * p.waves);
  if (p.residency == AINP_GP_LDS)
    hipLaunchKernelGGL((gap_phase_kernel<Tio, EPL, true>), grid, block, (size_t)p.lds_bytes, s,
                       (const Tio*)x, (Tio*)out, mask, mag, run_row, run_first, run_frames, window,
                       resid, (unsigned char*)ws, a);
  else
    hipLaunchKernelGGL((gap_phase_kernel<Tio, EPL, false>), grid, block, (size_t)p.lds_bytes, s,
                       (const Tio*)x, (Tio*)out, mask, mag, run_row, run_first, run_frames, window,
                       resid, (unsigned char*)ws, a);
  return check_launch("ainp_gap_phase");
}

static const char GP_SHAPE_RULE[] =
    "n_fft a power of two in [16, 2048], 1 <= win_length <= n_fft, 1 <= hop < win_length";
static const char GP_CAP_RULE[] =
    "a run longer than the cap: its span and one wave's transform do not fit in 160 KB of LDS";

}  // namespace ainp

using namespace ainp;

extern "C" int64_t ainp_gap_phase_plan(const uint8_t* mask, int64_t n_samples, int n_fft, int hop,
                                       int win_length, AinpGapPhaseRun* runs, int64_t max_runs) {
  if (max_runs < 0 || (max_runs > 0 && !runs))
    return record_bad_argument("ainp_gap_phase_plan", "runs holds max_runs >= 0 entries");
  const int64_t n = gp_find_runs(mask, n_samples, n_fft, hop, win_length, runs, max_runs);
  if (n == -1) return record_bad_argument("ainp_gap_phase_plan", GP_SHAPE_RULE);
  if (n == -2) {
    record_msg((std::string("ainp_gap_phase_plan: ") + GP_CAP_RULE).c_str());
    return AINP_EUNSUPPORTED;
  }
  return n;
}

extern "C" size_t ainp_gap_phase_workspace(int64_t n_runs, int64_t max_frames, int n_fft,
                                           int hop) {
  const GpPlan p = gp_plan(n_fft, hop, max_frames);
  if (!p.ok || n_runs <= 0 || p.residency == AINP_GP_LDS) return 0;
  return (size_t)n_runs * (size_t)p.state_bytes;
}

extern "C" int ainp_gap_phase(const void* x, void* out, int dtype, int64_t rows,
                              int64_t n_samples, const uint8_t* mask, const float* mag,
                              int64_t n_frames, const int32_t* run_row, const int32_t* run_first,
                              const int32_t* run_frames, int64_t n_runs, int64_t max_frames,
                              const double* window, int n_fft, int hop, int win_length,
                              int n_iter, double momentum, double* resid, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (dtype != 0 && dtype != 1)
    return record_bad_argument("ainp_gap_phase", "dtype 0 (float32) or 1 (float64)");
  if (!gp_shape_ok(n_fft, hop, win_length))
    return record_bad_argument("ainp_gap_phase", GP_SHAPE_RULE);
  if (n_iter < 1 || n_iter > GP_ITER_MAX || !(momentum >= 0.0 && momentum <= 1.0))
    return record_bad_argument("ainp_gap_phase", "n_iter in [1, 1000], momentum in [0, 1]");
  if (rows < 0 || n_runs < 0 || n_runs > 0x7fffffff || n_samples < 0 ||
      n_samples > 0x7fffffff || n_frames != 1 + n_samples / hop)
    return record_bad_argument("ainp_gap_phase",
                               "rows, n_runs >= 0, n_samples <= 2^31 - 1, "
                               "n_frames = 1 + n_samples / hop");
  if (n_runs == 0) return AINP_OK;
  if (max_frames < 1 || max_frames > n_frames)
    return record_bad_argument("ainp_gap_phase", "1 <= max_frames <= n_frames");
  const GpPlan p = gp_plan(n_fft, hop, max_frames);
  if (!p.ok) {
    record_msg((std::string("ainp_gap_phase: ") + GP_CAP_RULE).c_str());
    return AINP_EUNSUPPORTED;
  }
  const size_t need = ainp_gap_phase_workspace(n_runs, max_frames, n_fft, hop);
  if (!x || !out || x == out || !mask || !mag || !run_row || !run_first || !run_frames ||
      !window || rows == 0 || (need > 0 && (!workspace || workspace_bytes < need)))
    return record_bad_argument("ainp_gap_phase");
  GpArgs a;
  a.rows = rows;
  a.S = n_samples;
  a.T = n_frames;
  a.n_fft = n_fft;
  a.lgN = 0;
  while ((2 << a.lgN) < n_fft) ++a.lgN;   // N = n_fft / 2 = 2^lgN
  a.hop = hop;
  a.n_iter = n_iter;
  a.max_frames = (int)max_frames;
  a.slots = p.slots;
  a.mom = momentum / (1.0 + momentum);
  a.state_bytes = p.state_bytes;
  a.lay = p.lay;
  hipStream_t s = as_stream(stream);
#define AINP_GP(T, E)                                                                         \
  return gap_phase_launch<T, E>(x, out, mask, mag, run_row, run_first, run_frames, n_runs,   \
                                window, resid, workspace, a, p, s)
#define AINP_GP_E(T)                  \
  switch (p.slots / 64) {             \
    case 1: AINP_GP(T, 1);            \
    case 2: AINP_GP(T, 2);            \
    case 4: AINP_GP(T, 4);            \
    default: AINP_GP(T, 8);           \
  }
  if (dtype == 0) {
    AINP_GP_E(float)
  }
  AINP_GP_E(double)
#undef AINP_GP_E
#undef AINP_GP
}
