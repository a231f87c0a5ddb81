// resample.hip — rational-ratio polyphase FIR resampling (include/ainp.h:
// ainp_resample_poly; scipy.signal.resample_poly with its defaults, the 48 kHz
// export of models/AudioReg/train.m:72,203 and utils.load_audio's resampling).
//
// The host designs the filter in float64 (ainp/resample.py) and hands it over
// phase-major, table[p][k] = h[p + (tpp - 1 - k) up]; resample_plan.h decides
// tile, span and route for the launcher and the host query alike.
//
// grid: x = tiles of plan.tile outputs over [0, stride_out), y = rows; 256
// threads.  A workgroup stages the inputs its tile reads -- the span that
// starts at floor((m0 down + half) / up) - tpp + 1 for its first output m0 --
// into LDS with 16-byte loads where the row allows them, zeros for i < 0 and
// i >= n_in[r] (such samples are never read from memory), and on
// AINP_RS_LDS_TABLE the whole table behind it.  Lane t then produces outputs
// m0 + t, m0 + t + 256, ...: consecutive lanes hold consecutive outputs, so
// stores coalesce, neighbouring lanes read neighbouring (or, upsampling, the
// same) staged samples, and their phases differ, which the table's odd pitch
// spreads over the LDS banks.  m0 down is formed in 64 bits; inside the tile a
// lane divides once and then steps by the quotient and remainder of 256 down
// by up.  Each output is one chain of tpp fmas over ascending inputs in the
// element type.  Outputs past min(ceil(n_in up / down), stride_out) are written
// as zeros.  No atomics, nothing shared between workgroups: the same bits on
// every call.
#include <algorithm>

#include "common.h"
#include "resample_plan.h"

namespace ainp {

constexpr int RS_CHAINS = 4;   // outputs a lane computes side by side
constexpr int RS_STAGE = 4;    // 16-byte groups a lane loads before it stores them

struct RsArgs {
  int64_t stride_in, stride_out;
  int up, down, half, tpp, pitch, tile;
  int span_lds;    // staged elements (a multiple of the 16-byte group)
  int step_q, step_r;   // RS_THREADS * down = step_q * up + step_r
  int table_elems;
  int vec;         // rows start 16-byte aligned: stage with 16-byte loads
};

template <typename R>
struct RsVec;
template <>
struct RsVec<float> {
  typedef float4 type;
  static constexpr int N = 4;
};
template <>
struct RsVec<double> {
  typedef double2 type;
  static constexpr int N = 2;
};

template <typename R, bool TLDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    R* __restrict__ y, const R* __restrict__ x, const R* __restrict__ table,
    const int32_t* __restrict__ n_in, RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int V = RsVec<R>::N;
  typedef typename RsVec<R>::type VT;
  R* xs = reinterpret_cast<R*>(smem);   // [span_lds]
  R* ts = xs + a.span_lds;              // [table_elems] (TLDS)
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.y;
  const int64_t m0 = (int64_t)blockIdx.x * a.tile;
  const int64_t n = min(max((int64_t)n_in[r], (int64_t)0), a.stride_in);
  const int64_t n_out = (n * a.up + a.down - 1) / a.down;
  const int64_t limit = min(n_out, a.stride_out);
  R* __restrict__ yr = y + r * a.stride_out;
  const int64_t m_end = min(m0 + a.tile, a.stride_out);

  if (m0 >= limit) {   // a tile of the zero fill: nothing to stage
    for (int64_t m = m0 + tid; m < m_end; m += RS_THREADS) yr[m] = (R)0;
    return;
  }

  const int64_t c0 = m0 * a.down + a.half;
  const int64_t q0 = c0 / a.up;
  const int p0 = (int)(c0 - q0 * a.up);
  const int64_t b = q0 - a.tpp + 1;            // first input of the tile (may be < 0)
  const int64_t ba = b & ~(int64_t)(V - 1);    // the 16-byte group at or below it
  const int lead = (int)(b - ba);
  const R* __restrict__ xr = x + r * a.stride_in;

  // stage [ba, ba + span_lds): whole groups inside [0, n) by one 16-byte load
  // RS_STAGE loads of a lane are issued before the first of them is stored,
  // so a staging loop pays the memory latency once per batch, not per group
  for (int j0 = tid * V; j0 < a.span_lds; j0 += RS_STAGE * RS_THREADS * V) {
    R v[RS_STAGE][V];
#pragma unroll
    for (int u = 0; u < RS_STAGE; ++u) {
      const int j = j0 + u * RS_THREADS * V;
      const int64_t i = ba + j;
      if (a.vec && j < a.span_lds && i >= 0 && i + V <= n) {
        const VT w = *reinterpret_cast<const VT*>(xr + i);
        const R* we = reinterpret_cast<const R*>(&w);
#pragma unroll
        for (int e = 0; e < V; ++e) v[u][e] = we[e];
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
          v[u][e] = (j < a.span_lds && i + e >= 0 && i + e < n) ? xr[i + e] : (R)0;
      }
    }
#pragma unroll
    for (int u = 0; u < RS_STAGE; ++u) {
      const int j = j0 + u * RS_THREADS * V;
      if (j < a.span_lds) {
#pragma unroll
        for (int e = 0; e < V; ++e) xs[j + e] = v[u][e];
      }
    }
  }
  if (TLDS) {   // table_elems may be odd: 16-byte groups, then the tail
    const int nv = a.table_elems / V;
    for (int j0 = tid; j0 < nv; j0 += RS_STAGE * RS_THREADS) {
      VT w[RS_STAGE];
#pragma unroll
      for (int u = 0; u < RS_STAGE; ++u) {
        const int j = j0 + u * RS_THREADS;
        w[u] = reinterpret_cast<const VT*>(table)[j < nv ? j : j0];
      }
#pragma unroll
      for (int u = 0; u < RS_STAGE; ++u) {
        const int j = j0 + u * RS_THREADS;
        if (j < nv) reinterpret_cast<VT*>(ts)[j] = w[u];
      }
    }
    for (int j = nv * V + tid; j < a.table_elems; j += RS_THREADS) ts[j] = table[j];
  }
  __syncthreads();

  // this lane's first output: one division, then steps of (step_q, step_r)
  const int64_t cl = (int64_t)p0 + (int64_t)tid * a.down;
  int qo = (int)(cl / a.up);          // floor(c / up) - q0, < span
  int ph = (int)(cl - (int64_t)qo * a.up);
  const R* __restrict__ tb = TLDS ? ts : table;
  // RS_CHAINS outputs of a lane advance together, so that many independent
  // LDS reads are in flight; each output is still its own chain over ascending
  // k.  An output at or past `limit` runs on the tile's first taps (in bounds)
  // and is stored as zero.
  for (int64_t mb = m0 + tid; mb < m_end; mb += RS_CHAINS * RS_THREADS) {
    int xo[RS_CHAINS];        // offsets into xs and the table
    int64_t to[RS_CHAINS];
    R acc[RS_CHAINS];
    bool on[RS_CHAINS];
#pragma unroll
    for (int e = 0; e < RS_CHAINS; ++e) {
      on[e] = mb + e * RS_THREADS < min(limit, m_end);   // inside the tile's span
      xo[e] = lead + (on[e] ? qo : 0);
      to[e] = on[e] ? (int64_t)ph * a.pitch : (int64_t)0;
      acc[e] = (R)0;
      qo += a.step_q;
      ph += a.step_r;
      if (ph >= a.up) {
        ph -= a.up;
        ++qo;
      }
    }
#pragma unroll 2
    for (int k = 0; k < a.tpp; ++k) {
#pragma unroll
      for (int e = 0; e < RS_CHAINS; ++e) acc[e] = fma(xs[xo[e] + k], tb[to[e] + k], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < RS_CHAINS; ++e) {
      const int64_t m = mb + e * RS_THREADS;
      if (m < m_end) yr[m] = on[e] ? acc[e] : (R)0;
    }
  }
}

// up == down after reduction: y[r][m] = x[r][m] below min(n_in[r], stride_out), zero above
template <typename R>
__global__ __launch_bounds__(RS_THREADS) void resample_copy_kernel(
    R* __restrict__ y, const R* __restrict__ x, const int32_t* __restrict__ n_in,
    int64_t stride_in, int64_t stride_out, int tile) {
  const int64_t r = blockIdx.y;
  const int64_t n = min(max((int64_t)n_in[r], (int64_t)0), stride_in);
  const int64_t limit = min(n, stride_out);
  const int64_t m0 = (int64_t)blockIdx.x * tile;
  const int64_t m_end = min(m0 + tile, stride_out);
  for (int64_t m = m0 + threadIdx.x; m < m_end; m += RS_THREADS)
    y[r * stride_out + m] = m < limit ? x[r * stride_in + m] : (R)0;
}

template <typename R>
static int resample_launch(void* y, const void* x, const void* table, int64_t rows,
                           int64_t stride_in, int64_t stride_out, const int32_t* n_in,
                           const RsPlan& p, hipStream_t s) {
  const int64_t tiles = cdiv(stride_out, p.tile);
  if (tiles > 0x7fffffff || rows > 65535)
    return record_bad_argument("ainp_resample_poly", "rows <= 65535, stride_out / tile < 2^31");
  const dim3 grid((unsigned)tiles, (unsigned)rows);
  if (p.route == AINP_RS_COPY) {
    hipLaunchKernelGGL(resample_copy_kernel<R>, grid, dim3(RS_THREADS), 0, s, (R*)y, (const R*)x,
                       n_in, stride_in, stride_out, p.tile);
    return check_launch("ainp_resample_poly");
  }
  constexpr int V = RsVec<R>::N;
  RsArgs a;
  a.stride_in = stride_in;
  a.stride_out = stride_out;
  a.up = p.up;
  a.down = p.down;
  a.half = p.half;
  a.tpp = p.tpp;
  a.pitch = p.pitch;
  a.tile = p.tile;
  a.span_lds = (int)rs_span_lds(p.span, (int)sizeof(R));
  const int64_t step = (int64_t)RS_THREADS * p.down;
  a.step_q = (int)(step / p.up);
  a.step_r = (int)(step % p.up);
  a.table_elems = (int)p.table_elems;
  a.vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && stride_in % V == 0;
  const bool tlds = p.route == AINP_RS_LDS_TABLE;
  // the 16-byte table copy needs the table aligned; a cached device tensor is
  if (tlds && (reinterpret_cast<uintptr_t>(table) & 15) != 0)
    return record_bad_argument("ainp_resample_poly", "table 16-byte aligned");
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)resample_kernel<R, true>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)RS_LDS_MAX) == hipSuccess &&
      hipFuncSetAttribute((const void*)resample_kernel<R, false>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)RS_LDS_MAX) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_resample_poly: cannot reserve 160 KB of LDS");
  if (tlds)
    hipLaunchKernelGGL((resample_kernel<R, true>), grid, dim3(RS_THREADS), (size_t)p.lds_bytes, s,
                       (R*)y, (const R*)x, (const R*)table, n_in, a);
  else
    hipLaunchKernelGGL((resample_kernel<R, false>), grid, dim3(RS_THREADS), (size_t)p.lds_bytes,
                       s, (R*)y, (const R*)x, (const R*)table, n_in, a);
  return check_launch("ainp_resample_poly");
}

static const char RS_RATIO_RULE[] =
    "up, down >= 1 and a filter of 20 max(up, down) + 1 taps that fits in 160 KB of LDS";

}  // namespace ainp

using namespace ainp;

extern "C" int64_t ainp_resample_out_len(int64_t n_in, int up, int down) {
  if (n_in > 0x7fffffff) return -1;
  return rs_out_len(n_in, up, down);
}

extern "C" int ainp_resample_plan_query(int up, int down, int dtype, AinpResamplePlan* plan) {
  if (!plan) return record_bad_argument("ainp_resample_plan_query");
  *plan = AinpResamplePlan{};
  if (dtype != 0 && dtype != 1)
    return record_bad_argument("ainp_resample_plan_query", "dtype 0 (float32) or 1 (float64)");
  const RsPlan p = rs_plan(up, down, dtype ? 8 : 4);
  if (!p.ok) return record_bad_argument("ainp_resample_plan_query", RS_RATIO_RULE);
  plan->up = p.up;
  plan->down = p.down;
  plan->half = p.half;
  plan->taps = p.taps;
  plan->tpp = p.tpp;
  plan->pitch = p.pitch;
  plan->tile = p.tile;
  plan->span = p.span;
  plan->route = p.route;
  plan->table_elems = p.table_elems;
  plan->lds_bytes = p.lds_bytes;
  return AINP_OK;
}

extern "C" int ainp_resample_poly(void* y, const void* x, const void* table, int64_t rows,
                                  int64_t stride_in, int64_t stride_out, const int32_t* n_in,
                                  int up, int down, int dtype, void* stream) {
  if (dtype != 0 && dtype != 1)
    return record_bad_argument("ainp_resample_poly", "dtype 0 (float32) or 1 (float64)");
  const RsPlan p = rs_plan(up, down, dtype ? 8 : 4);
  if (!p.ok) return record_bad_argument("ainp_resample_poly", RS_RATIO_RULE);
  if (rows < 0 || stride_in < 0 || stride_out < 0 || stride_in > 0x7fffffff)
    return record_bad_argument("ainp_resample_poly",
                               "rows >= 0, 0 <= stride_in <= 2^31 - 1, stride_out >= 0");
  if (rows == 0 || stride_out == 0) return AINP_OK;
  if (!y || !n_in || (!x && stride_in > 0) || (!table && p.route != AINP_RS_COPY))
    return record_bad_argument("ainp_resample_poly");
  hipStream_t s = as_stream(stream);
  if (dtype == 0)
    return resample_launch<float>(y, x, table, rows, stride_in, stride_out, n_in, p, s);
  return resample_launch<double>(y, x, table, rows, stride_in, stride_out, n_in, p, s);
}
