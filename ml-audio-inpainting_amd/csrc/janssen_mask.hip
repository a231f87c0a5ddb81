// janssen_mask.hip — gap-wise Janssen autoregressive inpainting for any set of
// missing samples in a segment (models/AudioReg/utils/janssen_inp.m takes any
// NaN pattern; janssen.hip covers one contiguous run).  All arithmetic float64.
//
// One workgroup owns one segment for all maxit iterations, as in janssen.hip,
// and steps 1 to 3 of an iteration are that kernel's (ar_fit.h): the AR
// coefficients a of the current solution ("lpc" or "arburg"), then b[0..p], the
// autocorrelation of a.  With the sorted missing set M_0 < ... < M_{h-1}:
//   4. g_i = -sum_{n observed, |M_i - n| <= p} b[|M_i - n|] x_n.  xo, the segment
//      with its missing samples zeroed, is made once per launch in the
//      workspace, so a row is two dots over b[1..p] with no mask test.
//   5. G z = g, G[i][j] = b[|M_i - M_j|] where the distance is <= p, else 0.
//      G is not Toeplitz, so this is a Cholesky factorisation G = L L^T.
//      first(i) = the smallest j with M_i - M_j <= p is non-decreasing in i and
//      i - first(i) <= bw = min(h_max - 1, p): L keeps G's envelope, and it is
//      stored by columns as a band, Lc[k][i - k], i - k <= bw, in the workspace.
//      Left-looking over block columns of 8: G is never materialised.  For
//      the block column at c0 the panel is the rows c0 .. rend, rend = the first
//      row with first(i) beyond the block.  A lane owns up to R panel rows and
//      keeps their 8 entries in registers: G's entries from b and the index
//      list, minus sum_k L[i][k] L[c][k] over k in [max(first(c0), first(i)),
//      c0) -- rows c0 .. c0 + 7 of L staged through LDS in chunks of JM_KC
//      columns (k-major, read as broadcasts), L[i][k] read from the band with
//      consecutive lanes on consecutive addresses.  A wave starts at the first
//      k of its first row and skips the R slices whose rows lie beyond rend:
//      tiles outside the band cost nothing.  The 8 x 8 diagonal tile goes
//      through LDS into the lanes of every wave (lane l: row l & 7) and is
//      factored there, row-parallel, the pivot column fetched by v_readlane;
//      every wave computes the same bits, so no result has to be published.
//      The rows below the tile are solved against it in registers (its entries
//      by v_readlane again), and the forward substitution L y = g rides along
//      (right-looking: y of the block, lane-parallel, then g_i -= sum_c
//      L[i][c] y_c for the lane's rows).  L^T z = y runs over the blocks
//      backwards in the same way, lane l holding column l of the tile.  Plain
//      fused multiply-adds in a fixed order throughout, one order per element:
//      the same bits on every call.  A short last block is padded with the
//      identity.
//      Tiles of 8, not 16, and scalar FMAs, not v_mfma_f64_16x16x4_f64: the
//      unrolled triangular solves of a 16-tile keep 136 entries in scalar
//      registers and the kernel spilled beside burg_fit's 245 VGPRs, whereas
//      this form leaves no scratch with either estimator.
//   6. sol[M] = z (and history), unless a pivot was not positive and finite or
//      a z not finite: then the segment stops and the previous iterate stays
//      (the reference's chol break).
//
// LDS (doubles): B[nB] (r, then b; zero beyond p) | A[nB] (a, then y) | Y[nY]
// (g) | W[S] (signal chunks of the lag sums, then the staged rows of L, then
// z) | arburg only: XY, burg_fit's exchange | then int32: M[nY] | first[nY] |
// then the diagonal tile, 8 x 8 doubles.
// Workspace per segment (doubles): xo[n_max rounded up to even] |
// Lc[h_max * (bw + 1)].
#include <algorithm>
#include <climits>

#include "ar_fit.h"

namespace ainp {

constexpr int JM_TILE = 8;
constexpr int JM_KC = 256;   // columns of L staged per chunk

struct JmPlan {
  int nB, nY, S, nX;   // doubles
  int bw;              // index bandwidth of L
  int64_t n_pad;       // xo
  size_t lds() const {
    return ((size_t)2 * nB + nY + S + nX + JM_TILE * JM_TILE) * sizeof(double) +
           (size_t)2 * nY * sizeof(int32_t);
  }
  int64_t seg_doubles() const { return n_pad + (int64_t)nY * (bw + 1); }
};

// n_max: the longest segment the stride allows; h_max: the longest list
static JmPlan jm_plan(int64_t n_max, int p, int h_max, int method) {
  JmPlan l;
  l.nB = (std::max(p, h_max) + 3) & ~1;
  l.nY = (h_max + 1) & ~1;
  const int64_t want = std::max<int64_t>(2 * (int64_t)p, (int64_t)p + 1024);
  l.S = (int)std::max<int64_t>(JM_KC * JM_TILE, std::min<int64_t>(n_max, want));
  l.S = (l.S + 1) & ~1;
  l.nX = method == AINP_AR_BURG ? BG_XY : 0;
  l.bw = std::min(h_max - 1, p);
  l.n_pad = (n_max + 1) & ~(int64_t)1;
  return l;
}

// acc[r][c] -= L[i_r][k] * T[k][c] for k in [kbeg, kend), the first NR of the
// lane's rows; col(k)[i] = Lc + k * (LW - 1) + i is L[i][k]
template <int NR, int R>
__device__ __forceinline__ void jm_accumulate(double (&acc)[R][JM_TILE], const double* Lc,
                                              int lw1, const int (&irow)[R], const int (&ks)[R],
                                              const double* T, int kc, int kbeg, int kend) {
#pragma unroll 2
  for (int k = kbeg; k < kend; ++k) {
    const double* tk = T + (k - kc) * JM_TILE;
    const double* col = Lc + k * lw1;
    double lv[NR], t[JM_TILE];
#pragma unroll
    for (int r = 0; r < NR; ++r) lv[r] = k >= ks[r] ? -col[irow[r]] : 0.0;
#pragma unroll
    for (int c = 0; c < JM_TILE; ++c) t[c] = tk[c];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int c = 0; c < JM_TILE; ++c) acc[r][c] = fma(lv[r], t[c], acc[r][c]);
  }
}

// grid: one workgroup of NT lanes per segment.  dynamic LDS: JmPlan::lds().
template <int NT, int METHOD>
__global__ __launch_bounds__(NT) void janssen_mask_kernel(
    double* sol, int64_t stride, const int32_t* __restrict__ n_,
    const int32_t* __restrict__ miss_off, const int32_t* __restrict__ miss_idx, int h_max, int p,
    int maxit, double* __restrict__ history, int64_t hist_row, int32_t* __restrict__ iters_done,
    double* ws, int64_t seg_doubles, int64_t n_pad, int bw, int nB, int nY, int S, int nX) {
  static_assert(METHOD == AINP_AR_LPC || NT == BG_THREADS, "burg_fit needs its 512 lanes");
  constexpr int NW = NT / 64;
  // panel rows per lane and per pass.  The Burg fit leaves a lane 11 of its 256
  // registers (ar_fit.h), and what this loop keeps across it has to fit there
  constexpr int R = METHOD == AINP_AR_BURG ? 2 : 4, ROWS = NT * R;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double part[2][2][NW];
  __shared__ int s_bad;
  double* B = reinterpret_cast<double*>(smem);
  double* A = B + nB;
  double* Y = A + nB;
  double* W = Y + nY;
  int32_t* M = reinterpret_cast<int32_t*>(W + S + nX);
  int32_t* first = M + nY;
  double* D = reinterpret_cast<double*>(first + nY);   // the diagonal tile
  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x;

  // a segment the tables describe outside the supported range is left alone
  const int N = n_[seg], o0 = miss_off[seg], o1 = miss_off[seg + 1];
  const int64_t hl = (int64_t)o1 - o0;
  if (N <= p || N > JN_NMAX || (int64_t)N > stride || o0 < 0 || hl < 0 || hl > h_max ||
      hl > nY) {
    if (tid == 0) iters_done[seg] = -1;
    return;
  }
  const int h = (int)hl;
  if (h == 0) {
    if (tid == 0) iters_done[seg] = 0;
    return;
  }
  if (tid == 0) s_bad = 0;
  for (int j = tid; j < h; j += NT) M[j] = miss_idx[o0 + j];
  __syncthreads();
  for (int j = tid; j < h; j += NT) {
    const int m = M[j];
    if (m < 0 || m >= N || (j > 0 && m <= M[j - 1])) s_bad = 1;
  }
  __syncthreads();
  if (s_bad) {   // out of order or out of the row
    if (tid == 0) iters_done[seg] = -1;
    return;
  }

  double* x = sol + seg * stride;
  double* xo = ws + seg * seg_doubles;
  double* Lc = xo + n_pad;
  const int lw1 = bw;   // L[i][k] is Lc[k (bw + 1) + i - k]
  for (int i = tid; i < N; i += NT) xo[i] = x[i];
  for (int k = p + 1 + tid; k < nB; k += NT) B[k] = 0.0;   // stays zero
  for (int j = tid; j < h; j += NT) {
    // first(j): the lower bound of M_j - p in M
    const int want = M[j] - p;
    int lo = 0, hi = j;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (M[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    first[j] = lo;
  }
  __syncthreads();
  for (int j = tid; j < h; j += NT) {
    xo[M[j]] = 0.0;
    x[M[j]] = 0.0;
  }
  __syncthreads();

  const int C = N <= S ? N : S - p;
  int it = 0;   // on leaving the loop: the iterations completed
  for (; it < maxit; ++it) {
    // the sizes are opaque per iteration: what the compiler hoists out of this
    // loop stays live across the fit and the solve, and that spilled.  (burg_fit
    // takes N and p themselves, as in janssen.hip: its 33 bounds tests per lane
    // are then made once, ahead of the loop, and kept as scalar masks.)
    int Nq = N, pq = p, hq = h;
    asm volatile("" : "+s"(Nq), "+s"(pq), "+s"(hq));
    if (tid == 0) s_bad = 0;
    if constexpr (METHOD == AINP_AR_LPC) {
      // 1. autocorrelation of the current solution
      for (int k = tid; k <= pq; k += NT) B[k] = 0.0;
      if (tid == 0) A[0] = 1.0;
      for (int c0 = 0; c0 < Nq; c0 += C) {
        const int L = min(S, Nq - c0);
        __syncthreads();   // the previous chunk (or z) is no longer read
        for (int i = tid; i < L; i += NT) W[i] = x[c0 + i];
        __syncthreads();
        jn_lags<NT>(W, L, min(C, Nq - c0), pq, B);
      }
      __syncthreads();
      const double r0 = B[0];
      if (!(r0 > 0.0) || !isfinite(r0)) break;   // silent (or unusable) context

      // 2. AR coefficients
      if (!jn_levinson<false, NT>(B, pq, A, nullptr, nullptr, part)) break;
    } else {
      // 1 + 2. AR coefficients by Burg's estimator
      if (!burg_fit<1>(x, 0.0, N, p, A, W + S, part)) break;
    }
    __syncthreads();

    // 3. their autocorrelation, over r
    for (int k = tid; k <= pq; k += NT) B[k] = 0.0;
    __syncthreads();
    jn_lags<NT>(A, pq + 1, pq + 1, pq, B);
    __syncthreads();

    // 4. right-hand side: xo is zero on the missing samples
    for (int ii = tid; ii < hq; ii += NT) {
      const int m = M[ii];
      const int cl = min(pq, m), cr = min(pq, Nq - 1 - m);
      double acc = 0.0;
      if (cl > 0) acc = jn_dot<-1>(B + 1, xo + m - 1, cl);
      if (cr > 0) acc += jn_dot<1>(B + 1, xo + m + 1, cr);
      Y[ii] = -acc;
    }

    // 5. G = L L^T by block columns, L y = g alongside (y into A)
    bool ok = true;
    // the tile (lane l: row l mod 8) and y of the block; set here, so that no
    // value of the iteration before is carried across the fit
    double tl[JM_TILE] = {}, yv[JM_TILE] = {}, dinv = 0.0;
    for (int c0 = 0; c0 < hq && ok; c0 += JM_TILE) {
      // (opaque per block column: the compares of the lane's index with the
      // tile's rows and columns are not kept as 30 scalar pairs across the loop)
      int tb = tid;
      asm volatile("" : "+v"(tb));
      const int wb = tb >> 6;
      const int nb = min(JM_TILE, hq - c0);
      const int k0 = first[c0];
      int rend;
      {
        // the panel ends at the first row whose band starts beyond the block
        const int reach = M[c0 + nb - 1] + pq;
        int lo = c0 + nb, hi = hq;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (M[mid] <= reach) lo = mid + 1;
          else hi = mid;
        }
        rend = lo;
      }
      int mc[JM_TILE];
#pragma unroll
      for (int c = 0; c < JM_TILE; ++c) mc[c] = c < nb ? M[c0 + c] : INT_MIN / 2;
      for (int rb = c0; rb < rend; rb += ROWS) {
        double acc[R][JM_TILE];
        int irow[R], ks[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = rb + tb + r * NT;
          const bool live = i < rend;
          irow[r] = live ? i : c0;
          // (a row beyond the panel takes no k; what it holds is never stored)
          ks[r] = live ? max(k0, first[i]) : c0;
          const int mi = M[min(i, hq - 1)];
#pragma unroll
          for (int c = 0; c < JM_TILE; ++c) {
            const int d = abs(mi - mc[c]);
            acc[r][c] = d <= pq ? B[d] : 0.0;
          }
        }
        // the wave's slices that hold a row of the panel, and its first k
        const int w0 = rb + wb * 64;
        int nr = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) nr += w0 + r * NT < rend;
        const int wk = nr ? first[w0] : INT_MAX;
        for (int kc = k0; kc < c0; kc += JM_KC) {
          const int kn = min(JM_KC, c0 - kc);
          __syncthreads();   // the chunk before (or the lag sums' W) is no longer read
          for (int e = tb; e < kn * JM_TILE; e += NT) {
            const int kk = kc + e / JM_TILE, cc = c0 + e % JM_TILE;
            W[e] = cc < hq && kk >= first[cc] ? Lc[kk * lw1 + cc] : 0.0;
          }
          __syncthreads();
          const int kbeg = max(kc, wk), kend = kc + kn;
          if (nr == 1) jm_accumulate<1, R>(acc, Lc, lw1, irow, ks, W, kc, kbeg, kend);
          if constexpr (R >= 2)
            if (nr == 2) jm_accumulate<2, R>(acc, Lc, lw1, irow, ks, W, kc, kbeg, kend);
          if constexpr (R >= 3)
            if (nr == 3) jm_accumulate<3, R>(acc, Lc, lw1, irow, ks, W, kc, kbeg, kend);
          if constexpr (R >= 4)
            if (nr == 4) jm_accumulate<4, R>(acc, Lc, lw1, irow, ks, W, kc, kbeg, kend);
        }
        if (rb == c0) {
          // (opaque once more: this block's compares and addresses are not
          // computed ahead of the pass loop and kept through it)
          int tf = tb;
          asm volatile("" : "+v"(tf));
          const int lf = tf & (JM_TILE - 1);
          // the diagonal tile: into every wave's lanes, factored there
          __syncthreads();   // D of the block before is no longer read
          // (wave 0 alone, in program order: the identity, then the rows there are)
          if (tf < JM_TILE * JM_TILE) D[tf] = tf / JM_TILE == tf % JM_TILE ? 1.0 : 0.0;
          if (tf < nb) {
#pragma unroll
            for (int c = 0; c < JM_TILE; ++c) D[tf * JM_TILE + c] = acc[0][c];
          }
          __syncthreads();
#pragma unroll
          for (int c = 0; c < JM_TILE; ++c) tl[c] = D[lf * JM_TILE + c];
#pragma unroll
          for (int j = 0; j < JM_TILE; ++j) {
            const double piv = jn_readlane(tl[j], j);
            ok = ok && piv > 0.0 && isfinite(piv);
            const double d = sqrt(piv), inv = 1.0 / d;
            const double lij = lf == j ? d : tl[j] * inv;
            if (lf == j) dinv = inv;
            tl[j] = lij;
#pragma unroll
            for (int c = j + 1; c < JM_TILE; ++c)
              tl[c] = fma(-lij, jn_readlane(lij, c), tl[c]);
          }
          if (!ok) break;   // every lane alike: all waves factored the same tile
          if (tf < nb) {
#pragma unroll
            for (int c = 0; c < JM_TILE; ++c)
              if (c <= tf && tf - c <= bw) Lc[(c0 + c) * lw1 + c0 + tf] = tl[c];   // (p < 7)
          }
          // y of the block, L_jj y = g: lane l holds g_l and takes y_m as it is final
          double gy = lf < nb ? Y[c0 + lf] : 0.0;
#pragma unroll
          for (int m = 0; m < JM_TILE; ++m) {
            yv[m] = jn_readlane(gy * dinv, m);
            gy = fma(-tl[m], yv[m], gy);
          }
          if (tf == 0) {
#pragma unroll
            for (int m = 0; m < JM_TILE; ++m)
              if (m < nb) A[c0 + m] = yv[m];
          }
        }
        // the rows below the tile: L[i][c0 ..] = acc L_jj^-T, in place.  The
        // tile's entries are fetched where they are used, one row per step:
        // fetched ahead (out of the pass loop, or all at once) they are 272
        // scalar registers, and those spilled
#pragma unroll
        for (int c = 0; c < JM_TILE; ++c) asm volatile("" : "+v"(tl[c]));
#pragma unroll
        for (int c = 0; c < JM_TILE; ++c) {
#pragma unroll
          for (int m = 0; m < c; ++m) {
            const double l = jn_readlane(tl[m], c);
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][c] = fma(-acc[r][m], l, acc[r][c]);
          }
          const double di = jn_readlane(dinv, c);
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r][c] *= di;
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = rb + tb + r * NT;
          if (i < c0 + JM_TILE || i >= rend) continue;
          double s = Y[i];
#pragma unroll
          for (int c = 0; c < JM_TILE; ++c) {
            // beyond the band the entry is zero and has no place
            if (c < nb && i - (c0 + c) <= bw) Lc[(c0 + c) * lw1 + i] = acc[r][c];
            s = fma(-acc[r][c], yv[c], s);
          }
          Y[i] = s;
        }
      }
    }
    __syncthreads();
    if (!ok) break;

    // L^T z = y over the blocks backwards (z into W)
    for (int c0 = ((hq - 1) / JM_TILE) * JM_TILE; c0 >= 0; c0 -= JM_TILE) {
      int tb = tid;
      asm volatile("" : "+v"(tb));
      const int lb = tb & (JM_TILE - 1);
      const int nb = min(JM_TILE, hq - c0);
      // lane l holds column l of the tile (contiguous in the band) and y_l
      double dg = 1.0;
#pragma unroll
      for (int m = 0; m < JM_TILE; ++m) {
        tl[m] = lb < nb && m < nb && m >= lb && m - lb <= bw ? Lc[(c0 + lb) * lw1 + c0 + m]
                                                             : (m == lb ? 1.0 : 0.0);
        if (m == lb) dg = tl[m];
      }
      dinv = 1.0 / dg;
      double gy = lb < nb ? A[c0 + lb] : 0.0;
#pragma unroll
      for (int m = JM_TILE - 1; m >= 0; --m) {
        yv[m] = jn_readlane(gy * dinv, m);
        gy = fma(-tl[m], yv[m], gy);
      }
      if (tb == 0) {
#pragma unroll
        for (int m = 0; m < JM_TILE; ++m)
          if (m < nb) W[c0 + m] = yv[m];
      }
      for (int k = first[c0] + tb; k < c0; k += NT) {
        double s = A[k];
#pragma unroll
        for (int c = 0; c < JM_TILE; ++c) {
          const int cc = c0 + c;
          if (c < nb && k >= first[cc]) s = fma(-Lc[k * lw1 + cc], yv[c], s);
        }
        A[k] = s;
      }
      __syncthreads();
    }
    for (int j = tid; j < hq; j += NT)
      if (!isfinite(W[j])) s_bad = 1;
    __syncthreads();
    if (s_bad) break;

    // 6. accept the iterate
    double* hist = history ? history + ((seg * maxit + it) * hist_row) : nullptr;
    for (int j = tid; j < hq; j += NT) {
      const double z = W[j];
      x[M[j]] = z;
      if (hist) hist[j] = z;
    }
    __syncthreads();
  }
  if (tid == 0) iters_done[seg] = it;
}

static int jm_unsupported(const char* msg) {
  record_msg(msg);
  return AINP_EUNSUPPORTED;
}

template <int NT, int METHOD>
static int jm_launch(const JmPlan& l, double* sol, int64_t n_segments, int64_t stride,
                     const int32_t* n, const int32_t* miss_off, const int32_t* miss_idx,
                     int h_max, int p, int maxit, double* history, int64_t hist_row,
                     int32_t* iters_done, void* workspace, void* stream) {
  static const bool lds_ok =
      hipFuncSetAttribute((const void*)janssen_mask_kernel<NT, METHOD>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)jm_plan(JN_NMAX, JN_PMAX, JN_HMAX, METHOD).lds()) == hipSuccess;
  if (!lds_ok) return record_msg("ainp_janssen_mask: cannot reserve the solver's LDS");
  hipLaunchKernelGGL((janssen_mask_kernel<NT, METHOD>), dim3((unsigned)n_segments), dim3(NT),
                     l.lds(), as_stream(stream), sol, stride, n, miss_off, miss_idx, h_max, p,
                     maxit, history, hist_row, iters_done, static_cast<double*>(workspace),
                     l.seg_doubles(), l.n_pad, l.bw, l.nB, l.nY, l.S, l.nX);
  return check_launch("ainp_janssen_mask");
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_janssen_mask_workspace(int64_t n_segments, int n_max, int p, int h_max,
                                              int method) {
  if (n_segments < 1 || n_max < 1 || p < 1 || h_max < 1) return 0;
  const JmPlan l = jm_plan(std::min(n_max, JN_NMAX), std::min(p, JN_PMAX),
                           std::min(h_max, JN_HMAX), method);
  return (size_t)n_segments * (size_t)l.seg_doubles() * sizeof(double);
}

extern "C" int ainp_janssen_mask(double* sol, int64_t n_segments, int64_t stride, const int32_t* n,
                                 const int32_t* miss_off, const int32_t* miss_idx, int h_max,
                                 int p, int maxit, int method, double* history, int64_t hist_row,
                                 int32_t* iters_done, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (!sol || !n || !miss_off || !miss_idx || !iters_done || n_segments < 0 || stride < 1)
    return record_msg("ainp_janssen_mask: bad argument");
  if (method != AINP_AR_LPC && method != AINP_AR_BURG)
    return record_msg("ainp_janssen_mask: bad argument (method is AINP_AR_LPC or AINP_AR_BURG)");
  if (p < 1 || maxit < 1 || h_max < 1)
    return record_msg("ainp_janssen_mask: bad argument (p >= 1, maxit >= 1, h_max >= 1)");
  if (p > JN_PMAX || maxit > JN_ITMAX || h_max > JN_HMAX)
    return jm_unsupported(
        "ainp_janssen_mask: unsupported (p <= 3072, maxit <= 1000, h_max <= 2048)");
  if (stride <= p) return record_msg("ainp_janssen_mask: bad argument (p < n <= stride)");
  if (history && hist_row < h_max)
    return record_msg("ainp_janssen_mask: bad argument (hist_row >= h_max)");
  if (n_segments > 0x7fffffff) return jm_unsupported("ainp_janssen_mask: too many segments");
  const int64_t n_max = std::min<int64_t>(stride, JN_NMAX);
  if (workspace_bytes < ainp_janssen_mask_workspace(n_segments, (int)n_max, p, h_max, method) ||
      (workspace_bytes && !workspace))
    return record_msg("ainp_janssen_mask: workspace too small");
  if (n_segments == 0) return AINP_OK;
  const JmPlan l = jm_plan(n_max, p, h_max, method);
  if (method == AINP_AR_BURG)
    return jm_launch<BG_THREADS, AINP_AR_BURG>(l, sol, n_segments, stride, n, miss_off, miss_idx,
                                               h_max, p, maxit, history, hist_row, iters_done,
                                               workspace, stream);
  return jm_launch<JN_THREADS, AINP_AR_LPC>(l, sol, n_segments, stride, n, miss_off, miss_idx,
                                            h_max, p, maxit, history, hist_row, iters_done,
                                            workspace, stream);
}
