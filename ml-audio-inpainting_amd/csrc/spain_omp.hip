// spain_omp.hip — S-SPAIN with the OMP coefficient update, one window per
// workgroup (references/spain/sspain.m with f_update = 'OMP', driven by
// spain_segmentation.m; restated in DESIGN §14.3).  All arithmetic float64.
//
// The loop is spain.hip's S-SPAIN with z-bar = OMP_k(x-hat - u) in place of
// H_k(A (x-hat - u)); frame, objective, record, stop, projection, dual update
// and k schedule are the same; record, schedule, the row rule, load and closing
// are the same code (spain_window.h), and so are the transforms,
// the slots and the fixed-order sum (spain_fft.h).  OMP_k(v) is greedy least
// squares over the atoms d_m[i] = exp(2 pi i m i / M) / sqrt(M), i < w: while
// the residual is above tol = 10^(errdb / 20) |v| and fewer than k atoms are
// chosen, take the unselected half-spectrum bin with the largest |(A r)_m|
// (plain magnitudes, ties to the lower bin) and solve min |v - A* z| over
// conjugate-symmetric z on the chosen bins and their mirrors.
//
// The least squares runs in coefficient space over real columns: an atom m
// other than DC and Nyquist brings R_m = 2 Re d_m and I_m = -2 Im d_m with the
// unknowns (Re z_m, Im z_m); DC and Nyquist bring d_m itself (= R_m / 2) with
// one real unknown.
//   * right-hand side: <R_m, v> = 2 Re (A v)_m, <I_m, v> = 2 Im (A v)_m.  A v is
//     the first inner iteration's spectrum and stays in registers.
//   * Gram entries are values of the Dirichlet kernel g[d] = (1/M) sum_{i<w}
//     exp(2 pi i d i / M) = exp(i pi d (w-1) / M) sin(pi d / red) / (M sin(pi d /
//     M)), from sinpi / sincospi with exact arguments:
//       <R_p, R_q> = 2 Re g[p+q] + 2 Re g[p-q]   <R_p, I_q> = 2 Im g[p-q] - 2 Im g[p+q]
//       <I_p, I_q> = 2 Re g[p-q] - 2 Re g[p+q]   <I_p, R_q> = -2 Im g[p-q] - 2 Im g[p+q]
//   * G = L L^T of the chosen columns is kept as T = L^-1, packed lower
//     triangular in the row's global workspace.  Appending a column with Gram
//     vector a and squared norm alpha: l = T a (one wave per row of T),
//     lambda^2 = alpha - |l|^2 (the pivot: the column's squared norm orthogonal
//     to the chosen ones), new row of T = [-(l^T T) / lambda, 1 / lambda] (one
//     lane per column of T), y = (new row) . b, and the solution moves by
//     z += y (new row): two matrix-vector products per column and no
//     triangular solve.
//   * the residual is formed in place in the transform buffer from the inverse
//     transform of the sparse z: a lane rebuilds x-hat - u for its own samples.
//
// LDS beyond spain.hip's (transform, iterate, quarter wave): four vectors of
// D = min(w, 512) doubles (z, b, a, l), D column codes and the atom list; at
// w 4096, red 2: 117 KiB + 16 KiB + 4 KiB of the 160 KiB.  Every sum is in a
// fixed order (per lane in index order, a butterfly over the wave, waves in
// order), the argmax orders (magnitude, bin) totally: the same bits on every
// call and every lane takes the same branch.  No float atomics, no spin
// barriers.
#include <algorithm>
#include <cmath>

#include "spain_window.h"

namespace ainp {

constexpr double SO_PIVOT = 1e-10;  // smallest relative squared pivot of a new column

enum { SO_R = 0, SO_I = 1, SO_S = 2 };   // 2 Re d_m, -2 Im d_m, d_m (DC, Nyquist)

static size_t so_tsize(int w) {   // doubles of a row's packed T
  const size_t d = (size_t)sp_omp_dims(w);
  return d * (d + 1) / 2;
}

// g[d] of the header, any integer d
__device__ __forceinline__ cplx so_g(int d, int w, int M, int red) {
  const int dd = d & (M - 1);
  if (dd == 0) return {(double)w / (double)M, 0.0};
  const double s1 = sinpi((double)(dd % (2 * red)) / (double)red);
  const double s2 = sinpi((double)dd / (double)M);
  double sn, cs;
  sincospi((double)(((int64_t)dd * (w - 1)) % (2 * M)) / (double)M, &sn, &cs);
  const double q = s1 / (s2 * (double)M);
  return {cs * q, sn * q};
}

// <column (p, kp), column (q, kq)>; a column code is 4 m + kind
__device__ __forceinline__ double so_gram(int cp, int cq, int w, int M, int red) {
  const int p = cp >> 2, kp = cp & 3, q = cq >> 2, kq = cq & 3;
  const cplx gp = so_g(p + q, w, M, red), gm = so_g(p - q, w, M, red);
  double v;
  if (kp != SO_I && kq != SO_I) v = 2.0 * (gp.re + gm.re);
  else if (kp != SO_I) v = 2.0 * (gm.im - gp.im);
  else if (kq != SO_I) v = -2.0 * (gm.im + gp.im);
  else v = 2.0 * (gm.re - gp.re);
  if (kp == SO_S) v *= 0.5;
  if (kq == SO_S) v *= 0.5;
  return v;
}

// half-spectrum bin m -> the slot p that holds it and which part: 0 a, 1 b,
// 2 the real part of slot 0's a (DC), 3 its imaginary part (Nyquist)
__device__ __forceinline__ void so_slot(int m, int N, int& p, int& which) {
  if (m == 0) { p = 0; which = 2; }
  else if (m == N) { p = 0; which = 3; }
  else if (m == N / 2) { p = 0; which = 1; }
  else if (m < N / 2) { p = m; which = 0; }
  else { p = N - m; which = 1; }
}
__device__ __forceinline__ unsigned so_bit(int e, int which) {
  return which == 3 ? (1u << 30) : (1u << (2 * e + (which == 1 ? 1 : 0)));
}

struct SoLs {
  double* zc;   // the solution, one entry per real column
  double* bv;   // <column, v>
  double* av;   // Gram vector of the column being appended
  double* lv;   // T a
  int* code;    // 4 m + kind per column
  double* T;    // the row's packed L^-1 (global)
  double* part;
  double* ynew;
  int w, M, red;
};

// Append column `n` (code[n], bv[n] are set).  False, with nothing committed,
// if its relative squared pivot is under SO_PIVOT.  Ends on a barrier.
template <int NT>
__device__ bool so_append(const SoLs& q, int n, int slot, int tid) {
  const int cn = q.code[n];
  for (int i = tid; i < n; i += NT) q.av[i] = so_gram(q.code[i], cn, q.w, q.M, q.red);
  const double alpha = so_gram(cn, cn, q.w, q.M, q.red);
  __syncthreads();
  const int lane = tid & 63;
  for (int j = tid >> 6; j < n; j += NT / 64) {
    const double* Tj = q.T + (size_t)j * (j + 1) / 2;
    double acc = 0.0;
    for (int i = lane; i <= j; i += 64) acc += Tj[i] * q.av[i];
    acc = wave_sum_d(acc);
    if (lane == 0) q.lv[j] = acc;
  }
  __syncthreads();
  double acc = 0.0;
  for (int j = tid; j < n; j += NT) acc += q.lv[j] * q.lv[j];
  const double piv = alpha - sp_sum<NT>(acc, q.part, tid);
  if (!(piv >= SO_PIVOT * alpha)) return false;
  const double li = 1.0 / sqrt(piv);
  double* Tn = q.T + (size_t)n * (n + 1) / 2;
  acc = 0.0;
  for (int i = tid; i < n; i += NT) {
    double t = 0.0;
#pragma unroll 4
    for (int j = i; j < n; ++j) t += q.lv[j] * q.T[(size_t)j * (j + 1) / 2 + i];
    t *= -li;
    Tn[i] = t;
    acc += t * q.bv[i];
  }
  if (tid == 0) {
    Tn[n] = li;
    acc += li * q.bv[n];
  }
  const double y = sp_sum<NT>(acc, q.part, tid);
  if (tid == 0) q.ynew[slot] = y;
  __syncthreads();
  return true;
}

// grid: one workgroup of NT lanes per row.  dynamic LDS: SoLds.
template <int NT, int EPL>
__global__ __launch_bounds__(NT) void spain_omp_kernel(
    double* sol, int64_t stride, const int32_t* __restrict__ gap_start,
    const int32_t* __restrict__ gap_len, int w, int M, int lgN, int red, int s_step, int r_rate,
    double epsilon, int maxit, double tolfac, int32_t* __restrict__ iters,
    double* __restrict__ obj_history, int32_t* __restrict__ n_atoms, double* T_all,
    int64_t tsize, int nF, int nRow, int nCos, int nD, int nA) {
  constexpr int SP_TPL = 2 * EPL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double part[NT / 64];
  __shared__ double pkey[NT / 64];
  __shared__ int pbin[NT / 64];
  __shared__ double ynew[2];
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nF;
  double* xr = im + nF;
  double* ct = xr + nRow;
  SoLs q;
  q.zc = ct + nCos;
  q.bv = q.zc + nD;
  q.av = q.bv + nD;
  q.lv = q.av + nD;
  q.code = reinterpret_cast<int*>(q.lv + nD);
  int* atm = q.code + nD;   // the chosen bins, in order
  int* ato = atm + nA;      // an atom's first column
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  q.T = T_all + row * tsize;
  q.part = part;
  q.ynew = ynew;
  q.w = w;
  q.M = M;
  q.red = red;
  const int N = M / 2;
  const int gs = gap_start[row], gl = gap_len[row];
  double* hrow = obj_history ? obj_history + row * maxit : nullptr;
  int32_t* arow = n_atoms ? n_atoms + row * maxit : nullptr;
  if (!sp_run_ok(gs, gl, w)) {
    sp_row_close<NT>(iters, hrow, arow, 0, maxit, tid);
    return;
  }
  const SpRow R = {xr, sol + row * stride, hrow, arow, gs, gl};
  sp_row_load<NT>(R, ct, w, M, tid);

  const SpFft f = {re, im, ct, N, lgN, M};
  const double fwd = 1.0 / sqrt((double)M);   // analysis: FFT_M / sqrt(M)
  const double inv = 2.0 / sqrt((double)M);   // synthesis: (N-point sum) sqrt(M) / N
  const cplx zero = {0.0, 0.0};
  double ut[SP_TPL][2];   // u
#pragma unroll
  for (int e = 0; e < SP_TPL; ++e) ut[e][0] = ut[e][1] = 0.0;

  int n = 0, na = 0;   // real columns, atoms of the running OMP
  // the sparse z of the chosen atoms -> a lane's slots -> the transform buffer
  auto synthesise = [&]() {
    SpSpec<EPL> Z;
#pragma unroll
    for (int e = 0; e < EPL; ++e) Z.a[e] = Z.b[e] = zero;
    for (int j = 0; j < na; ++j) {
      int p, which;
      so_slot(atm[j], N, p, which);
      if ((p & (NT - 1)) != tid) continue;
      const int e0 = p / NT, off = ato[j];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        if (e != e0) continue;
        if (which == 0) Z.a[e] = {q.zc[off], q.zc[off + 1]};
        else if (which == 1) Z.b[e] = {q.zc[off], q.zc[off + 1]};
        else if (which == 2) Z.a[e].re = q.zc[off];
        else Z.a[e].im = q.zc[off];
      }
    }
    sp_merge<NT, EPL>(f, tid, Z);
    __syncthreads();
    sp_dit<NT>(f, tid);
  };

  double best = INFINITY;
  int k = s_step, cnt = 1, done = 0;
  while (cnt <= maxit) {
    // ---- z-bar = OMP_k(v), v = x-hat - u: the buffer holds r = v, zero-padded
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < SP_TPL; ++e) {
      const int t = tid + e * NT;
      if (t >= N) continue;
      cplx c = zero;
      if (2 * t < w) {
        c = {xr[2 * t] - ut[e][0], xr[2 * t + 1] - ut[e][1]};
        acc += c.re * c.re + c.im * c.im;
      }
      f.st(t, c);
    }
    double rn2 = sp_sum<NT>(acc, part, tid);   // its barriers publish the buffer
    const double tol = tolfac * sqrt(rn2);
    SpSpec<EPL> CV;   // A v
    unsigned chosen = 0;
    n = 0;
    na = 0;
    for (;;) {
      if (sqrt(rn2) <= tol) break;   // (a) the residual
      if (na == k) break;            // (b) the count
      SpSpec<EPL> CR;                // A r
      sp_dif<NT>(f, tid);
      sp_split<NT, EPL>(f, tid, fwd, CR);
      if (na == 0) CV = CR;
      // (c) the unselected bin with the largest magnitude, ties to the lower bin
      double bk = -1.0;
      int bm = 0x7fffffff;
      auto offer = [&](double key, int m, unsigned bit) {
        if (!(chosen & bit) && (key > bk || (key == bk && m < bm))) {
          bk = key;
          bm = m;
        }
      };
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int p = tid + e * NT;
        if (p >= N / 2) continue;
        if (p == 0) {
          offer(CR.a[e].re * CR.a[e].re, 0, so_bit(e, 2));
          offer(cabs2(CR.b[e]), N / 2, so_bit(e, 1));
          offer(CR.a[e].im * CR.a[e].im, N, so_bit(e, 3));
        } else {
          offer(cabs2(CR.a[e]), p, so_bit(e, 0));
          offer(cabs2(CR.b[e]), N - p, so_bit(e, 1));
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ok = __shfl_xor(bk, o, 64);
        const int om = __shfl_xor(bm, o, 64);
        if (ok > bk || (ok == bk && om < bm)) {
          bk = ok;
          bm = om;
        }
      }
      if ((tid & 63) == 0) {
        pkey[tid >> 6] = bk;
        pbin[tid >> 6] = bm;
      }
      __syncthreads();   // also: the split's reads are done
      bk = pkey[0];
      bm = pbin[0];
#pragma unroll
      for (int wv = 1; wv < NT / 64; ++wv)
        if (pkey[wv] > bk || (pkey[wv] == bk && pbin[wv] < bm)) {
          bk = pkey[wv];
          bm = pbin[wv];
        }
      if (bk < 0.0) break;   // every bin is chosen
      // (d) the dimension
      const bool single = bm == 0 || bm == N;
      const int nc = single ? 1 : 2;
      if (n + nc > w) break;
      int p, which;
      so_slot(bm, N, p, which);
      const bool mine = (p & (NT - 1)) == tid;
      const int e0 = p / NT;
      if (mine) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          if (e != e0) continue;
          if (which == 2) q.bv[n] = CV.a[e].re;
          else if (which == 3) q.bv[n] = CV.a[e].im;
          else {
            const cplx c = which == 0 ? CV.a[e] : CV.b[e];
            q.bv[n] = 2.0 * c.re;
            q.bv[n + 1] = 2.0 * c.im;
          }
        }
        q.code[n] = 4 * bm + (single ? SO_S : SO_R);
        if (!single) q.code[n + 1] = 4 * bm + SO_I;
      }
      __syncthreads();
      // (e) the pivots, (f) the least squares
      if (!so_append<NT>(q, n, 0, tid)) break;
      if (!single && !so_append<NT>(q, n + 1, 1, tid)) break;
      for (int i = tid; i < n + nc; i += NT) {
        double z = i < n ? q.zc[i] : 0.0;
        if (i <= n) z += ynew[0] * q.T[(size_t)n * (n + 1) / 2 + i];
        if (!single) z += ynew[1] * q.T[(size_t)(n + 1) * (n + 2) / 2 + i];
        q.zc[i] = z;
      }
      if (tid == 0) {
        atm[na] = bm;
        ato[na] = n;
      }
      if (mine) chosen |= so_bit(e0, which);
      n += nc;
      ++na;
      __syncthreads();
      // r = v - A* z in place, a lane on its own sample pairs
      synthesise();
      acc = 0.0;
#pragma unroll
      for (int e = 0; e < SP_TPL; ++e) {
        const int t = tid + e * NT;
        if (t >= N) continue;
        cplx c = zero;
        if (2 * t < w) {
          const cplx y = f.ld(t);
          c = {xr[2 * t] - ut[e][0] - y.re * inv, xr[2 * t + 1] - ut[e][1] - y.im * inv};
          acc += c.re * c.re + c.im * c.im;
        }
        f.st(t, c);
      }
      rn2 = sp_sum<NT>(acc, part, tid);
    }
    __syncthreads();

    // ---- obj = |A* z-bar - x-hat|
    synthesise();
    acc = 0.0;
#pragma unroll
    for (int e = 0; e < SP_TPL; ++e) {
      const int t = tid + e * NT;
      if (t >= N || 2 * t >= w) continue;
      const cplx c = f.ld(t);
      const double d0 = c.re * inv - xr[2 * t], d1 = c.im * inv - xr[2 * t + 1];
      acc += d0 * d0 + d1 * d1;
    }
    const double obj = sqrt(sp_sum<NT>(acc, part, tid));
    done = cnt;
    if (sp_record<NT>(R, obj, cnt, na, best, epsilon, tid)) break;
    __syncthreads();   // the record has read the row
    // x-hat = proj(x_e + u);  u += x_e - x-hat, a lane on its own sample pairs
#pragma unroll
    for (int e = 0; e < SP_TPL; ++e) {
      const int t = tid + e * NT;
      if (t >= N || 2 * t >= w) continue;
      const cplx c = f.ld(t);
      const double xe[2] = {c.re * inv, c.im * inv};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = 2 * t + h;
        if (i >= gs && i - gs < gl) xr[i] = xe[h] + ut[e][h];
        ut[e][h] += xe[h] - xr[i];
      }
    }
    __syncthreads();
    sp_next_pass(cnt, k, s_step, r_rate);
  }
  sp_row_close<NT>(iters, hrow, arow, done, maxit, tid);
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_spain_omp_workspace(int64_t n_rows, int w, int red) {
  if (n_rows < 0 || !sp_shape_ok(w, red)) return 0;
  return (size_t)n_rows * so_tsize(w) * sizeof(double);
}

extern "C" int ainp_spain_omp(double* sol, int64_t n_rows, int64_t stride,
                              const int32_t* gap_start, const int32_t* gap_len, int w, int red,
                              int s, int r, double epsilon, int maxit, double errdb,
                              int32_t* iters, double* obj_history, int32_t* n_atoms,
                              void* workspace, size_t ws_bytes, void* stream) {
  const char* fn = "ainp_spain_omp";
  if (int rc = sp_check_window_args(fn, sol && gap_start && gap_len && iters, n_rows, stride, w, red,
                                    true, s, r, epsilon, maxit))
    return rc;
  if (!(errdb >= -300.0 && errdb <= 0.0)) return record_bad_argument(fn, "-300 <= errdb <= 0");
  // the largest k of the schedule: k(cnt) = s (1 + cnt / r - 1 / r)
  const int64_t kmax = (int64_t)s * (1 + maxit / r - 1 / r);
  if (std::min<int64_t>(2 * kmax, w) > AINP_SPAIN_OMP_DIMS)
    return record_bad_argument(fn, "min(2 k(maxit), w) <= 512 real unknowns, "
                               "k(maxit) = s (1 + maxit / r - 1 / r)");
  if (n_rows > 0x7fffffff) return record_msg("ainp_spain_omp: too many rows");
  if (ws_bytes < ainp_spain_omp_workspace(n_rows, w, red) || (n_rows && !workspace))
    return record_msg("ainp_spain_omp: workspace too small");
  if (n_rows == 0) return AINP_OK;
  const int M = red * w;
  const SpLds l = sp_window_lds(w, M, true);
  const double tolfac = pow(10.0, errdb / 20.0);
#define SO_GO(NT, EPL)                                                                          \
  return sp_launch_rows<spain_omp_kernel<NT, EPL>, NT>(                                         \
      fn, sp_window_lds(SP_WMAX, SP_MMAX, true).bytes(), l.bytes(), n_rows, stream, sol,        \
      stride, gap_start, gap_len, w, M, sp_lgN(M), red, s, r, epsilon, maxit, tolfac, iters,    \
      obj_history, n_atoms, static_cast<double*>(workspace), (int64_t)so_tsize(w), l.nF,        \
      l.nRow, l.nCos, l.nD, l.nA)
  if (sp_lanes_256(M)) SO_GO(256, 2);
  SO_GO(SP_NT_BIG, SP_EPL_BIG);
#undef SO_GO
}
