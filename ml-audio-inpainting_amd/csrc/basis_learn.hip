// basis_learn.hip — learning the unitary sparsity-enhancing basis of SPAIN
// (references/basisopt/basis_opt_new.m; restated without CVX in DESIGN §14.4).
// All arithmetic float64.
//
// The convex subproblem of basis_opt_new.m:48-54,
//   min sum_im |Y + j 2 pi tridiag(d, e) Y|  s.t. |d_i| <= level, |e_i| <= level,
// is solved by a diagonally preconditioned primal-dual iteration to a relative
// duality gap; the update expm(j 2 pi A) is applied as a Taylor action, one
// band pass a term.  Y, lambda and sigma are [K][M_tr] with the training index
// contiguous.  An iteration is two launches and the launches are the barriers;
// there is no cooperative launch, no spin barrier and no float atomic:
//   bl_rows      one workgroup per row: rho_i = sum_m |Y_im|, fixed-order tree
//   bl_total     one workgroup: sum_i rho_i (the sparsity), lane 0 writes it
//   bl_reset     per solve: sigma_im, lambda = 0, (d, e) = (dbar, ebar) = 0, flags
//   bl_dual      lambda <- P_unit(lambda + sigma r(dbar, ebar)), one element a lane
//   bl_primal    one workgroup per row i: g_d[i], g_e[i] from rows i and i + 1 of
//                lambda and Y, then lane 0 steps, projects and extrapolates
//   bl_gap_rows  every `check` iterations: the row's parts of P and Re <lambda, Y>
//   bl_gap       one workgroup adds the parts; lane 0 alone writes P, D, the
//                iteration count and `done`
//   bl_band      Tout = (j 2 pi / n) tridiag(d, e) Tin, acc += Tout on [K][C]
//   bl_apply     U X for the final sparsity (once a call)
// Every solver kernel returns at once when `done` is set, so the result does
// not depend on how long the host goes on issuing: it reads the flag every
// BL_CHUNK checks, and one scalar (the sparsity) after each solve to take the
// accept / reject decision of basis_opt_new.m:45.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "spain_fft.h"

namespace ainp {

constexpr int BL_MMIN = 8, BL_MMAX = 2048;               // K = M / 2 + 1 with spain_learned's M
constexpr int64_t BL_ELEMS = (int64_t)1 << 26;          // K M_tr
constexpr int BL_MAXIT = 1 << 20, BL_CNT = 64;
constexpr int BL_CHUNK = 32;                             // checks between two looks at `done`
constexpr int BL_COLS = 6;                               // trace columns
constexpr double BL_2PI = 6.283185307179586476925;

struct BlWs {   // byte offsets into the workspace, each a multiple of 16
  size_t Y, Yold, lam, sigma, Ta, Tb, Aold, rho, d, e, db, eb, gd, ge, pP, pD, state, flags, total;
};
static BlWs bl_layout(int64_t K, int64_t Mt) {
  BlWs l;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 15) & ~(size_t)15;
    return o;
  };
  const int64_t C = std::max(K, Mt);
  l.Y = take(sizeof(cplx) * K * Mt);
  l.Yold = take(sizeof(cplx) * K * Mt);
  l.lam = take(sizeof(cplx) * K * Mt);
  l.sigma = take(sizeof(double) * K * Mt);
  l.Ta = take(sizeof(cplx) * K * C);
  l.Tb = take(sizeof(cplx) * K * C);
  l.Aold = take(sizeof(cplx) * K * K);
  l.rho = take(sizeof(double) * K);
  l.d = take(sizeof(double) * K);
  l.e = take(sizeof(cplx) * K);
  l.db = take(sizeof(double) * K);
  l.eb = take(sizeof(cplx) * K);
  l.gd = take(sizeof(double) * K);
  l.ge = take(sizeof(cplx) * K);
  l.pP = take(sizeof(double) * K);
  l.pD = take(sizeof(double) * K);
  l.state = take(sizeof(double) * 4);   // P, D, sparsity
  l.flags = take(sizeof(int) * 4);      // done, iterations
  l.total = at;
  return l;
}

// 1 / (2 pi x); a zero denominator is step 0: the variable or term has no effect
__device__ __forceinline__ double bl_inv(double x) { return x > 0.0 ? 1.0 / (BL_2PI * x) : 0.0; }
__device__ __forceinline__ double bl_abs(cplx z) { return hypot(z.re, z.im); }

// row i of tridiag(d, e) T at column c: d_i T_i + e_i T_{i+1} + conj(e_{i-1}) T_{i-1}
__device__ __forceinline__ cplx bl_band_at(const double* __restrict__ d, const cplx* __restrict__ e,
                                           const cplx* __restrict__ T, int i, int K, int64_t C,
                                           int64_t c) {
  const cplx t = T[i * C + c];
  cplx a = {d[i] * t.re, d[i] * t.im};
  if (i < K - 1) a = cadd(a, cmul(e[i], T[(i + 1) * C + c]));
  if (i > 0) a = cadd(a, cmulc(T[(i - 1) * C + c], e[i - 1]));
  return a;
}

// grid: one workgroup per row
template <int NT>
__global__ __launch_bounds__(NT) void bl_rows(const cplx* __restrict__ Y, int64_t Mt,
                                              double* __restrict__ rho) {
  __shared__ double psum[4];
  const cplx* y = Y + blockIdx.x * Mt;
  double acc = 0.0;
  for (int64_t m = threadIdx.x; m < Mt; m += NT) acc += bl_abs(y[m]);
  const double s = sp_sum<NT>(acc, psum, threadIdx.x);
  if (threadIdx.x == 0) rho[blockIdx.x] = s;
}

// grid: one workgroup.  The rows' sums in a fixed order; o1 nullable.
__global__ __launch_bounds__(256) void bl_total(const double* __restrict__ rho, int K, double* o0,
                                                double* o1) {
  __shared__ double psum[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < K; i += 256) acc += rho[i];
  const double s = sp_sum<256>(acc, psum, threadIdx.x);
  if (threadIdx.x != 0) return;
  *o0 = s;
  if (o1) *o1 = s;
}

// grid: (ceil(Mt / NT), K)
template <int NT>
__global__ __launch_bounds__(NT) void bl_reset(const cplx* __restrict__ Y, int K, int64_t Mt,
                                               double* __restrict__ sigma, cplx* __restrict__ lam,
                                               double* d, cplx* e, double* db, cplx* eb,
                                               int* flags) {
  const int i = blockIdx.y;
  const int64_t m = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d[i] = db[i] = 0.0;
    e[i] = eb[i] = {0.0, 0.0};
    if (i == 0) flags[0] = flags[1] = 0;
  }
  if (m >= Mt) return;
  const int64_t t = i * Mt + m;
  double s = bl_abs(Y[t]);
  if (i < K - 1) s += bl_abs(Y[t + Mt]);
  if (i > 0) s += bl_abs(Y[t - Mt]);
  sigma[t] = bl_inv(s);
  lam[t] = {0.0, 0.0};
}

// grid: (ceil(Mt / NT), K).  lambda <- P_unit(lambda + sigma (Y + j 2 pi A(dbar, ebar) Y))
template <int NT>
__global__ __launch_bounds__(NT) void bl_dual(const cplx* __restrict__ Y,
                                              const double* __restrict__ sigma,
                                              const double* __restrict__ db,
                                              const cplx* __restrict__ eb, cplx* __restrict__ lam,
                                              int K, int64_t Mt, const int* __restrict__ flags) {
  if (flags[0]) return;
  const int i = blockIdx.y;
  const int64_t m = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (m >= Mt) return;
  const int64_t t = i * Mt + m;
  const cplx a = bl_band_at(db, eb, Y, i, K, Mt, m), y = Y[t];
  const double sg = sigma[t];
  cplx z = lam[t];
  z.re += sg * (y.re - BL_2PI * a.im);
  z.im += sg * (y.im + BL_2PI * a.re);
  const double n = sqrt(cabs2(z));
  if (n > 1.0) {
    z.re /= n;
    z.im /= n;
  }
  lam[t] = z;
}

// grid: one workgroup per row i.  g_d[i] = 2 pi sum_m Im(l_i conj y_i),
// g_e[i] = j 2 pi sum_m (conj(l_{i+1}) y_i - l_i conj(y_{i+1})); then lane 0:
// d+ = clip(d - tau_d g_d), e+ = P_level(e - tau_e g_e), bar = 2 new - old.
template <int NT>
__global__ __launch_bounds__(NT) void bl_primal(const cplx* __restrict__ Y,
                                                const cplx* __restrict__ lam,
                                                const double* __restrict__ rho, double* d, cplx* e,
                                                double* db, cplx* eb, double* gd, cplx* ge,
                                                double level, int K, int64_t Mt,
                                                const int* __restrict__ flags) {
  __shared__ double psum[4];
  if (flags[0]) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  const bool off = i < K - 1;
  const cplx *y0 = Y + i * Mt, *l0 = lam + i * Mt;
  double ad = 0.0, aer = 0.0, aei = 0.0;
  for (int64_t m = tid; m < Mt; m += NT) {
    const cplx l = l0[m], y = y0[m];
    ad += l.im * y.re - l.re * y.im;
    if (off) {
      const cplx s = csub(cmulc(y, l0[Mt + m]), cmulc(l, y0[Mt + m]));
      aer -= s.im;   // j s
      aei += s.re;
    }
  }
  ad = sp_sum<NT>(ad, psum, tid);
  if (off) {
    aer = sp_sum<NT>(aer, psum, tid);
    aei = sp_sum<NT>(aei, psum, tid);
  }
  if (tid != 0) return;
  const double g = BL_2PI * ad, dn = fmin(fmax(d[i] - bl_inv(rho[i]) * g, -level), level);
  gd[i] = g;
  db[i] = 2.0 * dn - d[i];
  d[i] = dn;
  if (!off) return;
  const cplx gc = {BL_2PI * aer, BL_2PI * aei}, eo = e[i];
  const double tau = bl_inv(rho[i] + rho[i + 1]);
  cplx en = {eo.re - tau * gc.re, eo.im - tau * gc.im};
  const double n = sqrt(cabs2(en));
  if (n > level) {
    const double f = level / n;
    en.re *= f;
    en.im *= f;
  }
  ge[i] = gc;
  eb[i] = {2.0 * en.re - eo.re, 2.0 * en.im - eo.im};
  e[i] = en;
}

// grid: one workgroup per row.  pP[i] = sum_m |r_im(d, e)|, pD[i] = Re sum_m conj(l) y
template <int NT>
__global__ __launch_bounds__(NT) void bl_gap_rows(const cplx* __restrict__ Y,
                                                  const cplx* __restrict__ lam,
                                                  const double* __restrict__ d,
                                                  const cplx* __restrict__ e,
                                                  double* __restrict__ pP, double* __restrict__ pD,
                                                  int K, int64_t Mt,
                                                  const int* __restrict__ flags) {
  __shared__ double psum[4];
  if (flags[0]) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  double ap = 0.0, al = 0.0;
  for (int64_t m = tid; m < Mt; m += NT) {
    const cplx a = bl_band_at(d, e, Y, i, K, Mt, m), y = Y[i * Mt + m], l = lam[i * Mt + m];
    ap += bl_abs({y.re - BL_2PI * a.im, y.im + BL_2PI * a.re});
    al += l.re * y.re + l.im * y.im;
  }
  ap = sp_sum<NT>(ap, psum, tid);
  al = sp_sum<NT>(al, psum, tid);
  if (tid == 0) {
    pP[i] = ap;
    pD[i] = al;
  }
}

// grid: one workgroup.  P = sum pP, D = sum pD - level (sum |g_d| + sum |g_e|);
// lane 0 takes the stop decision, once.  trow: this solve's row of the trace.
__global__ __launch_bounds__(256) void bl_gap(const double* __restrict__ pP,
                                              const double* __restrict__ pD,
                                              const double* __restrict__ gd,
                                              const cplx* __restrict__ ge, int K, double level,
                                              double gap_tol, int it, int max_iters, double* state,
                                              int* flags, double* trow) {
  __shared__ double psum[4];
  if (flags[0]) return;
  const int tid = threadIdx.x;
  double ap = 0.0, al = 0.0, ag = 0.0;
  for (int i = tid; i < K; i += 256) {
    ap += pP[i];
    al += pD[i];
    ag += fabs(gd[i]);
    if (i < K - 1) ag += bl_abs(ge[i]);
  }
  ap = sp_sum<256>(ap, psum, tid);
  al = sp_sum<256>(al, psum, tid);
  ag = sp_sum<256>(ag, psum, tid);
  if (tid != 0) return;
  const double P = ap, D = al - level * ag;
  state[0] = P;
  state[1] = D;
  flags[1] = it;
  trow[1] = (double)it;
  trow[2] = P;
  trow[3] = D;
  if (P - D <= gap_tol * P || it == max_iters) flags[0] = 1;
}

// grid: (ceil(C / 256), K).  Tout = (j scale) tridiag(d, e) Tin, acc += Tout
__global__ __launch_bounds__(256) void bl_band(const double* __restrict__ d,
                                               const cplx* __restrict__ e,
                                               const cplx* __restrict__ Tin,
                                               cplx* __restrict__ Tout, cplx* __restrict__ acc,
                                               int K, int64_t C, double scale) {
  const int i = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const cplx a = bl_band_at(d, e, Tin, i, K, C, c);
  const cplx o = {-scale * a.im, scale * a.re};
  const int64_t t = i * C + c;
  Tout[t] = o;
  acc[t] = cadd(acc[t], o);
}

// grid: (ceil(Mt / 256), K).  out = U X, the reduction in index order
__global__ __launch_bounds__(256) void bl_apply(const cplx* __restrict__ U,
                                                const cplx* __restrict__ X,
                                                cplx* __restrict__ out, int K, int64_t Mt) {
  const int i = blockIdx.y;
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= Mt) return;
  cplx a = {0.0, 0.0};
  for (int r = 0; r < K; ++r) a = cadd(a, cmul(U[(int64_t)i * K + r], X[r * Mt + m]));
  out[i * Mt + m] = a;
}

// U = I, the trace NaN
__global__ __launch_bounds__(256) void bl_init(cplx* U, int K, double* trace, int ntrace) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < (int64_t)K * K) U[t] = {t / K == t % K ? 1.0 : 0.0, 0.0};
  if (t < ntrace) trace[t] = NAN;
}

__global__ void bl_note(double* trow, double level, double kept) {
  if (level == level) trow[0] = level;
  trow[5] = kept;
}

// the smallest n with (6 pi level)^n / n! < 1e-18 (|A| <= 3 level)
static int bl_terms(double level) {
  int n = 0;
  double term = 1.0;
  while (term >= 1e-18) {
    ++n;
    term *= 3.0 * BL_2PI * level / n;
  }
  return n;
}

static bool bl_shape_ok(int K, int64_t Mt) {
  const int64_t M = 2 * ((int64_t)K - 1);
  return K >= 1 && M >= BL_MMIN && M <= BL_MMAX && (M & (M - 1)) == 0 && Mt >= 1 &&
         K * Mt <= BL_ELEMS;
}

}  // namespace ainp

using namespace ainp;

extern "C" size_t ainp_basis_learn_workspace(int K, int64_t M_tr) {
  if (!bl_shape_ok(K, M_tr)) return 0;
  return bl_layout(K, M_tr).total;
}

extern "C" int ainp_basis_learn(const double* X, int K, int64_t M_tr, double level_init,
                                double epsilon, int cnt_max, double gap_tol, int max_iters,
                                int check, double* U, double* sparsity, double* trace,
                                void* workspace, size_t ws_bytes, void* stream) {
  if (!X || !U || !sparsity || !trace) return record_msg("ainp_basis_learn: bad argument");
  {
    const int64_t M = 2 * ((int64_t)K - 1);
    if (K < 1 || M < BL_MMIN || M > BL_MMAX || (M & (M - 1)))
      return record_msg("ainp_basis_learn: bad argument (K = M / 2 + 1, M a power of two, "
                        "8 <= M <= 2048)");
  }
  if (M_tr < 1) return record_msg("ainp_basis_learn: bad argument (M_tr >= 1)");
  if ((int64_t)K * M_tr > BL_ELEMS)
    return record_msg("ainp_basis_learn: bad argument (K M_tr <= 2^26)");
  if (!(epsilon > 0.0)) return record_msg("ainp_basis_learn: bad argument (epsilon > 0)");
  if (!(level_init > 0.0 && level_init <= 0.25))
    return record_msg("ainp_basis_learn: bad argument (0 < level_init <= 0.25)");
  if (cnt_max < 1 || cnt_max > BL_CNT)
    return record_msg("ainp_basis_learn: bad argument (1 <= cnt_max <= 64)");
  if (!(gap_tol >= 0.0)) return record_msg("ainp_basis_learn: bad argument (gap_tol >= 0)");
  if (check < 1 || check > max_iters || max_iters > BL_MAXIT)
    return record_msg("ainp_basis_learn: bad argument (1 <= check <= max_iters <= 2^20)");
  const int64_t Mt = M_tr;
  const BlWs l = bl_layout(K, Mt);
  if (!workspace || ws_bytes < l.total || ((uintptr_t)workspace & 15))
    return record_msg("ainp_basis_learn: workspace too small or not 16-byte aligned");

  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  auto dbl = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
  auto cpx = [&](size_t off) { return reinterpret_cast<cplx*>(ws + off); };
  cplx *Y = cpx(l.Y), *Yold = cpx(l.Yold), *lam = cpx(l.lam), *Ta = cpx(l.Ta), *Tb = cpx(l.Tb);
  cplx *Aold = cpx(l.Aold), *e = cpx(l.e), *eb = cpx(l.eb), *ge = cpx(l.ge);
  cplx* A = reinterpret_cast<cplx*>(U);
  const cplx* Xc = reinterpret_cast<const cplx*>(X);
  double *sigma = dbl(l.sigma), *rho = dbl(l.rho), *d = dbl(l.d), *db = dbl(l.db), *gd = dbl(l.gd);
  double *pP = dbl(l.pP), *pD = dbl(l.pD), *state = dbl(l.state);
  int* flags = reinterpret_cast<int*>(ws + l.flags);
  const bool narrow = Mt <= 64;   // one wave a row where the rows are that short
  const int nt = narrow ? 64 : 256;
  const dim3 gElem((unsigned)cdiv(Mt, nt), (unsigned)K), gRows((unsigned)K);
  const size_t bytesY = sizeof(cplx) * K * Mt, bytesA = sizeof(cplx) * K * K;
  int chunk = BL_CHUNK;
  if (const char* env = getenv("AINP_BASIS_LEARN_CHUNK")) chunk = atoi(env);   // 0: never look

#define BL_LAUNCH(kern, grid, ...)                                                      \
  do {                                                                                  \
    if (narrow)                                                                         \
      hipLaunchKernelGGL(kern<64>, grid, dim3(64), 0, st, __VA_ARGS__);                 \
    else                                                                                \
      hipLaunchKernelGGL(kern<256>, grid, dim3(256), 0, st, __VA_ARGS__);               \
  } while (0)

  // rho of `of`, their sum into state[2] and into o1
  auto measure = [&](const cplx* of, double* o1) {
    BL_LAUNCH(bl_rows, gRows, of, Mt, rho);
    hipLaunchKernelGGL(bl_total, dim3(1), dim3(256), 0, st, rho, K, state + 2, o1);
  };
  auto read_sparsity = [&](double& v) -> int {
    hipError_t err = hipMemcpyAsync(&v, state + 2, sizeof(double), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    return err == hipSuccess ? AINP_OK : record_error(err, "ainp_basis_learn");
  };
  auto copy = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
  };
  // the subproblem at `level` from zero; rho holds the row sums of Y
  auto solve = [&](double level, double* trow) -> int {
    BL_LAUNCH(bl_reset, gElem, Y, K, Mt, sigma, lam, d, e, db, eb, flags);
    int checks = 0;
    for (int it = 1; it <= max_iters; ++it) {
      BL_LAUNCH(bl_dual, gElem, Y, sigma, db, eb, lam, K, Mt, flags);
      BL_LAUNCH(bl_primal, gRows, Y, lam, rho, d, e, db, eb, gd, ge, level, K, Mt, flags);
      if (it % check == 0 || it == max_iters) {
        BL_LAUNCH(bl_gap_rows, gRows, Y, lam, d, e, pP, pD, K, Mt, flags);
        hipLaunchKernelGGL(bl_gap, dim3(1), dim3(256), 0, st, pP, pD, gd, ge, K, level, gap_tol, it,
                           max_iters, state, flags, trow);
        if (int rc = check_launch("ainp_basis_learn")) return rc;
        if (chunk > 0 && ++checks % chunk == 0 && it < max_iters) {
          // the flag was set on the device; the host only stops issuing
          int done = 0;
          hipError_t err = hipMemcpyAsync(&done, flags, sizeof(int), hipMemcpyDeviceToHost, st);
          if (err == hipSuccess) err = hipStreamSynchronize(st);
          if (err != hipSuccess) return record_error(err, "ainp_basis_learn");
          if (done) break;
        }
      }
    }
    return check_launch("ainp_basis_learn");
  };
  // T <- expm(j 2 pi tridiag(d, e)) T on [K][C]; `old` receives T as it was
  auto update = [&](cplx* T, cplx* old, int64_t C, size_t bytes, int terms) -> hipError_t {
    hipError_t err = copy(old, T, bytes);
    const dim3 grid((unsigned)cdiv(C, 256), (unsigned)K);
    const cplx* in = old;
    cplx* out = Ta;
    for (int n = 1; n <= terms; ++n) {
      hipLaunchKernelGGL(bl_band, grid, dim3(256), 0, st, d, e, in, out, T, K, C, BL_2PI / n);
      in = out;
      out = out == Ta ? Tb : Ta;
    }
    return err;
  };

  const int ntrace = cnt_max * BL_COLS;
  hipLaunchKernelGGL(bl_init, dim3((unsigned)cdiv(std::max<int64_t>((int64_t)K * K, ntrace), 256)),
                     dim3(256), 0, st, A, K, trace, ntrace);
  if (hipError_t err = copy(Y, Xc, bytesY)) return record_error(err, "ainp_basis_learn");
  measure(Y, sparsity);
  double sp = 0.0, sp_old = INFINITY, save = INFINITY, level = level_init;
  if (int rc = read_sparsity(sp)) return rc;
  int cnt = 1;
  // basis_opt_new.m:43-74
  while (level > epsilon) {
    while (sp < sp_old) {
      double* trow = trace + (size_t)BL_COLS * (cnt - 1);
      if (int rc = solve(level, trow)) return rc;
      save = sp_old;
      sp_old = sp;
      const int terms = bl_terms(level);
      hipError_t err = update(A, Aold, K, bytesA, terms);
      if (err == hipSuccess) err = update(Y, Yold, Mt, bytesY, terms);
      if (err != hipSuccess) return record_error(err, "ainp_basis_learn");
      measure(Y, trow + 4);
      hipLaunchKernelGGL(bl_note, dim3(1), dim3(1), 0, st, trow, level, 1.0);
      if (int rc = read_sparsity(sp)) return rc;
      if (++cnt > cnt_max) break;
    }
    if (cnt > cnt_max) break;
    // the last update made it worse: undo it and halve the level
    if (cnt >= 2)   // (a sparsity that is not a number never enters the loop above)
      hipLaunchKernelGGL(bl_note, dim3(1), dim3(1), 0, st, trace + (size_t)BL_COLS * (cnt - 2), NAN,
                         0.0);
    level *= 0.5;
    if (cnt >= 2) {
      hipError_t err = copy(A, Aold, bytesA);
      if (err == hipSuccess) err = copy(Y, Yold, bytesY);
      if (err != hipSuccess) return record_error(err, "ainp_basis_learn");
      BL_LAUNCH(bl_rows, gRows, Y, Mt, rho);
    }
    sp = sp_old;
    sp_old = save;
  }
  // sparsity_final = |U X|_1 from the returned U
  hipLaunchKernelGGL(bl_apply, dim3((unsigned)cdiv(Mt, 256), (unsigned)K), dim3(256), 0, st, A, Xc,
                     Ta, K, Mt);
  measure(Ta, sparsity + 1);
#undef BL_LAUNCH
  return check_launch("ainp_basis_learn");
}
