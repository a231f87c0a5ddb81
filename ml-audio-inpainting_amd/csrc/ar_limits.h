// ar_limits.h — the size limits of the audio-regression kernels (janssen.hip, janssen_mask.hip,
// ar_extrapolate.hip, janssen_windows.hip, and through spain_window.h and
// spain_plan.h spain.hip and spain_omp.hip), host and device.  The Python host
// layer restates them (ainp/janssen.py: P_MAX, N_MAX, GAP_MAX, MAXIT_MAX).
#pragma once

namespace ainp {

constexpr int JN_PMAX = 3072;    // AR order
constexpr int JN_NMAX = 16384;   // samples of a segment or a window
constexpr int JN_HMAX = 2048;    // missing samples of a segment, a window or a gap
constexpr int JN_ITMAX = 1000;   // Janssen iterations
constexpr int AINP_SPAIN_OMP_DIMS = 512;   // real unknowns of S-SPAIN OMP's least squares

}  // namespace ainp
