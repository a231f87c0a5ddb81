// capi.cpp — library identity and error reporting for the ainp C ABI.
#include <rocprofiler-sdk-roctx/roctx.h>
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "common.h"
#include "gemm_route.h"

namespace ainp {
static thread_local char g_last_error[512] = "";

int record_error(hipError_t e, const char* where) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: %s", where,
           hipGetErrorString(e));
  return AINP_ELAUNCH;
}
int record_msg(const char* msg) {
  snprintf(g_last_error, sizeof(g_last_error), "%s", msg);
  return AINP_EINVAL;
}
int record_bad_argument(const char* fn, const char* rule) {
  if (rule) snprintf(g_last_error, sizeof(g_last_error), "%s: bad argument (%s)", fn, rule);
  else snprintf(g_last_error, sizeof(g_last_error), "%s: bad argument", fn);
  return AINP_EINVAL;
}
}  // namespace ainp

extern "C" int ainp_abi_version(void) { return 1; }

// Host-only GEMM queries (gemm_route.h: what the launchers themselves call)
extern "C" int ainp_gemm_bf16nt_tile(int64_t M, int64_t N, int64_t K, int nsplit) {
  // a split's chunk is whole g16 K-tiles, so only the unsplit kc (= K) matters
  return ainp::route_gemm_bf16nt(M, N, K, nsplit, nsplit == 1 ? K : ainp::G16_BK,
                                 ainp::gemm_env()).tile;
}
extern "C" int ainp_gemm_splitk_granule(int family, int64_t K) {
  return ainp::splitk_granule(family, K);
}

// Per-phase trace ranges (SURVEY §5 tracing): roctx ranges of the
// rocprofiler-sdk marker API, recorded by `rocprofv3 --marker-trace`; a no-op
// cost (one call) when no profiler is attached.
extern "C" int ainp_range_push(const char* name) { return roctxRangePushA(name ? name : "?"); }
extern "C" int ainp_range_pop(void) { return roctxRangePop(); }
extern "C" void ainp_mark(const char* name) { roctxMarkA(name ? name : "?"); }
extern "C" const char* ainp_build_target(void) { return "gfx950"; }
extern "C" const char* ainp_last_error(void) { return ainp::g_last_error; }
