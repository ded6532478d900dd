// rtx_env.hip — the environment map's lookup on its own (rtx_env_sample): env(D) of n directions, one
// lane per direction. What the traced kernels add for a ray that meets no shape (rtx_trace_lights_env,
// rtx_trace_glass_env; rtx_env.h), here for a background plate, for the tests and as the yardstick of
// what the lookup costs alone. The arithmetic is written out in include/rtx_hip.h; DESIGN.md §16 has
// the rest. A translation unit of its own over the shared device text (rtx_device.h), like
// rtx_lights.hip.
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_env.h"

namespace {

struct EnvSampleParams {
  EnvFields env;
  const double* dir;  // [3][n]
  double* out;        // [3][n]
  int64_t n;
};

__global__ __launch_bounds__(256) void k_env_sample(EnvSampleParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  double r, g, b;
  env_radiance(p.env, p.dir[i], p.dir[p.n + i], p.dir[2 * p.n + i], r, g, b);
  p.out[i] = r;
  p.out[p.n + i] = g;
  p.out[2 * p.n + i] = b;
}

}  // namespace

extern "C" int rtx_env_sample(const rtx_env_t* env, const double* dirs, int64_t n, double* out, void* stream) {
  EnvSampleParams p{};
  if (const int rc = env_fields(env, p.env)) return rc;
  if (!dirs) return rtx_fail(RTX_E_ARG, "null direction pointer");
  if (!out) return rtx_fail(RTX_E_ARG, "null output pointer");
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative direction count");
  if (n == 0) return RTX_OK;
  p.dir = dirs;
  p.out = out;
  p.n = n;
  hipLaunchKernelGGL(k_env_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  return rtx_launched("k_env_sample");
}
