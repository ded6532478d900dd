// rtx_env.h — the environment map: what a ray that meets no shape sees (the reference returns black,
// base.py:100-121; its render settings carry a "background" image that nothing reads). An
// equirectangular float32 image [H][W][4] (RGB and a zero word), sampled bilinearly at the direction's
// spherical coordinates, the mapping of image_texel (rtx_device.h) applied to a direction. The
// arithmetic is written out in include/rtx_hip.h; DESIGN.md §16 has the rest. Included after
// rtx_device.h by the units that sample it (rtx_env.hip, rtx_lights.hip, rtx_glass.hip);
// rtx_device.h itself does not know it.
#pragma once

#include "rtx_internal.h"

namespace {

// The environment as a kernel reads it. Every field is wave-uniform (a kernel argument): the base
// pointer, the sizes, the gain and the turn stay in scalar registers.
typedef float env_texel_t __attribute__((ext_vector_type(4)));  // RGB and a zero word
struct EnvFields {
  const env_texel_t* texels;  // [height][width], 16-byte aligned: one 128-bit load per tap
  int width, height;
  double gr, gg, gb;  // intensity * colour
  double turn;        // rotation about +y in turns
};

// env(D): float64, in the order of include/rtx_hip.h, no contraction. A direction whose u or v is not
// finite (a NaN component) gives (0, 0, 0) and reads texel 0 only. The four taps are loaded before the
// first of them is used; their indices lie in the image whatever u and v are.
__device__ __forceinline__ void env_radiance(const EnvFields& e, double dx, double dy, double dz, double& r, double& g,
                                             double& b) {
  const int W = e.width, H = e.height;
  double u = (0.5 + atan2(dz, dx) / (2.0 * RTX_PI)) + e.turn;
  u = u - floor(u);
  const double sy = dy < -1.0 ? -1.0 : (dy > 1.0 ? 1.0 : dy);  // min(max(D.y, -1), 1); a NaN stays one
  double v = 0.5 - asin(sy) / RTX_PI;
  const bool ok = isfinite(u) && isfinite(v);
  if (!ok) u = v = 0.0;
  const double x = u * (double)W - 0.5, y = v * (double)H - 0.5;
  const double xf = floor(x), yf = floor(y);
  const double fx = x - xf, fy = y - yf;
  int i0 = (int)xf, j0 = (int)yf;  // u, v in [0, 1]: i0 in -1..W-1, j0 in -1..H-1
  int i1 = i0 + 1, j1 = j0 + 1;
  if (i1 >= W) i1 -= W;  // the seam wraps
  if (i0 < 0) i0 += W;
  i0 = min(max(i0, 0), W - 1);  // (no-ops for u, v in [0, 1])
  i1 = min(max(i1, 0), W - 1);
  j1 = min(max(j1, 0), H - 1);  // the poles clamp
  j0 = min(max(j0, 0), H - 1);
  env_texel_t t00 = e.texels[j0 * W + i0];
  env_texel_t t01 = e.texels[j0 * W + i1];
  env_texel_t t10 = e.texels[j1 * W + i0];
  env_texel_t t11 = e.texels[j1 * W + i1];
  // (an empty statement that names whole texels: without it the zero word is dead and the compiler
  // splits each tap into a 64-bit and a 32-bit load)
  asm volatile("" : "+v"(t00), "+v"(t01), "+v"(t10), "+v"(t11));
  const double ax = 1.0 - fx, ay = 1.0 - fy;
  const double topr = (double)t00.x * ax + (double)t01.x * fx, botr = (double)t10.x * ax + (double)t11.x * fx;
  const double topg = (double)t00.y * ax + (double)t01.y * fx, botg = (double)t10.y * ax + (double)t11.y * fx;
  const double topb = (double)t00.z * ax + (double)t01.z * fx, botb = (double)t10.z * ax + (double)t11.z * fx;
  r = ok ? (topr * ay + botr * fy) * e.gr : 0.0;
  g = ok ? (topg * ay + botg * fy) * e.gg : 0.0;
  b = ok ? (topb * ay + botb * fy) * e.gb : 0.0;
}

// rtx_env_t as the kernels take it, and the argument checks every entry that takes one shares (before
// any HIP call): 0, or the code rtx_fail returned.
inline int env_fields(const rtx_env_t* env, EnvFields& f) {
  if (!env) return rtx_fail(RTX_E_ARG, "null environment pointer");
  if (!env->texels) return rtx_fail(RTX_E_ARG, "null environment texel pointer");
  if (env->width < 1 || env->height < 1) return rtx_fail(RTX_E_ARG, "environment width and height must be >= 1");
  if ((int64_t)env->width * env->height > RTX_ENV_MAX_TEXELS)
    return rtx_fail(RTX_E_ARG, "environment larger than RTX_ENV_MAX_TEXELS (%d) texels", (int)RTX_ENV_MAX_TEXELS);
  if ((uintptr_t)env->texels % 16 != 0) return rtx_fail(RTX_E_ARG, "environment texels must be 16-byte aligned");
  for (int c = 0; c < 3; ++c)
    if (!(env->gain[c] - env->gain[c] == 0.0)) return rtx_fail(RTX_E_ARG, "environment gain must be finite");
  if (!(env->turn - env->turn == 0.0)) return rtx_fail(RTX_E_ARG, "environment turn must be finite");
  f.texels = (const env_texel_t*)env->texels;
  f.width = env->width;
  f.height = env->height;
  f.gr = env->gain[0];
  f.gg = env->gain[1];
  f.gb = env->gain[2];
  f.turn = env->turn;
  return RTX_OK;
}

}  // namespace
