// rtx_lights.hip — several point lights with intensity and colour (rtx_trace_lights): explicit rays
// through a scene that every point light of a table lights, each with e = intensity * colour per
// channel (the reference lights with scene.lights[0] alone, white, of strength 1: main.py "TODO: use
// multiple lights", domain.py "class PointLight:  # TODO: add intensity"). The arithmetic of a hit is
// written out in include/rtx_hip.h; DESIGN.md §15 has the rest. A translation unit of its own over the
// shared device text (rtx_device.h), like rtx_glass.hip: the render kernels compile from untouched text
// with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_env.h"

namespace {

constexpr int kLightWords = 6;    // a table row: position, e = intensity * colour
constexpr int kLightRayWords = 10;  // a pending ray: origin, direction, RGB weight, level
// Pending-ray stacks live in the workspace, kLightRayWords * lights_stack_entries(B) words per worker;
// the pool of workers is bounded by this budget and by kLightsMaxWorkers, whatever the ray count (the
// glass kernel's rule)
constexpr size_t kLightsStackBudget = size_t(256) << 20;
// 3,072 waves: kLightsWaves per SIMD on a 256-CU part, all resident (the glass kernel's pool; not
// measured against another for this kernel)
constexpr int64_t kLightsMaxWorkers = 196608;
// waves per SIMD the kernel is compiled for: 168 VGPRs, 8 spilled. Measured against 2 (189 VGPRs, none
// spilled) and 4 (128, 51 spilled) on lights_spec 1080p at cap 3, one light / three / eight: 111.6 / 170.6 /
// 319.5 us against 144.4 / 218.4 / 409.4 and 179.4 / 230.0 / 372.4 (profiles/lights_waves_ab.json)
constexpr int kLightsWaves = 3;

// A hit pushes at most one ray (the reflected one), and a ray's hits are the shapes at its nearest
// distance. A chain needs 1 entry; in a tree whose every ray meets t shapes each popped ray leaves
// t - 1 siblings below it, so after the pushes of level k (the last that pushes is B - 1) the stack holds
// (t - 1) k + t: B + 1 for ties of two at every level, 2B + 1 for ties of three.
__host__ __device__ constexpr int lights_stack_entries(int B) { return 2 * B + 2; }

int64_t lights_workers(int64_t n, int B) {
  const int64_t per = (int64_t)lights_stack_entries(B) * kLightRayWords * 8;
  int64_t w = (int64_t)(kLightsStackBudget / (size_t)per) / 64 * 64;
  if (w > kLightsMaxWorkers) w = kLightsMaxWorkers;
  const int64_t need = (n + 63) / 64 * 64;
  return need < w ? need : w;
}

struct LightsParams {
  const double* scene;
  int nsph;
  const double* lights;  // [n_lights][6]: px, py, pz, e_r, e_g, e_b
  int n_lights;
  const double* org;
  int64_t org_stride;
  const double* dir;
  int64_t n;
  int max_bounces;
  void* out;
  int out_kind;
  uint32_t* status;  // the workspace's RTX_WS_STATUS word
  double* stack;
  int64_t n_workers;
};

// The lane's stack of pending rays, lane-interleaved like the glass kernel's: word f of entry e of 64
// consecutive workers is one contiguous run.
struct LightRayStack {
  double* base;
  int64_t nw;
  int64_t w;
  __device__ __forceinline__ double& at(int e, int f) const {
    return base[((int64_t)e * kLightRayWords + f) * nw + w];
  }
  __device__ __forceinline__ void push(int e, double ox, double oy, double oz, double dx, double dy, double dz,
                                       double wr, double wg, double wb, int level) const {
    at(e, 0) = ox; at(e, 1) = oy; at(e, 2) = oz;
    at(e, 3) = dx; at(e, 4) = dy; at(e, 5) = dz;
    at(e, 6) = wr; at(e, 7) = wg; at(e, 8) = wb;
    at(e, 9) = (double)level;
  }
};

// One lane per ray item; a bounded pool of workers loops over the items. A lane walks its ray tree with
// a stack of pending rays and a forward-folded weight per channel (the glass kernel's walk): every
// shaded hit adds W[c] * (its colour with a black reflection) and pushes the reflected ray with weight
// ((W[c] * 0.5) * g) * sum_i lit_i e_i[c]. The lanes of a wave that need a new ray pop and search
// together; a lane at a tie shades its shapes one per round in scene order. The loop over the lights is
// wave-uniform (the table row comes through the scalar cache): one any-hit shadow search per light, and
// the specular of a light only where some lane of the wave is lit by it.
// The kernel's body is rtx_lights_walk.inc, included below into k_trace_lights (ENV false: the kernel as it was)
// and into k_trace_lights_env (ENV true: a popped ray that meets no shape adds env(D), rtx_env.h, before the
// lane goes on; the lookup runs where little is live, after the pop and before any shade).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kLightsWaves, kLightsWaves)))
void k_trace_lights(LightsParams p) {
  constexpr bool ENV = false;
  const EnvFields env{};  // (not read)
#include "rtx_lights_walk.inc"
}

struct LightsEnvParams : LightsParams {
  EnvFields env;
};

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kLightsWaves, kLightsWaves)))
void k_trace_lights_env(LightsEnvParams p) {
  constexpr bool ENV = true;
  const EnvFields& env = p.env;
#include "rtx_lights_walk.inc"
}

}  // namespace

extern "C" size_t rtx_lights_workspace_bytes(int64_t n_rays, int max_bounces) {
  if (n_rays < 0 || max_bounces < 0 || max_bounces > RTX_LIGHTS_MAX_BOUNCES) return 0;
  return (size_t)RTX_WS_HDR_BYTES +
         (size_t)lights_workers(n_rays, max_bounces) * lights_stack_entries(max_bounces) * kLightRayWords * 8;
}

namespace {

// rtx_trace_lights (with_env false: env is not read) and rtx_trace_lights_env behind one set of checks
int trace_lights_call(const double* scene, int n_spheres, const double* lights, int n_lights, const double* origins,
                      int64_t origin_stride, const double* dirs, int64_t n, int max_bounces, void* out, int out_kind,
                      void* workspace, size_t workspace_bytes, void* stream, bool with_env, const rtx_env_t* env) {
  if (const int rc = stack_call_pointers(scene, {{lights, "null lights table pointer"}}, origins, dirs, out, workspace))
    return rc;
  if (n_spheres < 1 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (n_lights < 1 || n_lights > RTX_MAX_POINT_LIGHTS)
    return rtx_fail(RTX_E_ARG, "n_lights out of range (1..%d)", (int)RTX_MAX_POINT_LIGHTS);
  if (max_bounces < 0 || max_bounces > RTX_LIGHTS_MAX_BOUNCES)
    return rtx_fail(RTX_E_ARG, "max_bounces out of range (0..%d): a multi-light scene needs a finite cap",
                    (int)RTX_LIGHTS_MAX_BOUNCES);
  // (the size is computed ahead of the checks on out_kind and n: the size function has no effects and gives 0 for n < 0)
  if (const int rc = stack_call_rays(out_kind, n, origin_stride, workspace_bytes,
                                     rtx_lights_workspace_bytes(n, max_bounces), "rtx_lights_workspace_bytes"))
    return rc;
  LightsEnvParams p{};
  if (with_env)
    if (const int rc = env_fields(env, p.env)) return rc;
  if (n == 0) return RTX_OK;
  p.scene = scene;
  p.nsph = n_spheres;
  p.lights = lights;
  p.n_lights = n_lights;
  stack_params(p, origins, origin_stride, dirs, n, max_bounces, out, out_kind, workspace, lights_workers(n, max_bounces));
  const dim3 grid((unsigned)(p.n_workers / 64));
  if (with_env) {
    hipLaunchKernelGGL(k_trace_lights_env, grid, dim3(64), 0, (hipStream_t)stream, p);
    return rtx_launched("k_trace_lights_env");
  }
  hipLaunchKernelGGL(k_trace_lights, grid, dim3(64), 0, (hipStream_t)stream, (const LightsParams&)p);
  return rtx_launched("k_trace_lights");
}

}  // namespace

extern "C" int rtx_trace_lights(const double* scene, int n_spheres, const double* lights, int n_lights,
                                const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                                int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes,
                                void* stream) {
  return trace_lights_call(scene, n_spheres, lights, n_lights, origins, origin_stride, dirs, n, max_bounces, out,
                           out_kind, workspace, workspace_bytes, stream, false, nullptr);
}

extern "C" int rtx_trace_lights_env(const double* scene, int n_spheres, const double* lights, int n_lights,
                                    const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                                    int max_bounces, void* out, int out_kind, void* workspace,
                                    size_t workspace_bytes, void* stream, const rtx_env_t* env) {
  return trace_lights_call(scene, n_spheres, lights, n_lights, origins, origin_stride, dirs, n, max_bounces, out,
                           out_kind, workspace, workspace_bytes, stream, true, env);
}
