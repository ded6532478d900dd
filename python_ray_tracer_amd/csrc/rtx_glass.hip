// rtx_glass.hip — transmission (rtx_trace_glass): explicit rays through a scene in which some spheres
// are solid glass. A ray that meets such a sphere from outside is refracted in, crosses the ball and
// is refracted out; the ray that leaves is traced like any other, one more level of raytrace_scene
// (the reference marks the spot: shader.py:143 "TODO: VOIR TRANSMISSION"). Every hit adds
// transmission * transmission_gain after the iridescence term (shader.py:110), lit or not. The
// arithmetic of the passage is written out in include/rtx_hip.h; DESIGN.md §14 has the rest. A
// translation unit of its own over the shared device text (rtx_device.h), like rtx_occlusion.hip: the
// render kernels compile from untouched text with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_env.h"

namespace {

constexpr int kRayWords = 8;  // a pending ray: origin, direction, weight, level
// Pending-ray stacks live in the workspace, kRayWords * glass_stack_entries(B) words per worker; the
// pool of workers is bounded by this budget and by kGlassMaxWorkers, whatever the ray count (the
// general kernel's rule, kStackBudget / workers_for)
constexpr size_t kGlassStackBudget = size_t(256) << 20;
// 3,072 waves: the 3 per SIMD its 146 VGPRs allow on a 256-CU part, all resident (A/B against 131,072 workers,
// two alternating pairs, glass_spec 1080p: B = 3 176.4 -> 146.5 us, B = 5 269.0 -> 231.9 us)
constexpr int64_t kGlassMaxWorkers = 196608;
// waves per SIMD the kernel is compiled for (A/B against 4, which takes 127 VGPRs and spills 4, with 262,144
// workers: B = 3 -2.8%, B = 5 +2.9%)
constexpr int kGlassWaves = 3;
// (The stacks are in the workspace, not in LDS: [entry][word][lane] there is 4 KB per entry and wave, so the
// 64 KB a block may ask for hold caps up to 3 only and two waves per CU, measured 2.7x slower at B = 3;
// DESIGN.md §14, profiles/glass_ab.json.)

__host__ __device__ constexpr int glass_stack_entries(int B) { return 4 * B + 4; }

int64_t glass_workers(int64_t n, int B) {
  const int64_t per = (int64_t)glass_stack_entries(B) * kRayWords * 8;
  int64_t w = (int64_t)(kGlassStackBudget / (size_t)per) / 64 * 64;
  if (w > kGlassMaxWorkers) w = kGlassMaxWorkers;
  const int64_t need = (n + 63) / 64 * 64;
  return need < w ? need : w;
}

struct GlassParams {
  const double* scene;
  int nsph;
  const double* glass;  // [2][nsph]: transmission_gain, specular_ior
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

// The lane's stack of pending rays, lane-interleaved like the general kernel's Stack: word f of entry
// e of 64 consecutive workers is one contiguous run.
struct RayStack {
  double* base;
  int64_t nw;
  int64_t w;
  __device__ __forceinline__ double& at(int e, int f) const {
    return base[((int64_t)e * kRayWords + f) * nw + w];
  }
  __device__ __forceinline__ void push(int e, double ox, double oy, double oz, double dx, double dy, double dz,
                                       double wt, int level) const {
    at(e, 0) = ox; at(e, 1) = oy; at(e, 2) = oz;
    at(e, 3) = dx; at(e, 4) = dy; at(e, 5) = dz;
    at(e, 6) = wt;
    at(e, 7) = (double)level;
  }
};

// The ray that leaves a solid glass ball (centre C, 1/radius inv_r, index ior) which the ray D met
// from outside at P with normal n and c = D.n < 0: refracted in at P, straight across, refracted out
// at E. No total internal reflection: by the ball's symmetry the exit angle is the entry angle.
__device__ __forceinline__ void through_ball(double px, double py, double pz, double dx, double dy, double dz,
                                             double nx, double ny, double nz, double c, double cx, double cy,
                                             double cz, double inv_r, double ior, double& ox, double& oy, double& oz,
                                             double& rx, double& ry, double& rz) {
  const double eta = div_cr(1.0, ior);
  const double ci = -c;
  const double k = 1.0 - (eta * eta) * (1.0 - ci * ci);
  const double f = eta * ci - sqrt_cr(k);
  double tx = dx * eta + nx * f, ty = dy * eta + ny * f, tz = dz * eta + nz * f;
  norm3(tx, ty, tz);
  const double b = dot3(tx, ty, tz, px - cx, py - cy, pz - cz);
  const double b2 = 2.0 * b;
  const double ex = px - tx * b2, ey = py - ty * b2, ez = pz - tz * b2;  // the exit point
  const double ux = (ex - cx) * inv_r, uy = (ey - cy) * inv_r, uz = (ez - cz) * inv_r;
  const double ce = dot3(tx, ty, tz, ux, uy, uz);
  const double ke = max0(1.0 - (ior * ior) * (1.0 - ce * ce));
  const double g = sqrt_cr(ke) - ior * ce;
  ox = ex + ux * 0.0001;
  oy = ey + uy * 0.0001;
  oz = ez + uz * 0.0001;
  rx = tx * ior + ux * g;
  ry = ty * ior + uy * g;
  rz = tz * ior + uz * g;
  norm3(rx, ry, rz);
}

// One lane per ray item; a bounded pool of workers loops over the items. A lane walks its ray tree
// with a stack of pending rays and a forward-folded weight (the general kernel's sum, trace_general):
// every shaded hit adds weight * (its colour with a black reflection), and pushes the reflected ray
// with weight (w * 0.5) * g and the transmitted ray with weight w * gain. The lanes of a wave that
// need a new ray pop and search together (the search loops are wave-uniform, the sphere table comes
// through the scalar cache); a lane at a tie (several shapes at the nearest distance, base.py:102-119)
// shades them one per round in scene order.
// The kernel's body is rtx_glass_walk.inc, included below into k_trace_glass (ENV false: the kernel as it was)
// and into k_trace_glass_env (ENV true: a popped ray that meets no shape adds env(D), rtx_env.h, before the
// lane goes on; the lookup runs where little is live, after the pop and before any shade).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kGlassWaves, kGlassWaves)))
void k_trace_glass(GlassParams p) {
  constexpr bool ENV = false;
  const EnvFields env{};  // (not read)
#include "rtx_glass_walk.inc"
}

struct GlassEnvParams : GlassParams {
  EnvFields env;
};

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kGlassWaves, kGlassWaves)))
void k_trace_glass_env(GlassEnvParams p) {
  constexpr bool ENV = true;
  const EnvFields& env = p.env;
#include "rtx_glass_walk.inc"
}

}  // namespace

extern "C" size_t rtx_glass_workspace_bytes(int64_t n_rays, int max_bounces) {
  if (n_rays < 0 || max_bounces < 0 || max_bounces > RTX_GLASS_MAX_BOUNCES) return 0;
  return (size_t)RTX_WS_HDR_BYTES +
         (size_t)glass_workers(n_rays, max_bounces) * glass_stack_entries(max_bounces) * kRayWords * 8;
}

namespace {

// rtx_trace_glass (with_env false: env is not read) and rtx_trace_glass_env behind one set of checks
int trace_glass_call(const double* scene, int n_spheres, const double* glass, const double* origins,
                     int64_t origin_stride, const double* dirs, int64_t n, int max_bounces, void* out, int out_kind,
                     void* workspace, size_t workspace_bytes, void* stream, bool with_env, const rtx_env_t* env) {
  if (const int rc = stack_call_pointers(scene, {{glass, "null glass table pointer"}}, origins, dirs, out, workspace))
    return rc;
  if (n_spheres < 1 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (max_bounces < 0 || max_bounces > RTX_GLASS_MAX_BOUNCES)
    return rtx_fail(RTX_E_ARG, "max_bounces out of range (0..%d): a transmissive scene needs a finite cap",
                    (int)RTX_GLASS_MAX_BOUNCES);
  // (the size is computed ahead of the checks on out_kind and n: the size function has no effects and gives 0 for n < 0)
  if (const int rc = stack_call_rays(out_kind, n, origin_stride, workspace_bytes,
                                     rtx_glass_workspace_bytes(n, max_bounces), "rtx_glass_workspace_bytes"))
    return rc;
  GlassEnvParams p{};
  if (with_env)
    if (const int rc = env_fields(env, p.env)) return rc;
  if (n == 0) return RTX_OK;
  p.scene = scene;
  p.nsph = n_spheres;
  p.glass = glass;
  stack_params(p, origins, origin_stride, dirs, n, max_bounces, out, out_kind, workspace, glass_workers(n, max_bounces));
  const dim3 grid((unsigned)(p.n_workers / 64));
  if (with_env) {
    hipLaunchKernelGGL(k_trace_glass_env, grid, dim3(64), 0, (hipStream_t)stream, p);
    return rtx_launched("k_trace_glass_env");
  }
  hipLaunchKernelGGL(k_trace_glass, grid, dim3(64), 0, (hipStream_t)stream, (const GlassParams&)p);
  return rtx_launched("k_trace_glass");
}

}  // namespace

extern "C" int rtx_trace_glass(const double* scene, int n_spheres, const double* glass, const double* origins,
                               int64_t origin_stride, const double* dirs, int64_t n, int max_bounces, void* out,
                               int out_kind, void* workspace, size_t workspace_bytes, void* stream) {
  return trace_glass_call(scene, n_spheres, glass, origins, origin_stride, dirs, n, max_bounces, out, out_kind,
                          workspace, workspace_bytes, stream, false, nullptr);
}

extern "C" int rtx_trace_glass_env(const double* scene, int n_spheres, const double* glass, const double* origins,
                                   int64_t origin_stride, const double* dirs, int64_t n, int max_bounces, void* out,
                                   int out_kind, void* workspace, size_t workspace_bytes, void* stream,
                                   const rtx_env_t* env) {
  return trace_glass_call(scene, n_spheres, glass, origins, origin_stride, dirs, n, max_bounces, out, out_kind,
                          workspace, workspace_bytes, stream, true, env);
}
