// rtx_mesh.hip — triangle meshes (rtx_trace_mesh, rtx_trace_mesh_uv): explicit rays through the spheres of
// a scene and the triangles of a mesh table, lit by a table of point lights as rtx_trace_lights lights its spheres (the
// reference's only Shape is the sphere, domain.py:43-50). The triangle test, the group rule, the normals
// and the shadow rule are written out in include/rtx_hip.h; DESIGN.md §17 has the rest. A translation
// unit of its own over the shared device text (rtx_device.h), like rtx_lights.hip: the other kernels
// compile from untouched text with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_mesh_device.h"

namespace {

constexpr int kLightWords = 6;      // a lights table row: position, e = intensity * colour
constexpr int kMeshRayWords = 10;   // a pending ray: origin, direction, RGB weight, level
// Pending-ray stacks live in the workspace, kMeshRayWords * mesh_stack_entries(B) words per worker; the
// pool of workers is bounded by this budget and by kMeshMaxWorkers, whatever the ray count (the lights
// kernel's rule and figures)
constexpr size_t kMeshStackBudget = size_t(256) << 20;
constexpr int64_t kMeshMaxWorkers = 196608;
// waves per SIMD the kernel is compiled for: 168 VGPRs, 12 spilled. Measured against 2 (181 VGPRs, none
// spilled) and 4 (128, 77 spilled) on mesh_spec 1080p at cap 3, icosphere level 2 / 4 / 6: 1,148 / 1,391 /
// 3,582 us against 1,255 / 1,734 / 4,123 and 1,213 / 1,499 / 3,686 (profiles/mesh_waves_ab.json)
constexpr int kMeshWaves = 3;

// A hit pushes at most one ray, and a ray's hits are the spheres at its nearest distance and the triangle
// group if it ties with them: the lights kernel's count (2B + 1 for ties of three at every level).
__host__ __device__ constexpr int mesh_stack_entries(int B) { return 2 * B + 2; }

int64_t mesh_workers(int64_t n, int B) {
  const int64_t per = (int64_t)mesh_stack_entries(B) * kMeshRayWords * 8;
  int64_t w = (int64_t)(kMeshStackBudget / (size_t)per) / 64 * 64;
  if (w > kMeshMaxWorkers) w = kMeshMaxWorkers;
  const int64_t need = (n + 63) / 64 * 64;
  return need < w ? need : w;
}

struct MeshParams {
  const double* scene;
  int nsph;
  const double* mesh;
  int64_t mesh_words;
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

// The lane's stack of pending rays, lane-interleaved like the lights kernel's
struct MeshRayStack {
  double* base;
  int64_t nw;
  int64_t w;
  __device__ __forceinline__ double& at(int e, int f) const {
    return base[((int64_t)e * kMeshRayWords + f) * nw + w];
  }
  __device__ __forceinline__ void push(int e, double ox, double oy, double oz, double dx, double dy, double dz,
                                       double wr, double wg, double wb, int level) const {
    at(e, 0) = ox; at(e, 1) = oy; at(e, 2) = oz;
    at(e, 3) = dx; at(e, 4) = dy; at(e, 5) = dz;
    at(e, 6) = wr; at(e, 7) = wg; at(e, 8) = wb;
    at(e, 9) = (double)level;
  }
};

// One lane per ray item; a bounded pool of workers loops over the items (the lights kernel's walk: a
// stack of pending rays and a forward-folded weight per channel). A popped ray's hits are the spheres at
// its nearest distance, in scene order, then the triangle group's if it is as near; the lanes shade one
// hit per round. A lane on a triangle takes its point's terms from the triangle's row, its material from
// the mesh's row and a shadow test with t_self = FARAWAY; everything after that is one text for both.
// The kernel's body is rtx_mesh_walk.inc, included below into k_trace_mesh (UV false: the kernel as it was)
// and into k_trace_mesh_uv (UV true: a lane on a triangle whose mesh has an image takes its texture colour
// from the table's UV part and texel blocks, mesh_uv_colour).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kMeshWaves, kMeshWaves)))
void k_trace_mesh(MeshParams p) {
  constexpr bool UV = false;
#include "rtx_mesh_walk.inc"
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kMeshWaves, kMeshWaves)))
void k_trace_mesh_uv(MeshParams p) {
  constexpr bool UV = true;
#include "rtx_mesh_walk.inc"
}

}  // namespace

extern "C" size_t rtx_mesh_workspace_bytes(int64_t n_rays, int max_bounces) {
  if (n_rays < 0 || max_bounces < 0 || max_bounces > RTX_MESH_MAX_BOUNCES) return 0;
  return (size_t)RTX_WS_HDR_BYTES +
         (size_t)mesh_workers(n_rays, max_bounces) * mesh_stack_entries(max_bounces) * kMeshRayWords * 8;
}

namespace {

// rtx_trace_mesh (uv false) and rtx_trace_mesh_uv behind one set of checks
int trace_mesh_call(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words, const double* lights,
                    int n_lights, const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                    int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes, void* stream,
                    bool uv) {
  if (const int rc = stack_call_pointers(scene, {{mesh, "null mesh table pointer"}, {lights, "null lights table pointer"}},
                                         origins, dirs, out, workspace))
    return rc;
  if (n_spheres < 0 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (mesh_words < RTX_MESH_HDR_WORDS || mesh_words > INT32_MAX)
    return rtx_fail(RTX_E_ARG, "mesh_words out of range (%d..2^31 - 1)", (int)RTX_MESH_HDR_WORDS);
  if (n_lights < 1 || n_lights > RTX_MAX_POINT_LIGHTS)
    return rtx_fail(RTX_E_ARG, "n_lights out of range (1..%d)", (int)RTX_MAX_POINT_LIGHTS);
  if (max_bounces < 0 || max_bounces > RTX_MESH_MAX_BOUNCES)
    return rtx_fail(RTX_E_ARG, "max_bounces out of range (0..%d): a mesh scene needs a finite cap",
                    (int)RTX_MESH_MAX_BOUNCES);
  // (the size is computed ahead of the checks on out_kind and n: the size function has no effects and gives 0 for n < 0)
  if (const int rc = stack_call_rays(out_kind, n, origin_stride, workspace_bytes,
                                     rtx_mesh_workspace_bytes(n, max_bounces), "rtx_mesh_workspace_bytes"))
    return rc;
  if (n == 0) return RTX_OK;
  MeshParams p{};
  p.scene = scene;
  p.nsph = n_spheres;
  p.mesh = mesh;
  p.mesh_words = mesh_words;
  p.lights = lights;
  p.n_lights = n_lights;
  stack_params(p, origins, origin_stride, dirs, n, max_bounces, out, out_kind, workspace, mesh_workers(n, max_bounces));
  const dim3 grid((unsigned)(p.n_workers / 64));
  if (uv) {
    hipLaunchKernelGGL(k_trace_mesh_uv, grid, dim3(64), 0, (hipStream_t)stream, p);
    return rtx_launched("k_trace_mesh_uv");
  }
  hipLaunchKernelGGL(k_trace_mesh, grid, dim3(64), 0, (hipStream_t)stream, p);
  return rtx_launched("k_trace_mesh");
}

}  // namespace

extern "C" int rtx_trace_mesh(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words,
                              const double* lights, int n_lights, const double* origins, int64_t origin_stride,
                              const double* dirs, int64_t n, int max_bounces, void* out, int out_kind, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return trace_mesh_call(scene, n_spheres, mesh, mesh_words, lights, n_lights, origins, origin_stride, dirs, n,
                         max_bounces, out, out_kind, workspace, workspace_bytes, stream, false);
}

extern "C" int rtx_trace_mesh_uv(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words,
                                 const double* lights, int n_lights, const double* origins, int64_t origin_stride,
                                 const double* dirs, int64_t n, int max_bounces, void* out, int out_kind,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  return trace_mesh_call(scene, n_spheres, mesh, mesh_words, lights, n_lights, origins, origin_stride, dirs, n,
                         max_bounces, out, out_kind, workspace, workspace_bytes, stream, true);
}
