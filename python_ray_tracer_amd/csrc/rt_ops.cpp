// rt_ops.cpp — the PyTorch-ROCm custom-op surface of the render path:
// TORCH_LIBRARY(rt, m) over the C ABI of librtx_hip.so (include/rtx_hip.h).
//
//   rt::render_tile   <- NumpyRenderer.get_ray_directions + raytrace_scene, fused, for one interleaved
//                        row tile of the scene camera's frame, or a run of part_run parts (a rank's
//                        weighted share: rtx_render_camera_sched) (base.py:91-141, shader.py:63-161)
//   rt::render_frames <- F x render_image_pipeline's render step in one launch (application.py:43-52)
//   rt::trace         <- NumpyRenderer.raytrace_scene(O, D, scene) on arbitrary rays (base.py:91-121)
//   rt::shade_hits    <- NumpyShader.create(shape, scene, O, D, t, renderer) (shader.py:63-112)
//   rt::intersect     <- NumpySphere.intersect (shape.py:28-51)
//   rt::quantize_u8   <- save_image's (255*clip(c,0,1)).astype(uint8) (base.py:143-151)
//   rt::assemble_rows <- the multi-GPU frame's row un-permute (application.render_frame_distributed),
//                        equal shares or weighted ones (root_run / run: rtx_assemble_runs)
//   rt::resolve_samples <- no counterpart: the box filter of a k x k supersampled frame
//                        (HipRenderer(samples=k), rtx_resolve_samples)
//   rt::primary_aovs, rt::primary_aovs_rays
//                     <- no counterpart: the primary hit's intermediates as render passes (depth, id,
//                        hits, position, normal, albedo, lit; rtx_primary_aovs), for a row tile of the
//                        camera's frame or for explicit rays
//   rt::trace_glass   <- no counterpart (shader.py:143, "TODO: VOIR TRANSMISSION"): raytrace_scene on explicit rays
//                        through a scene with solid glass spheres (rtx_trace_glass); allocates its workspace
//   rt::trace_lights  <- no counterpart (main.py, "TODO: use multiple lights"): raytrace_scene on explicit rays with
//                        every point light of a table (rtx_trace_lights); allocates its workspace
//   rt::trace_mesh    <- no counterpart (the reference's only Shape is the sphere): raytrace_scene on explicit rays
//                        through the spheres and the triangles of a mesh table (rtx_trace_mesh)
//   rt::mesh_build    <- no counterpart: the table of rt::trace_mesh made on the device from the meshes' arrays
//                        (rtx_mesh_build), value for value the host's meshes.mesh_table
//   rt::mesh_aovs     <- no counterpart: rt::primary_aovs_rays' passes for a scene with a mesh table, with the
//                        triangle's number, barycentrics and face normal (rtx_mesh_aovs)
//   rt::trace_mesh_uv <- no counterpart: rt::trace_mesh on a table with texture coordinates and texel blocks
//                        (rtx_trace_mesh_uv): image textures on meshes
//   rt::env_sample, rt::trace_lights_env, rt::trace_glass_env
//                     <- no counterpart (raytrace_scene adds nothing on a miss, base.py:100-121): the environment
//                        map's lookup alone, and the two kernels above with it for every ray that meets no shape
//   rt::occlusion     <- no counterpart: ambient occlusion and soft shadows of the primary hit, side x side
//                        any-hit rays per hit from the id, position and normal passes (rtx_occlusion)
//   rt::edge_mask, rt::sample_dirs, rt::resolve_scatter
//                     <- no counterpart: adaptive anti-aliasing (HipRenderer(samples=k, adaptive=True);
//                        rtx_edge_mask, rtx_sample_dirs, rtx_resolve_scatter), with the tensor-size checks
//                        the bare-pointer C ABI cannot make
//   rt::camera_rays   <- generalises get_ray_directions (base.py:123-141): the sample rays of a perspective
//                        camera (domain.PerspectiveCamera; rtx_camera_rays) for a row tile of its frame
//   rt::status        <- reads and clears the workspace's sticky RTX_ST_* flags
//   rt::comm_unique_id, rt::comm_init, rt::comm_destroy, rt::tiles_create, rt::tiles_submit,
//   rt::tiles_finish, rt::tiles_destroy
//                     <- the row-tiled multi-GPU frame of render_frame_distributed, one native call
//                        per frame and rank (rtx_tiles_*: render, RCCL gather to the root, assembly)
//   rt::workspace_bytes
//
// Conventions (those of a TORCH_CHECKed op): tensors must live on the GPU, be contiguous and have
// the documented dtype, or the op raises RuntimeError; every op runs under a device guard of its
// input's device (so the occupancy query, the CU count and the launch all see that device, whatever
// the current device is); outputs are allocated by the caching allocator on the input's device and
// returned; work is enqueued on the current HIP stream of that device and is asynchronous, except
// for the error channel below. The ops keep no state: the caller owns the workspace (zero-filled
// once, its counters left zeroed by every call) and the optional stats buffer (accumulated into).
//
// Error channel of the render ops (render_tile, render_frames, trace, shade_hits), check=True (the
// default), mirroring HipRenderer:
//   * before the first launch on a blob (and again after any in-place write to it), the blob's
//     header (magic, sphere count) is read back to the host — one small synchronous copy — and a
//     blob that disagrees with n_spheres raises RuntimeError (the kernel would refuse it,
//     RTX_ST_BAD_SCENE, and render nothing); later calls on the same blob do not synchronise;
//   * after a launch that can defer chains beyond the fast kernel's levels (max_bounces -1 or above
//     RTX_FAST_MAX_BOUNCES), the workspace's status word is read back (a synchronisation) and
//     cleared; RTX_ST_STACK_OVERFLOW raises RuntimeError("maximum recursion depth exceeded ...",
//     where HipRenderer raises RecursionError), any other flag raises RuntimeError.
// check=False keeps the op fully asynchronous (no host synchronisation): the caller reads and clears the
// flags later with rt::status(workspace).
#include <ATen/ATen.h>
#include <ATen/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <mutex>
#include <optional>
#include <tuple>
#include <vector>

#include "../../include/rtx_hip.h"

namespace {

void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == RTX_OK, what, " failed (", rc, "): ", rtx_last_error());
}

bool on_gpu(const at::Tensor& t) { return t.is_cuda(); }

void check_gpu(const at::Tensor& t, const char* name, at::ScalarType dtype) {
  TORCH_CHECK(on_gpu(t), name, " must be a GPU tensor, got one on ", t.device());
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_same_device(const at::Tensor& a, const at::Tensor& b, const char* name) {
  TORCH_CHECK(a.device() == b.device(), name, " is on ", b.device(), ", the scene on ", a.device());
}

void* stream_of(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check_scene_shape(const at::Tensor& scene, int64_t n_spheres) {
  TORCH_CHECK(scene.dim() == 1, "scene must be the 1-D packed blob (scene_pack.pack_scene)");
  TORCH_CHECK(n_spheres >= 1 && n_spheres <= RTX_MAX_SPHERES, "n_spheres out of range: ", n_spheres);
  TORCH_CHECK(scene.numel() >= RTX_HDR_WORDS + n_spheres * (RTX_GEOM_WORDS + RTX_MAT_WORDS),
              "scene blob too short for ", n_spheres, " spheres");
}

void check_scene(const at::Tensor& scene, int64_t n_spheres) {
  check_gpu(scene, "scene", at::kDouble);
  check_scene_shape(scene, n_spheres);
}

// Blobs whose headers passed, keyed by the tensor object (held weakly: a live entry cannot be a freed
// tensor's address reused by a new one), its data pointer, size and version counter (bumped by every
// in-place write): a blob is read back once per content version, not on every call, so repeated
// renders of one scene stay asynchronous.
struct CheckedBlob {
  c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl> impl{
      c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>::reclaim(
          c10::UndefinedTensorImpl::singleton())};
  const void* data = nullptr;
  int64_t numel = -1, version = -1, n_spheres = -1;
  bool matches(const at::Tensor& t, int64_t ns) const {
    return !impl.expired() && impl._unsafe_get_target() == t.unsafeGetTensorImpl() && data == t.data_ptr() &&
           numel == t.numel() && version == version_of(t) && n_spheres == ns;
  }
  // inference tensors keep no version counter (_version() throws): they are keyed on the object, its
  // storage and size alone (a blob rewritten in place under inference_mode is caught by the kernel's
  // own header test, RTX_ST_BAD_SCENE, which renders nothing)
  static int64_t version_of(const at::Tensor& t) { return t.is_inference() ? -2 : (int64_t)t._version(); }
};
constexpr int kCheckedBlobs = 32;
std::mutex g_checked_mu;
CheckedBlob g_checked[kCheckedBlobs];
int g_checked_next = 0;

// The header words of F blobs (rows of a [F, L] tensor, or one 1-D blob) against n_spheres: the
// host-side form of the kernel's RTX_ST_BAD_SCENE test (one synchronous copy of 2 words per blob,
// once per blob content: see CheckedBlob).
void check_headers(const at::Tensor& blobs, int64_t n_spheres) {
  {
    std::lock_guard<std::mutex> lock(g_checked_mu);
    for (const CheckedBlob& c : g_checked)
      if (c.matches(blobs, n_spheres)) return;
  }
  const at::Tensor head = (blobs.dim() == 1 ? blobs.narrow(0, 0, 2).unsqueeze(0) : blobs.narrow(1, 0, 2)).to(at::kCPU);
  const auto h = head.contiguous();
  const double* w = h.data_ptr<double>();
  for (int64_t f = 0; f < h.size(0); ++f) {
    TORCH_CHECK(w[2 * f + RTX_H_MAGIC] == RTX_MAGIC, "scene blob ", f, " is not a packed scene (bad magic)");
    TORCH_CHECK(w[2 * f + RTX_H_NSPH] == (double)n_spheres, "n_spheres=", n_spheres, " but scene blob ", f,
                " holds ", w[2 * f + RTX_H_NSPH], " spheres");
  }
  std::lock_guard<std::mutex> lock(g_checked_mu);
  CheckedBlob& c = g_checked[g_checked_next];
  g_checked_next = (g_checked_next + 1) % kCheckedBlobs;
  c.impl = c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>(blobs.getIntrusivePtr());
  c.data = blobs.data_ptr();
  c.numel = blobs.numel();
  c.version = CheckedBlob::version_of(blobs);
  c.n_spheres = n_spheres;
}

// After a launch: read and clear the sticky status flags when the launch can set them (chains
// deferred beyond the fast kernel's levels); raise on any.
void check_status_after(at::Tensor& ws, int64_t max_bounces) {
  if (max_bounces >= 0 && max_bounces <= RTX_FAST_MAX_BOUNCES) return;
  at::Tensor word = ws.narrow(0, 4 * RTX_WS_STATUS, 4);
  const int32_t st = word.view(at::kInt).item<int32_t>();
  if (st == 0) return;
  word.zero_();
  TORCH_CHECK(!(st & RTX_ST_STACK_OVERFLOW), "maximum recursion depth exceeded (reflection chain > ",
              RTX_UNBOUNDED_LEVELS, " levels; HipRenderer raises RecursionError)");
  TORCH_CHECK(!(st & RTX_ST_BAD_SCENE), "the scene blob's header disagrees with n_spheres: nothing was rendered");
  TORCH_CHECK(!(st & RTX_ST_UNRENDERED), "a render passed RTX_F_NO_GENERAL but deferred rays: pixels unwritten");
  TORCH_CHECK(false, "render status flags ", st, " (RTX_ST_LIST_OVERFLOW: deferred list full)");
}

// local rows of the run of `run` parts from `part` (tiling.n_local_rows)
int64_t tile_rows(int64_t height, int64_t row_block, int64_t n_parts, int64_t part, int64_t run = 1) {
  const int64_t cycle = row_block * n_parts, own = row_block * run, q = height / cycle,
                rem = height % cycle - part * row_block;
  return q * own + (rem < 0 ? 0 : rem > own ? own : rem);
}

void check_tile(int64_t width, int64_t height, int64_t row_block, int64_t n_parts, int64_t part, int64_t part_run) {
  TORCH_CHECK(width > 0 && height > 0 && row_block > 0 && n_parts > 0 && part >= 0 && part_run >= 1 &&
                  part + part_run <= n_parts,
              "bad frame/tile geometry (part ", part, ", part_run ", part_run, " of ", n_parts, " parts)");
}

// frames: 0 = a single output, F > 0 = [F, ...] outputs of F frames
at::Tensor new_output(const at::Tensor& like, int64_t n, int64_t rows, int64_t width, int64_t out_kind,
                      int64_t frames = 0) {
  auto o = like.options();
  std::vector<int64_t> shape;
  if (frames > 0) shape.push_back(frames);
  if (out_kind == RTX_OUT_F32_SOA || out_kind == RTX_OUT_F64_SOA) {
    shape.push_back(3);
    shape.push_back(n);
    return at::empty(shape, o.dtype(out_kind == RTX_OUT_F32_SOA ? at::kFloat : at::kDouble));
  }
  TORCH_CHECK(out_kind == RTX_OUT_U8_HWC, "bad out_kind ", out_kind);
  if (rows >= 0) {
    shape.push_back(rows);
    shape.push_back(width);
  } else {
    shape.push_back(n);
  }
  shape.push_back(3);
  return at::empty(shape, o.dtype(at::kByte));
}

void check_workspace(const at::Tensor& ws, const at::Tensor& scene, int64_t n, int64_t max_bounces) {
  check_gpu(ws, "workspace", at::kByte);
  check_same_device(scene, ws, "workspace");
  const size_t need = rtx_workspace_bytes(n, (int)max_bounces);
  TORCH_CHECK((size_t)ws.numel() >= need, "workspace too small: ", ws.numel(), " < ", need,
              " bytes (rt::workspace_bytes)");
}

uint64_t* stats_ptr(const std::optional<at::Tensor>& stats, const at::Tensor& scene) {
  if (!stats.has_value()) return nullptr;
  check_gpu(*stats, "stats", at::kLong);
  check_same_device(scene, *stats, "stats");
  TORCH_CHECK(stats->numel() >= RTX_S_WORDS, "stats needs ", RTX_S_WORDS, " int64 words");
  return (uint64_t*)stats->data_ptr();
}

void check_bounces(int64_t max_bounces) {
  TORCH_CHECK(max_bounces >= RTX_UNBOUNDED, "max_bounces must be >= 0, or -1 (unbounded)");
}

// origins [3] (shared, stride 0) or [3, n]; returns the stride
int64_t check_rays(const at::Tensor& scene, const at::Tensor& origins, const at::Tensor& dirs) {
  check_gpu(origins, "origins", at::kDouble);
  check_gpu(dirs, "dirs", at::kDouble);
  check_same_device(scene, origins, "origins");
  check_same_device(scene, dirs, "dirs");
  TORCH_CHECK(dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be [3, n]");
  const int64_t n = dirs.size(1);
  if (origins.dim() == 1) {
    TORCH_CHECK(origins.numel() == 3, "a shared origin is 3 doubles");
    return 0;
  }
  TORCH_CHECK(origins.dim() == 2 && origins.size(0) == 3 && origins.size(1) == n, "origins must be [3] or [3, n]");
  return n;
}

// ---- ops ---------------------------------------------------------------------------------------

at::Tensor render_tile(const at::Tensor& scene, int64_t n_spheres, int64_t width, int64_t height, int64_t row_block,
                       int64_t n_parts, int64_t part, int64_t max_bounces, int64_t out_kind, at::Tensor& workspace,
                       const std::optional<at::Tensor>& stats, bool check, int64_t part_run) {
  check_scene(scene, n_spheres);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  check_tile(width, height, row_block, n_parts, part, part_run);
  check_bounces(max_bounces);
  const int64_t rows = tile_rows(height, row_block, n_parts, part, part_run);
  const int64_t n = width * rows;
  check_workspace(workspace, scene, n, max_bounces);
  if (check) check_headers(scene, n_spheres);
  at::Tensor out = new_output(scene, n, rows, width, out_kind);
  // a run of parts (a rank's weighted share, distributed.ROOT_SHARES) in one launch; bottom-up order
  check_rc(rtx_render_camera_sched(scene.data_ptr<double>(), (int)n_spheres, (int)width, (int)height, (int)row_block,
                                   (int)n_parts, (int)part, (int)part_run, (int)rows, (int)max_bounces, out.data_ptr(),
                                   (int)out_kind, workspace.data_ptr(), (size_t)workspace.numel(),
                                   stats_ptr(stats, scene), stream_of(scene), 0u, nullptr, nullptr, nullptr),
           "rtx_render_camera_sched");
  if (check) check_status_after(workspace, max_bounces);
  return out;
}

at::Tensor render_frames(const at::Tensor& scenes, int64_t n_spheres, int64_t width, int64_t height,
                         int64_t max_bounces, int64_t out_kind, at::Tensor& workspace,
                         const std::optional<at::Tensor>& stats, bool check) {
  check_gpu(scenes, "scenes", at::kDouble);
  TORCH_CHECK(scenes.dim() == 2, "scenes must be [F, L]: one packed blob per frame (rows padded to one length)");
  const int64_t F = scenes.size(0);
  TORCH_CHECK(F >= 1 && F <= 65535, "1 to 65535 frames per launch, got ", F);
  TORCH_CHECK(n_spheres >= 1 && n_spheres <= RTX_MAX_SPHERES, "n_spheres out of range: ", n_spheres);
  TORCH_CHECK(scenes.size(1) >= RTX_HDR_WORDS + n_spheres * (RTX_GEOM_WORDS + RTX_MAT_WORDS),
              "scene blobs too short for ", n_spheres, " spheres");
  const at::OptionalDeviceGuard guard(at::device_of(scenes));
  TORCH_CHECK(width > 0 && height > 0, "bad frame geometry");
  check_bounces(max_bounces);
  const int64_t n = width * height;
  check_workspace(workspace, scenes, F * n, max_bounces);
  if (check) check_headers(scenes, n_spheres);
  at::Tensor out = new_output(scenes, n, height, width, out_kind, F);
  check_rc(rtx_render_frames(scenes.data_ptr<double>(), scenes.stride(0), (int)F, (int)n_spheres, (int)width,
                             (int)height, (int)max_bounces, out.data_ptr(), (int)out_kind, workspace.data_ptr(),
                             (size_t)workspace.numel(), stats_ptr(stats, scenes), stream_of(scenes)),
           "rtx_render_frames");
  if (check) check_status_after(workspace, max_bounces);
  return out;
}

at::Tensor trace(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& origins, const at::Tensor& dirs,
                 int64_t max_bounces, int64_t out_kind, at::Tensor& workspace, const std::optional<at::Tensor>& stats,
                 bool check) {
  check_scene(scene, n_spheres);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  const int64_t stride = check_rays(scene, origins, dirs);
  const int64_t n = dirs.size(1);
  check_bounces(max_bounces);
  TORCH_CHECK(out_kind == RTX_OUT_F32_SOA || out_kind == RTX_OUT_F64_SOA, "trace returns colour: out_kind 0 or 1");
  check_workspace(workspace, scene, n, max_bounces);
  if (check) check_headers(scene, n_spheres);
  at::Tensor out = new_output(scene, n, -1, 0, out_kind);
  check_rc(rtx_trace_rays(scene.data_ptr<double>(), (int)n_spheres, origins.data_ptr<double>(), stride,
                          dirs.data_ptr<double>(), n, (int)max_bounces, out.data_ptr(), (int)out_kind,
                          workspace.data_ptr(), (size_t)workspace.numel(), stats_ptr(stats, scene), stream_of(scene)),
           "rtx_trace_rays");
  if (check) check_status_after(workspace, max_bounces);
  return out;
}

at::Tensor shade_hits(const at::Tensor& scene, int64_t n_spheres, int64_t shape, const at::Tensor& origins,
                      const at::Tensor& dirs, const at::Tensor& t, int64_t max_bounces, int64_t out_kind,
                      at::Tensor& workspace, const std::optional<at::Tensor>& stats, bool check) {
  check_scene(scene, n_spheres);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  const int64_t stride = check_rays(scene, origins, dirs);
  const int64_t n = dirs.size(1);
  check_gpu(t, "t", at::kDouble);
  check_same_device(scene, t, "t");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == n, "t must be [n]: one hit distance per ray");
  TORCH_CHECK(shape >= 0 && shape < n_spheres, "shape index out of range: ", shape,
              " (NumpyShader.create raises ValueError for a shape not in scene.shapes)");
  check_bounces(max_bounces);
  TORCH_CHECK(out_kind == RTX_OUT_F32_SOA || out_kind == RTX_OUT_F64_SOA, "shade_hits returns colour: out_kind 0 or 1");
  check_workspace(workspace, scene, n, max_bounces);
  if (check) check_headers(scene, n_spheres);
  at::Tensor out = new_output(scene, n, -1, 0, out_kind);
  check_rc(rtx_shade_hits(scene.data_ptr<double>(), (int)n_spheres, (int)shape, origins.data_ptr<double>(), stride,
                          dirs.data_ptr<double>(), t.data_ptr<double>(), n, (int)max_bounces, out.data_ptr(),
                          (int)out_kind, workspace.data_ptr(), (size_t)workspace.numel(), stats_ptr(stats, scene),
                          stream_of(scene)),
           "rtx_shade_hits");
  if (check) check_status_after(workspace, max_bounces);
  return out;
}

at::Tensor intersect(const at::Tensor& sphere, const at::Tensor& origins, const at::Tensor& dirs) {
  check_gpu(sphere, "sphere", at::kDouble);
  TORCH_CHECK(sphere.numel() >= RTX_GEOM_WORDS, "sphere: ", RTX_GEOM_WORDS, " geometry words");
  const at::OptionalDeviceGuard guard(at::device_of(sphere));
  const int64_t stride = check_rays(sphere, origins, dirs);
  const int64_t n = dirs.size(1);
  at::Tensor t = at::empty({n}, dirs.options());
  check_rc(rtx_sphere_intersect(sphere.data_ptr<double>(), origins.data_ptr<double>(), stride,
                                dirs.data_ptr<double>(), n, t.data_ptr<double>(), stream_of(dirs)),
           "rtx_sphere_intersect");
  return t;
}

at::Tensor quantize_u8(const at::Tensor& color) {
  TORCH_CHECK(on_gpu(color) && color.is_contiguous(), "color must be a contiguous GPU tensor");
  TORCH_CHECK(color.dim() == 2 && color.size(0) == 3, "color must be [3, n]");
  int kind;
  if (color.scalar_type() == at::kFloat) {
    kind = RTX_OUT_F32_SOA;
  } else {
    TORCH_CHECK(color.scalar_type() == at::kDouble, "color must be float32 or float64");
    kind = RTX_OUT_F64_SOA;
  }
  const at::OptionalDeviceGuard guard(at::device_of(color));
  const int64_t n = color.size(1);
  at::Tensor out = at::empty({n, 3}, color.options().dtype(at::kByte));
  check_rc(rtx_quantize_u8(color.data_ptr(), kind, n, (uint8_t*)out.data_ptr(), stream_of(color)), "rtx_quantize_u8");
  return out;
}

at::Tensor assemble_out(const at::Tensor& tiles, int64_t width, int64_t height, int64_t out_kind) {
  TORCH_CHECK(tiles.is_contiguous() && tiles.dim() == 2, "tiles must be a contiguous [P, L] GPU tensor");
  if (out_kind == RTX_OUT_U8_HWC) {
    TORCH_CHECK(tiles.scalar_type() == at::kByte, "uint8 tiles for out_kind 2");
    return at::empty({height, width, 3}, tiles.options());
  }
  TORCH_CHECK((out_kind == RTX_OUT_F32_SOA && tiles.scalar_type() == at::kFloat) ||
                  (out_kind == RTX_OUT_F64_SOA && tiles.scalar_type() == at::kDouble),
              "tiles dtype does not match out_kind");
  return at::empty({3, height * width}, tiles.options());
}

at::Tensor assemble_rows(const at::Tensor& tiles, int64_t width, int64_t height, int64_t row_block, int64_t out_kind,
                         int64_t root_run, int64_t run) {
  TORCH_CHECK(on_gpu(tiles), "tiles must be a contiguous [P, L] GPU tensor");
  TORCH_CHECK(root_run >= 1 && run >= 1, "root_run and run must be >= 1");
  const at::OptionalDeviceGuard guard(at::device_of(tiles));
  at::Tensor out = assemble_out(tiles, width, height, out_kind);
  // rank i's tile at row i (its run of parts: rank 0 parts [0, root_run), rank i >= 1 the run
  // [root_run + (i - 1) run, + run) of the root_run + (P - 1) run interleave); equal runs of one
  // part are rtx_assemble_rows
  check_rc(rtx_assemble_runs(tiles.data_ptr(), tiles.stride(0) * (int64_t)tiles.element_size(), (int)tiles.size(0),
                             (int)root_run, (int)run, (int)width, (int)height, (int)row_block, (int)out_kind,
                             out.data_ptr(), stream_of(tiles)),
           "rtx_assemble_runs");
  return out;
}

// samples [3, k*rows*k*width] or [F, 3, ...] float64; returns the frame's shape and the frame count
// (0: unbatched). Shared by the kernel and its Meta form.
int64_t check_samples_shape(const at::Tensor& samples, int64_t k, int64_t width, int64_t rows, int64_t out_kind) {
  TORCH_CHECK(k >= 1 && k <= 8, "k (samples per pixel side) must be in 1..8, got ", k);
  TORCH_CHECK(width > 0 && rows > 0, "bad frame geometry (width ", width, ", rows ", rows, ")");
  TORCH_CHECK(out_kind == RTX_OUT_F32_SOA || out_kind == RTX_OUT_F64_SOA || out_kind == RTX_OUT_U8_HWC,
              "bad out_kind ", out_kind);
  TORCH_CHECK(samples.scalar_type() == at::kDouble, "samples must be ", at::kDouble, ", got ", samples.scalar_type());
  TORCH_CHECK((samples.dim() == 2 || samples.dim() == 3) && samples.size(-2) == 3,
              "samples must be [3, k*rows*k*width] or [F, 3, k*rows*k*width]");
  const int64_t frames = samples.dim() == 3 ? samples.size(0) : 0;
  TORCH_CHECK(samples.dim() == 2 || frames >= 1, "samples holds no frame");
  TORCH_CHECK(width <= INT32_MAX && rows <= INT32_MAX && frames <= INT32_MAX &&
                  (double)(k * k) * (double)width * (double)rows * (double)(frames ? frames : 1) < 2147483648.0,
              "k*k*width*rows*frames must stay below 2^31");
  const int64_t ns = k * rows * k * width;
  TORCH_CHECK(samples.size(-1) == ns, "samples holds ", samples.size(-1), " samples per plane, but k=", k, ", width=",
              width, ", rows=", rows, " need ", ns, " (", (frames ? frames : 1) * 3 * ns, " in all, got ",
              samples.numel(), ")");
  return frames;
}

at::Tensor resolve_samples(const at::Tensor& samples, int64_t k, int64_t width, int64_t rows, int64_t out_kind) {
  check_gpu(samples, "samples", at::kDouble);
  const int64_t frames = check_samples_shape(samples, k, width, rows, out_kind);
  const at::OptionalDeviceGuard guard(at::device_of(samples));
  at::Tensor out = new_output(samples, rows * width, rows, width, out_kind, frames);
  check_rc(rtx_resolve_samples(samples.data_ptr<double>(), (int)k, (int)width, (int)rows, (int)(frames ? frames : 1),
                               out.data_ptr(), (int)out_kind, stream_of(samples)),
           "rtx_resolve_samples");
  return out;
}

// ---- primary-hit render passes (rtx_primary_aovs) ----------------------------------------------
// `passes`: a mask of RTX_AOV_* bits; the result holds one tensor per set bit, in bit order: depth
// float64 [n], id int32 [n], hits int32 [n], position / normal / albedo float64 [3, n], lit uint8 [n].
// Shared by the kernels and their Meta forms.
std::vector<at::Tensor> new_aovs(const at::Tensor& like, int64_t n, int64_t passes) {
  TORCH_CHECK(passes > 0 && (passes & ~(int64_t)RTX_AOV_ALL) == 0, "passes must be a non-empty mask of RTX_AOV_* bits (1..",
              (int)RTX_AOV_ALL, "), got ", passes);
  const auto o = like.options();
  std::vector<at::Tensor> out;
  if (passes & RTX_AOV_DEPTH) out.push_back(at::empty({n}, o.dtype(at::kDouble)));
  if (passes & RTX_AOV_ID) out.push_back(at::empty({n}, o.dtype(at::kInt)));
  if (passes & RTX_AOV_HITS) out.push_back(at::empty({n}, o.dtype(at::kInt)));
  if (passes & RTX_AOV_POSITION) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_AOV_NORMAL) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_AOV_ALBEDO) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_AOV_LIT) out.push_back(at::empty({n}, o.dtype(at::kByte)));
  return out;
}

// the seven output pointers of `out` (new_aovs(passes)), null where a pass is not requested
struct AovPtrs {
  void* p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  AovPtrs(const std::vector<at::Tensor>& out, int64_t passes) {
    size_t k = 0;
    for (int b = 0; b < 7; ++b)
      if (passes & (int64_t(1) << b)) p[b] = out[k++].data_ptr();
  }
};

std::vector<at::Tensor> primary_aovs(const at::Tensor& scene, int64_t n_spheres, int64_t width, int64_t height,
                                     int64_t row_block, int64_t n_parts, int64_t part, int64_t part_run,
                                     int64_t passes, bool check) {
  check_scene(scene, n_spheres);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  check_tile(width, height, row_block, n_parts, part, part_run);
  const int64_t rows = tile_rows(height, row_block, n_parts, part, part_run);
  std::vector<at::Tensor> out = new_aovs(scene, width * rows, passes);
  if (check) check_headers(scene, n_spheres);
  if (rows == 0) return out;  // an empty tile: nothing to launch (an empty tensor's pointer may be null)
  const AovPtrs a(out, passes);
  check_rc(rtx_primary_aovs(scene.data_ptr<double>(), (int)n_spheres, (int)width, (int)height, (int)row_block,
                            (int)n_parts, (int)part, (int)part_run, (int)rows, (double*)a.p[0], (int32_t*)a.p[1],
                            (int32_t*)a.p[2], (double*)a.p[3], (double*)a.p[4], (double*)a.p[5], (uint8_t*)a.p[6],
                            stream_of(scene)),
           "rtx_primary_aovs");
  return out;
}

std::vector<at::Tensor> primary_aovs_rays(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& origins,
                                          const at::Tensor& dirs, int64_t passes, bool check) {
  check_scene(scene, n_spheres);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  const int64_t stride = check_rays(scene, origins, dirs);
  const int64_t n = dirs.size(1);
  std::vector<at::Tensor> out = new_aovs(scene, n, passes);
  if (check) check_headers(scene, n_spheres);
  if (n == 0) return out;
  const AovPtrs a(out, passes);
  check_rc(rtx_primary_aovs_rays(scene.data_ptr<double>(), (int)n_spheres, origins.data_ptr<double>(), stride,
                                 dirs.data_ptr<double>(), n, (double*)a.p[0], (int32_t*)a.p[1], (int32_t*)a.p[2],
                                 (double*)a.p[3], (double*)a.p[4], (double*)a.p[5], (uint8_t*)a.p[6],
                                 stream_of(scene)),
           "rtx_primary_aovs_rays");
  return out;
}

// ---- adaptive anti-aliasing (rtx_edge_mask, rtx_sample_dirs, rtx_resolve_scatter) ---------------
// The C ABI takes bare pointers: the tensor sizes are checked here. Shared by the kernels and their
// Meta forms.
void check_frame(int64_t width, int64_t height) {
  TORCH_CHECK(width > 0 && height > 0 && (double)width * (double)height < 2147483648.0,
              "bad frame geometry (width ", width, ", height ", height, "): positive, width*height below 2^31");
}

void check_edge_inputs(const at::Tensor& color, const at::Tensor& id, const at::Tensor& hits, const at::Tensor& lit,
                       int64_t width, int64_t height, double contrast) {
  check_frame(width, height);
  TORCH_CHECK(contrast >= 0.0, "contrast must be >= 0 (inf: no colour test), got ", contrast);
  const int64_t n = width * height;
  TORCH_CHECK(color.scalar_type() == at::kDouble && color.dim() == 2 && color.size(0) == 3 && color.size(1) == n,
              "color must be ", at::kDouble, " [3, width*height]");
  TORCH_CHECK(id.scalar_type() == at::kInt && id.dim() == 1 && id.size(0) == n, "id must be ", at::kInt,
              " [width*height]");
  TORCH_CHECK(hits.scalar_type() == at::kInt && hits.dim() == 1 && hits.size(0) == n, "hits must be ", at::kInt,
              " [width*height]");
  TORCH_CHECK(lit.scalar_type() == at::kByte && lit.dim() == 1 && lit.size(0) == n, "lit must be ", at::kByte,
              " [width*height]");
}

at::Tensor edge_mask(const at::Tensor& color, const at::Tensor& id, const at::Tensor& hits, const at::Tensor& lit,
                     int64_t width, int64_t height, double contrast) {
  check_gpu(color, "color", at::kDouble);
  check_gpu(id, "id", at::kInt);
  check_gpu(hits, "hits", at::kInt);
  check_gpu(lit, "lit", at::kByte);
  check_same_device(color, id, "id");
  check_same_device(color, hits, "hits");
  check_same_device(color, lit, "lit");
  check_edge_inputs(color, id, hits, lit, width, height, contrast);
  const at::OptionalDeviceGuard guard(at::device_of(color));
  at::Tensor mask = at::empty({width * height}, color.options().dtype(at::kByte));
  check_rc(rtx_edge_mask(color.data_ptr<double>(), id.data_ptr<int32_t>(), hits.data_ptr<int32_t>(),
                         lit.data_ptr<uint8_t>(), (int)width, (int)height, contrast, mask.data_ptr<uint8_t>(),
                         stream_of(color)),
           "rtx_edge_mask");
  return mask;
}

// pixels int32 [n_flagged]; returns n_flagged
int64_t check_pixels(const at::Tensor& pixels, int64_t k, int64_t width, int64_t height) {
  TORCH_CHECK(k >= 1 && k <= 8, "k (samples per pixel side) must be in 1..8, got ", k);
  check_frame(width, height);
  TORCH_CHECK(pixels.scalar_type() == at::kInt && pixels.dim() == 1, "pixels must be ", at::kInt, " [n_flagged]");
  TORCH_CHECK((double)pixels.size(0) * (double)(k * k) < 2147483648.0, "n_flagged*k*k must stay below 2^31");
  return pixels.size(0);
}

at::Tensor sample_dirs(const at::Tensor& sample_scene, int64_t k, int64_t width, int64_t height,
                       const at::Tensor& pixels) {
  check_gpu(sample_scene, "sample_scene", at::kDouble);
  check_gpu(pixels, "pixels", at::kInt);
  check_same_device(sample_scene, pixels, "pixels");
  TORCH_CHECK(sample_scene.dim() == 1 && sample_scene.numel() >= RTX_HDR_WORDS,
              "sample_scene must be a 1-D packed scene (at least its header)");
  const int64_t nf = check_pixels(pixels, k, width, height);
  const at::OptionalDeviceGuard guard(at::device_of(sample_scene));
  at::Tensor dirs = at::empty({3, nf * k * k}, sample_scene.options());
  if (nf == 0) return dirs;  // (an empty tensor's pointer may be null)
  check_rc(rtx_sample_dirs(sample_scene.data_ptr<double>(), (int)k, (int)width, (int)height,
                           pixels.data_ptr<int32_t>(), (int)nf, dirs.data_ptr<double>(), stream_of(sample_scene)),
           "rtx_sample_dirs");
  return dirs;
}

void check_scatter(const at::Tensor& samples, int64_t k, const at::Tensor& pixels, int64_t width, int64_t height,
                   const at::Tensor& out, int64_t out_kind) {
  const int64_t nf = check_pixels(pixels, k, width, height);
  TORCH_CHECK(samples.scalar_type() == at::kDouble && samples.dim() == 2 && samples.size(0) == 3 &&
                  samples.size(1) == nf * k * k,
              "samples must be ", at::kDouble, " [3, n_flagged*k*k]");
  const int64_t n = width * height;
  if (out_kind == RTX_OUT_U8_HWC) {
    TORCH_CHECK(out.scalar_type() == at::kByte && out.numel() == 3 * n, "out must be ", at::kByte,
                " [height, width, 3] for out_kind 2");
  } else {
    TORCH_CHECK(out_kind == RTX_OUT_F32_SOA || out_kind == RTX_OUT_F64_SOA, "bad out_kind ", out_kind);
    const at::ScalarType want = out_kind == RTX_OUT_F32_SOA ? at::kFloat : at::kDouble;
    TORCH_CHECK(out.scalar_type() == want && out.dim() == 2 && out.size(0) == 3 && out.size(1) == n, "out must be ",
                want, " [3, width*height] for out_kind ", out_kind);
  }
}

void resolve_scatter(const at::Tensor& samples, int64_t k, const at::Tensor& pixels, int64_t width, int64_t height,
                     at::Tensor& out, int64_t out_kind) {
  check_gpu(samples, "samples", at::kDouble);
  check_gpu(pixels, "pixels", at::kInt);
  TORCH_CHECK(on_gpu(out) && out.is_contiguous(), "out must be a contiguous GPU tensor");
  check_same_device(samples, pixels, "pixels");
  check_same_device(samples, out, "out");
  check_scatter(samples, k, pixels, width, height, out, out_kind);
  if (pixels.size(0) == 0) return;
  const at::OptionalDeviceGuard guard(at::device_of(samples));
  check_rc(rtx_resolve_scatter(samples.data_ptr<double>(), (int)k, pixels.data_ptr<int32_t>(), (int)pixels.size(0),
                               (int)width, (int)height, out.data_ptr(), (int)out_kind, stream_of(samples)),
           "rtx_resolve_scatter");
}

// ---- a perspective camera's rays (rtx_camera_rays) -----------------------------------------------
// cam: the camera record, a HOST float64 tensor of RTX_CAM_WORDS words (it travels as a kernel
// argument); lens: the device lens table [2, k*k] or None. Returns (origins or None, dirs): origins
// [3, n] when a lens table is given, else None (a pinhole's rays share the origin cam[RTX_C_EYE ..]).
// The sizes of both tensors are checked here: the C ABI takes bare pointers. Returns the rays of a
// plane, n. Shared by the kernel and its Meta form.
int64_t check_camera_rays(const at::Tensor& cam, const std::optional<at::Tensor>& lens, int64_t k, int64_t width,
                          int64_t height, int64_t row_block, int64_t n_parts, int64_t part, int64_t part_run) {
  TORCH_CHECK(cam.scalar_type() == at::kDouble && cam.dim() == 1 && cam.numel() == RTX_CAM_WORDS,
              "cam must be the camera record: ", at::kDouble, " [", (int)RTX_CAM_WORDS, "], got ", cam.scalar_type(), " ",
              cam.sizes());
  TORCH_CHECK(k >= 1 && k <= 8, "k (samples per pixel side) must be in 1..8, got ", k);
  check_tile(width, height, row_block, n_parts, part, part_run);
  TORCH_CHECK(k * width < 2147483648LL && k * height < 2147483648LL, "k*width and k*height must stay below 2^31");
  const int64_t rows = tile_rows(height, row_block, n_parts, part, part_run);
  TORCH_CHECK((double)(k * k) * (double)width * (double)rows < 2147483648.0,
              "k*k*width*rows must stay below 2^31 rays");
  if (lens.has_value()) {
    TORCH_CHECK(lens->scalar_type() == at::kDouble && lens->numel() == 2 * k * k, "lens must be ", at::kDouble,
                " [2, k*k] = ", 2 * k * k, " words, got ", lens->scalar_type(), " with ", lens->numel());
  }
  return k * k * width * rows;
}

std::tuple<std::optional<at::Tensor>, at::Tensor> camera_rays(const at::Tensor& cam,
                                                             const std::optional<at::Tensor>& lens, int64_t k,
                                                             int64_t width, int64_t height, int64_t row_block,
                                                             int64_t n_parts, int64_t part, int64_t part_run) {
  TORCH_CHECK(cam.device().is_cpu(), "cam must be a host tensor (the record is a kernel argument), got one on ",
              cam.device());
  TORCH_CHECK(cam.is_contiguous(), "cam must be contiguous");
  if (lens.has_value()) check_gpu(*lens, "lens", at::kDouble);
  const int64_t n = check_camera_rays(cam, lens, k, width, height, row_block, n_parts, part, part_run);
  const int64_t rows = tile_rows(height, row_block, n_parts, part, part_run);
  // without a lens table no argument names a device: the rays land on the current one
  const at::Device dev = lens.has_value() ? lens->device() : at::Device(at::kCUDA, c10::hip::current_device());
  const at::OptionalDeviceGuard guard(dev);
  const auto opts = at::TensorOptions().dtype(at::kDouble).device(dev);
  std::optional<at::Tensor> origins;
  if (lens.has_value()) origins = at::empty({3, n}, opts);
  at::Tensor dirs = at::empty({3, n}, opts);
  if (n == 0) return {origins, dirs};  // (an empty tensor's pointer may be null)
  check_rc(rtx_camera_rays(cam.data_ptr<double>(), lens.has_value() ? lens->data_ptr<double>() : nullptr, (int)k,
                           (int)width, (int)height, (int)row_block, (int)n_parts, (int)part, (int)part_run, (int)rows,
                           origins.has_value() ? origins->data_ptr<double>() : nullptr, dirs.data_ptr<double>(),
                           c10::hip::getCurrentHIPStream(dev.index()).stream()),
           "rtx_camera_rays");
  return {origins, dirs};
}

// ---- occlusion passes (rtx_occlusion) -------------------------------------------------------------
// `passes`: a mask of RTX_OCC_* bits; the result holds one float32 [n] tensor per set bit, in bit
// order (ao, soft_lit). The C ABI takes bare pointers: the tensor sizes are checked here. Returns n.
// Shared by the kernel and its Meta form.
int64_t check_occlusion(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& id, const at::Tensor& position,
                        const at::Tensor& normal, const at::Tensor& table, const at::Tensor& rot,
                        double max_distance, double light_radius, int64_t passes) {
  check_scene_shape(scene, n_spheres);
  TORCH_CHECK(passes > 0 && (passes & ~(int64_t)RTX_OCC_ALL) == 0,
              "passes must be a non-empty mask of RTX_OCC_* bits (1..", (int)RTX_OCC_ALL, "), got ", passes);
  TORCH_CHECK(id.scalar_type() == at::kInt && id.dim() == 1, "id must be ", at::kInt, " [n], got ", id.scalar_type(),
              " ", id.sizes());
  const int64_t n = id.size(0);
  TORCH_CHECK(position.scalar_type() == at::kDouble && position.dim() == 2 && position.size(0) == 3 &&
                  position.size(1) == n,
              "position must be ", at::kDouble, " [3, n] with n = ", n, ", got ", position.scalar_type(), " ",
              position.sizes());
  TORCH_CHECK(normal.scalar_type() == at::kDouble && normal.dim() == 2 && normal.size(0) == 3 && normal.size(1) == n,
              "normal must be ", at::kDouble, " [3, n] with n = ", n, ", got ", normal.scalar_type(), " ",
              normal.sizes());
  TORCH_CHECK(table.scalar_type() == at::kDouble && table.dim() == 2 && table.size(0) == 3,
              "table must be the hemisphere table: ", at::kDouble, " [3, side*side], got ", table.scalar_type(), " ",
              table.sizes());
  int64_t side = 0;
  while (side * side < table.size(1)) ++side;
  TORCH_CHECK(side >= 1 && side <= 8 && side * side == table.size(1),
              "table must hold side*side samples with side in 1..8, got ", table.size(1));
  TORCH_CHECK(rot.scalar_type() == at::kDouble && rot.dim() == 2 && rot.size(0) == 2 && rot.size(1) == 64,
              "rot must be the rotation table: ", at::kDouble, " [2, 64], got ", rot.scalar_type(), " ", rot.sizes());
  TORCH_CHECK(max_distance > 0.0 && max_distance <= 1.0e39, "max_distance must lie in (0, 1e39], got ", max_distance);
  TORCH_CHECK(light_radius >= 0.0 && light_radius <= 1.7976931348623157e308,
              "light_radius must be finite and not negative, got ", light_radius);
  return n;
}

std::vector<at::Tensor> new_occlusion(const at::Tensor& like, int64_t n, int64_t passes) {
  std::vector<at::Tensor> out;
  for (int b = 0; b < 2; ++b)
    if (passes & (int64_t(1) << b)) out.push_back(at::empty({n}, like.options().dtype(at::kFloat)));
  return out;
}

std::vector<at::Tensor> occlusion(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& id,
                                  const at::Tensor& position, const at::Tensor& normal, const at::Tensor& table,
                                  const at::Tensor& rot, double max_distance, double light_radius, int64_t passes,
                                  bool check) {
  check_gpu(scene, "scene", at::kDouble);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  const struct { const at::Tensor& t; const char* name; at::ScalarType dtype; } in[] = {
      {id, "id", at::kInt}, {position, "position", at::kDouble}, {normal, "normal", at::kDouble},
      {table, "table", at::kDouble}, {rot, "rot", at::kDouble}};
  for (const auto& a : in) {
    check_gpu(a.t, a.name, a.dtype);
    check_same_device(scene, a.t, a.name);
  }
  const int64_t n = check_occlusion(scene, n_spheres, id, position, normal, table, rot, max_distance, light_radius,
                                    passes);
  std::vector<at::Tensor> out = new_occlusion(scene, n, passes);
  if (check) check_headers(scene, n_spheres);
  if (n == 0) return out;  // (an empty tensor's pointer may be null)
  int64_t side = 0;
  while (side * side < table.size(1)) ++side;
  float* ptr[2] = {nullptr, nullptr};
  size_t k = 0;
  for (int b = 0; b < 2; ++b)
    if (passes & (int64_t(1) << b)) ptr[b] = out[k++].data_ptr<float>();
  check_rc(rtx_occlusion(scene.data_ptr<double>(), (int)n_spheres, id.data_ptr<int32_t>(), position.data_ptr<double>(),
                         normal.data_ptr<double>(), n, table.data_ptr<double>(), (int)side, rot.data_ptr<double>(),
                         max_distance, light_radius, ptr[0], ptr[1], stream_of(scene)),
           "rtx_occlusion");
  return out;
}

// ---- the kernels with a stack of pending rays: transmission (rtx_trace_glass), several point lights
// (rtx_trace_lights), triangle meshes (rtx_trace_mesh, rtx_trace_mesh_uv), each also under an environment ----
// Shapes and ranges of their arguments, shared by the kernels and their Meta forms.
// dirs [3, n], origins [3] or [3, n], the bounce cap (0..cap: a `noun` scene needs one) and out_kind: returns n.
int64_t check_rays_args(const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t cap,
                        const char* noun, int64_t out_kind) {
  TORCH_CHECK(dirs.scalar_type() == at::kDouble && dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be ", at::kDouble,
              " [3, n], got ", dirs.scalar_type(), " ", dirs.sizes());
  const int64_t n = dirs.size(1);
  TORCH_CHECK(origins.scalar_type() == at::kDouble &&
                  ((origins.dim() == 1 && origins.numel() == 3) ||
                   (origins.dim() == 2 && origins.size(0) == 3 && origins.size(1) == n)),
              "origins must be ", at::kDouble, " [3] (shared) or [3, n] with n = ", n, ", got ", origins.scalar_type(),
              " ", origins.sizes());
  TORCH_CHECK(max_bounces >= 0 && max_bounces <= cap, "max_bounces must lie in 0..", (int)cap, " (a ", noun,
              " scene needs a finite cap), got ", max_bounces);
  TORCH_CHECK(out_kind == RTX_OUT_F32_SOA || out_kind == RTX_OUT_F64_SOA || out_kind == RTX_OUT_U8_HWC,
              "bad out_kind ", out_kind);
  return n;
}

void check_lights_table(const at::Tensor& lights) {
  TORCH_CHECK(lights.scalar_type() == at::kDouble && lights.dim() == 2 && lights.size(1) == 6 &&
                  lights.size(0) >= 1 && lights.size(0) <= RTX_MAX_POINT_LIGHTS,
              "lights must be ", at::kDouble, " [L, 6] with L in 1..", (int)RTX_MAX_POINT_LIGHTS,
              " (lights.lights_table), got ", lights.scalar_type(), " ", lights.sizes());
}

int64_t check_glass(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& glass, const at::Tensor& origins,
                    const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind) {
  check_scene_shape(scene, n_spheres);
  TORCH_CHECK(glass.scalar_type() == at::kDouble && glass.dim() == 2 && glass.size(0) == 2 &&
                  glass.size(1) == n_spheres,
              "glass must be ", at::kDouble, " [2, n_spheres] (glass.glass_table), got ", glass.scalar_type(), " ",
              glass.sizes());
  return check_rays_args(origins, dirs, max_bounces, RTX_GLASS_MAX_BOUNCES, "transmissive", out_kind);
}

int64_t check_lights(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& lights, const at::Tensor& origins,
                     const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind) {
  check_scene_shape(scene, n_spheres);
  check_lights_table(lights);
  return check_rays_args(origins, dirs, max_bounces, RTX_LIGHTS_MAX_BOUNCES, "multi-light", out_kind);
}

int64_t check_mesh(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh, const at::Tensor& lights,
                   const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind) {
  TORCH_CHECK(scene.dim() == 1, "scene must be the 1-D packed blob (scene_pack.pack_scene)");
  TORCH_CHECK(n_spheres >= 0 && n_spheres <= RTX_MAX_SPHERES, "n_spheres out of range: ", n_spheres);
  TORCH_CHECK(scene.numel() >= RTX_HDR_WORDS + n_spheres * (RTX_GEOM_WORDS + RTX_MAT_WORDS),
              "scene blob too short for ", n_spheres, " spheres");
  TORCH_CHECK(mesh.scalar_type() == at::kDouble && mesh.dim() == 1 && mesh.numel() >= RTX_MESH_HDR_WORDS &&
                  mesh.numel() <= INT32_MAX,
              "mesh must be ", at::kDouble, " [words] with at least ", (int)RTX_MESH_HDR_WORDS,
              " words (meshes.mesh_table), got ", mesh.scalar_type(), " ", mesh.sizes());
  check_lights_table(lights);
  return check_rays_args(origins, dirs, max_bounces, RTX_MESH_MAX_BOUNCES, "mesh", out_kind);
}

// The mesh table's header against its length: the host-side form of the kernel's own test, which reads a
// table that fails it as one without triangles (one synchronous copy of the header)
void check_mesh_header(const at::Tensor& mesh, bool uv = false) {
  const at::Tensor head = mesh.narrow(0, 0, RTX_MESH_HDR_WORDS).to(at::kCPU).contiguous();
  const double* h = head.data_ptr<double>();
  const double w = (double)mesh.numel(), T = h[RTX_MH_NTRI], M = h[RTX_MH_NMESH], N = h[RTX_MH_NNODES];
  const double ta = h[RTX_MH_TRIS], ma = h[RTX_MH_MATS], na = h[RTX_MH_NODES];
  TORCH_CHECK(h[RTX_MH_MAGIC] == RTX_MESH_MAGIC, "mesh is not a mesh table (bad magic; meshes.mesh_table)");
  TORCH_CHECK(h[RTX_MH_WORDS] == w && T >= 1 && T <= RTX_MAX_TRIANGLES && M >= 1 && M <= T && N >= 1 && N <= 2 * T &&
                  ta >= RTX_MESH_HDR_WORDS && ta + T * RTX_TRI_WORDS <= w && ma >= RTX_MESH_HDR_WORDS &&
                  ma + M * RTX_MAT_WORDS <= w && na >= RTX_MESH_HDR_WORDS && na + N * RTX_NODE_WORDS <= w,
              "mesh table: the header's counts and offsets do not fit its ", mesh.numel(), " words");
  if (uv) {  // rt::trace_mesh_uv: the UV part and the texel part
    const double ua = h[RTX_MH_UVS], xa = h[RTX_MH_TEXELS];
    TORCH_CHECK(ua >= RTX_MESH_HDR_WORDS && ua + T * RTX_UV_WORDS <= w && xa >= RTX_MESH_HDR_WORDS && xa <= w,
                "mesh table: the offsets of the UV part and the texel blocks do not fit its ", mesh.numel(),
                " words (a table of meshes.mesh_table with an ImageTexture on a mesh)");
  }
}

// ---- the environment map (rtx_env_sample, rtx_trace_lights_env, rtx_trace_glass_env) ----------------
// Shapes and ranges of an environment's arguments, shared by the kernels and their Meta forms: texels
// float32 [H, W, 4], gain three finite numbers, turn finite. Fills env but for its device pointer.
void check_env(const at::Tensor& texels, c10::ArrayRef<double> gain, double turn, rtx_env_t& env) {
  TORCH_CHECK(texels.scalar_type() == at::kFloat && texels.dim() == 3 && texels.size(2) == 4 && texels.size(0) >= 1 &&
                  texels.size(1) >= 1 && texels.size(0) * texels.size(1) <= RTX_ENV_MAX_TEXELS,
              "texels must be ", at::kFloat, " [H, W, 4] with 1 <= H * W <= ", (int)RTX_ENV_MAX_TEXELS, ", got ",
              texels.scalar_type(), " ", texels.sizes());
  TORCH_CHECK(gain.size() == 3 && std::isfinite(gain[0]) && std::isfinite(gain[1]) && std::isfinite(gain[2]),
              "gain must be three finite numbers (intensity * colour)");
  TORCH_CHECK(std::isfinite(turn), "turn must be finite (rotation / 360), got ", turn);
  env.texels = nullptr;
  env.height = (int)texels.size(0);
  env.width = (int)texels.size(1);
  for (int c = 0; c < 3; ++c) env.gain[c] = gain[c];
  env.turn = turn;
}

int64_t check_env_dirs(const at::Tensor& dirs) {
  TORCH_CHECK(dirs.scalar_type() == at::kDouble && dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be ", at::kDouble,
              " [3, n], got ", dirs.scalar_type(), " ", dirs.sizes());
  return dirs.size(1);
}

at::Tensor env_sample(const at::Tensor& texels, c10::ArrayRef<double> gain, double turn, const at::Tensor& dirs) {
  check_gpu(texels, "texels", at::kFloat);
  const at::OptionalDeviceGuard guard(at::device_of(texels));
  check_gpu(dirs, "dirs", at::kDouble);
  check_same_device(texels, dirs, "dirs");
  rtx_env_t env;
  check_env(texels, gain, turn, env);
  const int64_t n = check_env_dirs(dirs);
  at::Tensor out = at::empty({3, n}, dirs.options());
  if (n == 0) return out;  // (an empty tensor's pointer may be null)
  env.texels = texels.data_ptr<float>();
  check_rc(rtx_env_sample(&env, dirs.data_ptr<double>(), n, out.data_ptr<double>(), stream_of(texels)), "rtx_env_sample");
  return out;
}

// ---- the ops of the kernels with a stack of pending rays ------------------------------------------------
struct NamedTensor {
  const at::Tensor& t;
  const char* name;
};

struct EnvArg {  // an op's environment arguments, and the struct the op's body fills from them
  const at::Tensor& texels;
  c10::ArrayRef<double> gain;
  double turn;
  rtx_env_t env;
};

struct StackOp {  // what one of these ops is, beside its arguments
  const char* entry;                    // the library's entry, for the error message
  size_t (*ws_bytes)(int64_t, int);     // its workspace size function
  int64_t depth;                        // the pending rays a lane's stack holds, for the overflow message
  const at::Tensor* mesh = nullptr;     // the mesh table whose header is checked with the blob's, if any
  bool uv = false;                      // ... with its UV part
};

// The body of rt::trace_glass, trace_lights, trace_mesh, trace_mesh_uv, trace_lights_env and trace_glass_env: the
// device guard and the device checks of the float64 inputs `in` (and the environment's texels), `shape()` (the
// op's check_*: returns n), the output, the headers, the op's own zeroed workspace, `call(n, out, ws)` (the
// library's entry) and the status.
template <class Shape, class Call>
at::Tensor trace_stack_rays(const StackOp& op, const at::Tensor& scene, int64_t n_spheres,
                            std::initializer_list<NamedTensor> in, Shape&& shape, Call&& call, int64_t max_bounces,
                            int64_t out_kind, bool check, EnvArg* e = nullptr) {
  check_gpu(scene, "scene", at::kDouble);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  for (const auto& a : in) {
    check_gpu(a.t, a.name, at::kDouble);
    check_same_device(scene, a.t, a.name);
  }
  if (e) {
    check_gpu(e->texels, "texels", at::kFloat);
    check_same_device(scene, e->texels, "texels");
  }
  const int64_t n = shape();
  if (e) check_env(e->texels, e->gain, e->turn, e->env);
  at::Tensor out = new_output(scene, n, -1, 0, out_kind);
  if (check) {
    check_headers(scene, n_spheres);
    if (op.mesh) check_mesh_header(*op.mesh, op.uv);
  }
  if (n == 0) return out;  // (an empty tensor's pointer may be null)
  if (e) e->env.texels = e->texels.data_ptr<float>();
  // the op's own workspace: the zeroed header and the workers' stacks of pending rays
  at::Tensor ws = at::zeros({(int64_t)op.ws_bytes(n, (int)max_bounces)}, scene.options().dtype(at::kByte));
  check_rc(call(n, out, ws), op.entry);
  if (check) {  // (a synchronisation; check=False leaves an overflowed lane's dropped rays unreported)
    const int32_t st = ws.narrow(0, 4 * RTX_WS_STATUS, 4).view(at::kInt).item<int32_t>();
    TORCH_CHECK(!(st & RTX_ST_STACK_OVERFLOW), "maximum recursion depth exceeded (a ray tree with ties needed more than ",
                op.depth, " pending rays; HipRenderer raises RecursionError)");
  }
  return out;
}

// rt::trace_glass (e null) and rt::trace_glass_env
at::Tensor trace_glass_under(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& glass,
                             const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                             bool check, EnvArg* e) {
  const StackOp op{e ? "rtx_trace_glass_env" : "rtx_trace_glass", rtx_glass_workspace_bytes, 4 * max_bounces + 4};
  return trace_stack_rays(
      op, scene, n_spheres, {{glass, "glass"}, {origins, "origins"}, {dirs, "dirs"}},
      [&] { return check_glass(scene, n_spheres, glass, origins, dirs, max_bounces, out_kind); },
      [&](int64_t n, at::Tensor& out, at::Tensor& ws) {
        const double *S = scene.data_ptr<double>(), *G = glass.data_ptr<double>(), *O = origins.data_ptr<double>(),
                     *D = dirs.data_ptr<double>();
        const int64_t stride = origins.dim() == 1 ? 0 : n;
        if (e)
          return rtx_trace_glass_env(S, (int)n_spheres, G, O, stride, D, n, (int)max_bounces, out.data_ptr(),
                                     (int)out_kind, ws.data_ptr(), (size_t)ws.numel(), stream_of(scene), &e->env);
        return rtx_trace_glass(S, (int)n_spheres, G, O, stride, D, n, (int)max_bounces, out.data_ptr(), (int)out_kind,
                               ws.data_ptr(), (size_t)ws.numel(), stream_of(scene));
      },
      max_bounces, out_kind, check, e);
}

// rt::trace_lights (e null) and rt::trace_lights_env
at::Tensor trace_lights_under(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& lights,
                              const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                              bool check, EnvArg* e) {
  const StackOp op{e ? "rtx_trace_lights_env" : "rtx_trace_lights", rtx_lights_workspace_bytes, 2 * max_bounces + 2};
  return trace_stack_rays(
      op, scene, n_spheres, {{lights, "lights"}, {origins, "origins"}, {dirs, "dirs"}},
      [&] { return check_lights(scene, n_spheres, lights, origins, dirs, max_bounces, out_kind); },
      [&](int64_t n, at::Tensor& out, at::Tensor& ws) {
        const double *S = scene.data_ptr<double>(), *T = lights.data_ptr<double>(), *O = origins.data_ptr<double>(),
                     *D = dirs.data_ptr<double>();
        const int64_t stride = origins.dim() == 1 ? 0 : n;
        const int L = (int)lights.size(0);
        if (e)
          return rtx_trace_lights_env(S, (int)n_spheres, T, L, O, stride, D, n, (int)max_bounces, out.data_ptr(),
                                      (int)out_kind, ws.data_ptr(), (size_t)ws.numel(), stream_of(scene), &e->env);
        return rtx_trace_lights(S, (int)n_spheres, T, L, O, stride, D, n, (int)max_bounces, out.data_ptr(),
                                (int)out_kind, ws.data_ptr(), (size_t)ws.numel(), stream_of(scene));
      },
      max_bounces, out_kind, check, e);
}

// rt::trace_mesh (uv false) and rt::trace_mesh_uv
at::Tensor trace_mesh_call(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh, const at::Tensor& lights,
                           const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                           bool check, bool uv) {
  const StackOp op{uv ? "rtx_trace_mesh_uv" : "rtx_trace_mesh", rtx_mesh_workspace_bytes, 2 * max_bounces + 2, &mesh, uv};
  return trace_stack_rays(
      op, scene, n_spheres, {{mesh, "mesh"}, {lights, "lights"}, {origins, "origins"}, {dirs, "dirs"}},
      [&] { return check_mesh(scene, n_spheres, mesh, lights, origins, dirs, max_bounces, out_kind); },
      [&](int64_t n, at::Tensor& out, at::Tensor& ws) {
        return (uv ? rtx_trace_mesh_uv : rtx_trace_mesh)(
            scene.data_ptr<double>(), (int)n_spheres, mesh.data_ptr<double>(), mesh.numel(), lights.data_ptr<double>(),
            (int)lights.size(0), origins.data_ptr<double>(), origins.dim() == 1 ? 0 : n, dirs.data_ptr<double>(), n,
            (int)max_bounces, out.data_ptr(), (int)out_kind, ws.data_ptr(), (size_t)ws.numel(), stream_of(scene));
      },
      max_bounces, out_kind, check);
}

at::Tensor trace_glass(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& glass, const at::Tensor& origins,
                       const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind, bool check) {
  return trace_glass_under(scene, n_spheres, glass, origins, dirs, max_bounces, out_kind, check, nullptr);
}

at::Tensor trace_lights(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& lights, const at::Tensor& origins,
                        const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind, bool check) {
  return trace_lights_under(scene, n_spheres, lights, origins, dirs, max_bounces, out_kind, check, nullptr);
}

at::Tensor trace_mesh(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh, const at::Tensor& lights,
                      const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                      bool check) {
  return trace_mesh_call(scene, n_spheres, mesh, lights, origins, dirs, max_bounces, out_kind, check, false);
}

at::Tensor trace_mesh_uv(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh, const at::Tensor& lights,
                         const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                         bool check) {
  return trace_mesh_call(scene, n_spheres, mesh, lights, origins, dirs, max_bounces, out_kind, check, true);
}

// ---- primary-hit render passes of a mesh scene (rtx_mesh_aovs) ------------------------------------------
// `passes`: a mask of RTX_MESH_AOV_* bits; the result holds one tensor per set bit, in bit order: depth float64
// [n], id / hits int32 [n], position / normal / geometric_normal / albedo float64 [3, n], lit uint8 [n], triangle
// int32 [n], bary float64 [2, n]. Shared by the kernel and its Meta form.
std::vector<at::Tensor> new_mesh_aovs(const at::Tensor& like, int64_t n, int64_t passes) {
  TORCH_CHECK(passes > 0 && (passes & ~(int64_t)RTX_MESH_AOV_ALL) == 0,
              "passes must be a non-empty mask of RTX_MESH_AOV_* bits (1..", (int)RTX_MESH_AOV_ALL, "), got ", passes);
  const auto o = like.options();
  std::vector<at::Tensor> out;
  if (passes & RTX_MESH_AOV_DEPTH) out.push_back(at::empty({n}, o.dtype(at::kDouble)));
  if (passes & RTX_MESH_AOV_ID) out.push_back(at::empty({n}, o.dtype(at::kInt)));
  if (passes & RTX_MESH_AOV_HITS) out.push_back(at::empty({n}, o.dtype(at::kInt)));
  if (passes & RTX_MESH_AOV_POSITION) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_MESH_AOV_NORMAL) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_MESH_AOV_GEOMETRIC_NORMAL) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_MESH_AOV_ALBEDO) out.push_back(at::empty({3, n}, o.dtype(at::kDouble)));
  if (passes & RTX_MESH_AOV_LIT) out.push_back(at::empty({n}, o.dtype(at::kByte)));
  if (passes & RTX_MESH_AOV_TRIANGLE) out.push_back(at::empty({n}, o.dtype(at::kInt)));
  if (passes & RTX_MESH_AOV_BARY) out.push_back(at::empty({2, n}, o.dtype(at::kDouble)));
  return out;
}

// Shapes and ranges of rt::mesh_aovs' arguments (check_mesh's, without a bounce cap or an out_kind): returns n.
// shape_ids, if given: int32 [n_spheres + meshes], at least one mesh.
int64_t check_mesh_aovs(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh, const at::Tensor& lights,
                        const std::optional<at::Tensor>& shape_ids, const at::Tensor& origins,
                        const at::Tensor& dirs) {
  const int64_t n = check_mesh(scene, n_spheres, mesh, lights, origins, dirs, 0, RTX_OUT_F64_SOA);
  if (shape_ids.has_value())
    TORCH_CHECK(shape_ids->scalar_type() == at::kInt && shape_ids->dim() == 1 && shape_ids->numel() >= n_spheres + 1,
                "shape_ids must be ", at::kInt, " [n_spheres + meshes] (one entry per sphere, then one per mesh of "
                "the table), got ", shape_ids->scalar_type(), " ", shape_ids->sizes());
  return n;
}

std::vector<at::Tensor> mesh_aovs(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh,
                                  const at::Tensor& lights, const std::optional<at::Tensor>& shape_ids,
                                  const at::Tensor& origins, const at::Tensor& dirs, int64_t passes, bool check) {
  check_gpu(scene, "scene", at::kDouble);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  for (const NamedTensor& a : {NamedTensor{mesh, "mesh"}, NamedTensor{lights, "lights"},
                               NamedTensor{origins, "origins"}, NamedTensor{dirs, "dirs"}}) {
    check_gpu(a.t, a.name, at::kDouble);
    check_same_device(scene, a.t, a.name);
  }
  if (shape_ids.has_value()) {
    check_gpu(*shape_ids, "shape_ids", at::kInt);
    check_same_device(scene, *shape_ids, "shape_ids");
  }
  const int64_t n = check_mesh_aovs(scene, n_spheres, mesh, lights, shape_ids, origins, dirs);
  std::vector<at::Tensor> out = new_mesh_aovs(scene, n, passes);
  if (check) {
    check_headers(scene, n_spheres);
    check_mesh_header(mesh);
    if (shape_ids.has_value()) {  // (one more synchronous copy of the header's mesh count)
      const double meshes = mesh.narrow(0, RTX_MH_NMESH, 1).item<double>();
      TORCH_CHECK((double)shape_ids->numel() == (double)n_spheres + meshes, "shape_ids must have one entry per sphere "
                  "and per mesh of the table (", n_spheres, " + ", meshes, "), got ", shape_ids->sizes());
    }
  }
  if (n == 0) return out;  // (an empty tensor's pointer may be null)
  void* p[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t k = 0;
  for (int b = 0; b < 10; ++b)
    if (passes & (int64_t(1) << b)) p[b] = out[k++].data_ptr();
  check_rc(rtx_mesh_aovs(scene.data_ptr<double>(), (int)n_spheres, mesh.data_ptr<double>(), mesh.numel(),
                         lights.data_ptr<double>(), (int)lights.size(0),
                         shape_ids.has_value() ? shape_ids->data_ptr<int32_t>() : nullptr, origins.data_ptr<double>(),
                         origins.dim() == 1 ? 0 : n, dirs.data_ptr<double>(), n, (double*)p[0], (int32_t*)p[1],
                         (int32_t*)p[2], (double*)p[3], (double*)p[4], (double*)p[5], (double*)p[6], (uint8_t*)p[7],
                         (int32_t*)p[8], (double*)p[9], stream_of(scene)),
           "rtx_mesh_aovs");
  return out;
}

at::Tensor trace_lights_env(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& lights,
                            const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                            const at::Tensor& texels, c10::ArrayRef<double> gain, double turn, bool check) {
  EnvArg e{texels, gain, turn, {}};
  return trace_lights_under(scene, n_spheres, lights, origins, dirs, max_bounces, out_kind, check, &e);
}

at::Tensor trace_glass_env(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& glass,
                           const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                           const at::Tensor& texels, c10::ArrayRef<double> gain, double turn, bool check) {
  EnvArg e{texels, gain, turn, {}};
  return trace_glass_under(scene, n_spheres, glass, origins, dirs, max_bounces, out_kind, check, &e);
}

int64_t status(at::Tensor& workspace) {
  check_gpu(workspace, "workspace", at::kByte);
  TORCH_CHECK(workspace.numel() >= RTX_WS_HDR_BYTES, "workspace shorter than its header");
  const at::OptionalDeviceGuard guard(at::device_of(workspace));
  at::Tensor word = workspace.narrow(0, 4 * RTX_WS_STATUS, 4);
  const int32_t st = word.view(at::kInt).item<int32_t>();
  if (st) word.zero_();
  return st;
}

int64_t workspace_bytes(int64_t n_rays, int64_t max_bounces) {
  return (int64_t)rtx_workspace_bytes(n_rays, (int)max_bounces);
}

// ---- the row-tiled multi-GPU frame (rtx_tiles_*, rtx_comm_*; csrc/rtx_tiles.hip) ---------------
// Handles are plain int64: a communicator from comm_init, a plan from tiles_create. The caller keeps
// the plan's buffers (send / recv, the workspace, the frame) alive until tiles_destroy, as the C ABI
// asks. These are what distributed.TileGather drives through ctypes; an integrator binding only the
// ops gets the same overlapped native gather.

void* as_ptr(int64_t h) { return reinterpret_cast<void*>(static_cast<intptr_t>(h)); }
int64_t as_handle(void* p) { return static_cast<int64_t>(reinterpret_cast<intptr_t>(p)); }

struct DeviceScope {  // the current device set to `device` (>= 0) for the scope
  int prev = -1;
  explicit DeviceScope(int64_t device) {
    if (device >= 0) {
      TORCH_CHECK(hipGetDevice(&prev) == hipSuccess, "hipGetDevice failed");
      TORCH_CHECK(hipSetDevice((int)device) == hipSuccess, "hipSetDevice(", device, ") failed");
    }
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

at::Tensor comm_unique_id() {
  check_rc(rtx_rccl_load(nullptr), "rtx_rccl_load");
  at::Tensor id = at::empty({128}, at::TensorOptions().dtype(at::kByte));
  check_rc(rtx_comm_unique_id(id.data_ptr()), "rtx_comm_unique_id");
  return id;
}

int64_t comm_init(const at::Tensor& unique_id, int64_t world, int64_t rank, int64_t device, int64_t max_ctas) {
  TORCH_CHECK(!unique_id.is_cuda() && unique_id.scalar_type() == at::kByte && unique_id.numel() == 128 &&
                  unique_id.is_contiguous(),
              "unique_id must be the 128-byte host uint8 tensor comm_unique_id returned (broadcast to every rank)");
  check_rc(rtx_rccl_load(nullptr), "rtx_rccl_load");
  DeviceScope scope(device);
  void* comm = nullptr;
  check_rc(rtx_comm_init(unique_id.data_ptr(), (int)world, (int)rank, (int)max_ctas, &comm), "rtx_comm_init");
  return as_handle(comm);
}

void comm_destroy(int64_t comm) { check_rc(rtx_comm_destroy(as_ptr(comm)), "rtx_comm_destroy"); }

int64_t tiles_create(int64_t comm, int64_t world, int64_t rank, int64_t root, int64_t width, int64_t height,
                     int64_t row_block, int64_t out_kind, int64_t slots, at::TensorList send, at::TensorList recv,
                     int64_t part_bytes, int64_t root_run, int64_t run, int64_t flags, int64_t device) {
  TORCH_CHECK(slots >= 1 && slots <= RTX_TILES_MAX_SLOTS, "slots must be in 1..", RTX_TILES_MAX_SLOTS);
  TORCH_CHECK(send.empty() || (int64_t)send.size() == slots, "send: one buffer per slot, or none");
  TORCH_CHECK(recv.empty() || (int64_t)recv.size() == slots, "recv: one buffer per slot, or none");
  std::vector<void*> sp, rp;
  for (const at::Tensor& t : send) {
    check_gpu(t, "send buffer", at::kByte);
    TORCH_CHECK(t.numel() >= part_bytes, "a send buffer must hold part_bytes");
    sp.push_back(t.data_ptr());
  }
  for (const at::Tensor& t : recv) {
    check_gpu(t, "recv buffer", at::kByte);
    TORCH_CHECK(t.numel() >= world * part_bytes, "a recv buffer must hold world * part_bytes");
    rp.push_back(t.data_ptr());
  }
  DeviceScope scope(device);
  void* plan = nullptr;
  check_rc(rtx_tiles_create(as_ptr(comm), (int)world, (int)rank, (int)root, (int)width, (int)height, (int)row_block,
                            (int)out_kind, (int)slots, sp.empty() ? nullptr : sp.data(),
                            rp.empty() ? nullptr : rp.data(), part_bytes, (int)root_run, (int)run,
                            (unsigned)flags, &plan),
           "rtx_tiles_create");
  return as_handle(plan);
}

void tiles_submit(int64_t plan, int64_t slot, const at::Tensor& scene, int64_t n_spheres, int64_t max_bounces,
                  at::Tensor& workspace, const std::optional<at::Tensor>& frame, int64_t flags) {
  check_scene(scene, n_spheres);
  const at::OptionalDeviceGuard guard(at::device_of(scene));
  check_bounces(max_bounces);
  check_gpu(workspace, "workspace", at::kByte);
  check_same_device(scene, workspace, "workspace");
  if (frame) {
    TORCH_CHECK(frame->is_cuda() && frame->is_contiguous(), "frame must be a contiguous GPU tensor");
    check_same_device(scene, *frame, "frame");
  }
  check_rc(rtx_tiles_submit(as_ptr(plan), (int)slot, scene.data_ptr<double>(), (int)n_spheres, (int)max_bounces,
                            workspace.data_ptr(), (size_t)workspace.numel(), (unsigned)flags, nullptr, nullptr,
                            nullptr, frame ? frame->data_ptr() : nullptr, stream_of(scene)),
           "rtx_tiles_submit");
}

void tiles_finish(int64_t plan, int64_t slot, int64_t device) {
  TORCH_CHECK(device >= 0, "tiles_finish needs the plan's device index");
  check_rc(rtx_tiles_finish(as_ptr(plan), (int)slot, c10::hip::getCurrentHIPStream((int)device).stream()),
           "rtx_tiles_finish");
}

void tiles_destroy(int64_t plan) { check_rc(rtx_tiles_destroy(as_ptr(plan)), "rtx_tiles_destroy"); }

// ---- fake (Meta) kernels: output shapes only, for tracing (torch.compile / FakeTensor) ----------

at::Tensor render_tile_meta(const at::Tensor& scene, int64_t n_spheres, int64_t width, int64_t height,
                            int64_t row_block, int64_t n_parts, int64_t part, int64_t, int64_t out_kind, at::Tensor&,
                            const std::optional<at::Tensor>&, bool, int64_t part_run) {
  check_scene_shape(scene, n_spheres);
  check_tile(width, height, row_block, n_parts, part, part_run);
  const int64_t rows = tile_rows(height, row_block, n_parts, part, part_run);
  return new_output(scene, width * rows, rows, width, out_kind);
}

at::Tensor render_frames_meta(const at::Tensor& scenes, int64_t, int64_t width, int64_t height, int64_t,
                              int64_t out_kind, at::Tensor&, const std::optional<at::Tensor>&, bool) {
  TORCH_CHECK(scenes.dim() == 2, "scenes must be [F, L]");
  return new_output(scenes, width * height, height, width, out_kind, scenes.size(0));
}

at::Tensor trace_meta(const at::Tensor& scene, int64_t, const at::Tensor&, const at::Tensor& dirs, int64_t,
                      int64_t out_kind, at::Tensor&, const std::optional<at::Tensor>&, bool) {
  TORCH_CHECK(dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be [3, n]");
  return new_output(scene, dirs.size(1), -1, 0, out_kind);
}

at::Tensor shade_hits_meta(const at::Tensor& scene, int64_t, int64_t, const at::Tensor&, const at::Tensor& dirs,
                           const at::Tensor&, int64_t, int64_t out_kind, at::Tensor&,
                           const std::optional<at::Tensor>&, bool) {
  TORCH_CHECK(dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be [3, n]");
  return new_output(scene, dirs.size(1), -1, 0, out_kind);
}

at::Tensor intersect_meta(const at::Tensor&, const at::Tensor&, const at::Tensor& dirs) {
  TORCH_CHECK(dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be [3, n]");
  return at::empty({dirs.size(1)}, dirs.options());
}

at::Tensor quantize_u8_meta(const at::Tensor& color) {
  TORCH_CHECK(color.dim() == 2 && color.size(0) == 3, "color must be [3, n]");
  return at::empty({color.size(1), 3}, color.options().dtype(at::kByte));
}

at::Tensor assemble_rows_meta(const at::Tensor& tiles, int64_t width, int64_t height, int64_t, int64_t out_kind,
                              int64_t root_run, int64_t run) {
  TORCH_CHECK(root_run >= 1 && run >= 1, "root_run and run must be >= 1");
  return assemble_out(tiles, width, height, out_kind);
}

at::Tensor resolve_samples_meta(const at::Tensor& samples, int64_t k, int64_t width, int64_t rows, int64_t out_kind) {
  const int64_t frames = check_samples_shape(samples, k, width, rows, out_kind);
  return new_output(samples, rows * width, rows, width, out_kind, frames);
}

std::vector<at::Tensor> primary_aovs_meta(const at::Tensor& scene, int64_t n_spheres, int64_t width, int64_t height,
                                          int64_t row_block, int64_t n_parts, int64_t part, int64_t part_run,
                                          int64_t passes, bool) {
  check_scene_shape(scene, n_spheres);
  check_tile(width, height, row_block, n_parts, part, part_run);
  return new_aovs(scene, width * tile_rows(height, row_block, n_parts, part, part_run), passes);
}

std::vector<at::Tensor> primary_aovs_rays_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor&,
                                               const at::Tensor& dirs, int64_t passes, bool) {
  check_scene_shape(scene, n_spheres);
  TORCH_CHECK(dirs.dim() == 2 && dirs.size(0) == 3, "dirs must be [3, n]");
  return new_aovs(scene, dirs.size(1), passes);
}

std::vector<at::Tensor> occlusion_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& id,
                                       const at::Tensor& position, const at::Tensor& normal, const at::Tensor& table,
                                       const at::Tensor& rot, double max_distance, double light_radius,
                                       int64_t passes, bool) {
  return new_occlusion(scene, check_occlusion(scene, n_spheres, id, position, normal, table, rot, max_distance,
                                              light_radius, passes), passes);
}

at::Tensor trace_glass_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& glass,
                            const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                            bool) {
  return new_output(scene, check_glass(scene, n_spheres, glass, origins, dirs, max_bounces, out_kind), -1, 0, out_kind);
}

at::Tensor trace_lights_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& lights,
                             const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                             bool) {
  return new_output(scene, check_lights(scene, n_spheres, lights, origins, dirs, max_bounces, out_kind), -1, 0, out_kind);
}

at::Tensor trace_mesh_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh, const at::Tensor& lights,
                           const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces, int64_t out_kind,
                           bool) {
  return new_output(scene, check_mesh(scene, n_spheres, mesh, lights, origins, dirs, max_bounces, out_kind), -1, 0,
                    out_kind);
}

std::vector<at::Tensor> mesh_aovs_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& mesh,
                                       const at::Tensor& lights, const std::optional<at::Tensor>& shape_ids,
                                       const at::Tensor& origins, const at::Tensor& dirs, int64_t passes, bool) {
  return new_mesh_aovs(scene, check_mesh_aovs(scene, n_spheres, mesh, lights, shape_ids, origins, dirs), passes);
}

at::Tensor env_sample_meta(const at::Tensor& texels, c10::ArrayRef<double> gain, double turn, const at::Tensor& dirs) {
  rtx_env_t env;
  check_env(texels, gain, turn, env);
  return at::empty({3, check_env_dirs(dirs)}, dirs.options());
}

at::Tensor trace_lights_env_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& lights,
                                 const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces,
                                 int64_t out_kind, const at::Tensor& texels, c10::ArrayRef<double> gain, double turn,
                                 bool check) {
  rtx_env_t env;
  check_env(texels, gain, turn, env);
  return trace_lights_meta(scene, n_spheres, lights, origins, dirs, max_bounces, out_kind, check);
}

at::Tensor trace_glass_env_meta(const at::Tensor& scene, int64_t n_spheres, const at::Tensor& glass,
                                const at::Tensor& origins, const at::Tensor& dirs, int64_t max_bounces,
                                int64_t out_kind, const at::Tensor& texels, c10::ArrayRef<double> gain, double turn,
                                bool check) {
  rtx_env_t env;
  check_env(texels, gain, turn, env);
  return trace_glass_meta(scene, n_spheres, glass, origins, dirs, max_bounces, out_kind, check);
}

at::Tensor edge_mask_meta(const at::Tensor& color, const at::Tensor& id, const at::Tensor& hits,
                          const at::Tensor& lit, int64_t width, int64_t height, double contrast) {
  check_edge_inputs(color, id, hits, lit, width, height, contrast);
  return at::empty({width * height}, color.options().dtype(at::kByte));
}

at::Tensor sample_dirs_meta(const at::Tensor& sample_scene, int64_t k, int64_t width, int64_t height,
                            const at::Tensor& pixels) {
  TORCH_CHECK(sample_scene.dim() == 1 && sample_scene.numel() >= RTX_HDR_WORDS,
              "sample_scene must be a 1-D packed scene (at least its header)");
  return at::empty({3, check_pixels(pixels, k, width, height) * k * k}, sample_scene.options().dtype(at::kDouble));
}

void resolve_scatter_meta(const at::Tensor& samples, int64_t k, const at::Tensor& pixels, int64_t width,
                          int64_t height, at::Tensor& out, int64_t out_kind) {
  check_scatter(samples, k, pixels, width, height, out, out_kind);
}

// (on the device of the lens table; without one, of cam: no argument names the GPU the rays land on)
std::tuple<std::optional<at::Tensor>, at::Tensor> camera_rays_meta(const at::Tensor& cam,
                                                                  const std::optional<at::Tensor>& lens, int64_t k,
                                                                  int64_t width, int64_t height, int64_t row_block,
                                                                  int64_t n_parts, int64_t part, int64_t part_run) {
  const int64_t n = check_camera_rays(cam, lens, k, width, height, row_block, n_parts, part, part_run);
  const auto opts = (lens.has_value() ? lens->options() : cam.options()).dtype(at::kDouble);
  std::optional<at::Tensor> origins;
  if (lens.has_value()) origins = at::empty({3, n}, opts);
  return {origins, at::empty({3, n}, opts)};
}

// ---- rt::mesh_build: the mesh table made on the device (rtx_mesh_build) -------------------------------------
// Shapes and ranges of its arguments, shared by the kernel and its Meta form: returns T.
int64_t check_mesh_build(const at::Tensor& vertices, const at::Tensor& faces, const at::Tensor& tri_mesh,
                         const std::optional<at::Tensor>& normals, const std::optional<at::Tensor>& mesh_smooth,
                         const std::optional<at::Tensor>& uvs, const at::Tensor& skeleton, int64_t max_leaf,
                         const at::Tensor& workspace) {
  TORCH_CHECK(vertices.scalar_type() == at::kDouble && vertices.dim() == 2 && vertices.size(1) == 3 &&
                  vertices.size(0) >= 1 && vertices.size(0) <= INT32_MAX,
              "vertices must be ", at::kDouble, " [V, 3] with V >= 1, got ", vertices.scalar_type(), " ", vertices.sizes());
  TORCH_CHECK(faces.scalar_type() == at::kInt && faces.dim() == 2 && faces.size(1) == 3 && faces.size(0) >= 1 &&
                  faces.size(0) <= RTX_MAX_TRIANGLES,
              "faces must be ", at::kInt, " [T, 3] with T in 1..", (int)RTX_MAX_TRIANGLES, ", got ", faces.scalar_type(),
              " ", faces.sizes());
  const int64_t T = faces.size(0);
  TORCH_CHECK(tri_mesh.scalar_type() == at::kInt && tri_mesh.dim() == 1 && tri_mesh.size(0) == T, "tri_mesh must be ",
              at::kInt, " [T] with T = ", T, ", got ", tri_mesh.scalar_type(), " ", tri_mesh.sizes());
  TORCH_CHECK(normals.has_value() == mesh_smooth.has_value(), "normals and mesh_smooth are given together or not at all");
  if (normals.has_value()) {
    TORCH_CHECK(normals->scalar_type() == at::kDouble && normals->sizes() == vertices.sizes(), "normals must be ",
                at::kDouble, " [V, 3] like the vertices, got ", normals->scalar_type(), " ", normals->sizes());
    TORCH_CHECK(mesh_smooth->scalar_type() == at::kInt && mesh_smooth->dim() == 1 && mesh_smooth->size(0) >= 1,
                "mesh_smooth must be ", at::kInt, " [M], got ", mesh_smooth->scalar_type(), " ", mesh_smooth->sizes());
  }
  if (uvs.has_value())
    TORCH_CHECK(uvs->scalar_type() == at::kDouble && uvs->dim() == 2 && uvs->size(0) == T && uvs->size(1) == RTX_UV_WORDS,
                "uvs must be ", at::kDouble, " [T, ", (int)RTX_UV_WORDS, "], got ", uvs->scalar_type(), " ", uvs->sizes());
  TORCH_CHECK(skeleton.scalar_type() == at::kDouble && skeleton.dim() == 1 && skeleton.numel() >= RTX_MESH_HDR_WORDS &&
                  skeleton.numel() <= INT32_MAX,
              "skeleton must be ", at::kDouble, " [words] with at least ", (int)RTX_MESH_HDR_WORDS,
              " words (meshes.device_inputs), got ", skeleton.scalar_type(), " ", skeleton.sizes());
  TORCH_CHECK(max_leaf >= 0 && max_leaf <= INT32_MAX, "max_leaf must be positive, or 0 for one leaf, got ", max_leaf);
  TORCH_CHECK(workspace.scalar_type() == at::kByte && workspace.dim() == 1, "workspace must be ", at::kByte,
              " [bytes], got ", workspace.scalar_type(), " ", workspace.sizes());
  return T;
}

// Fills `skeleton` in place; returns the build's two status words, int32 [2] (a copy: the workspace is the caller's
// to reuse). check: the skeleton's header against its length and the workspace's size are refused here, and a
// degenerate triangle raises (a synchronisation); without it the library's own codes and the status speak.
at::Tensor mesh_build(const at::Tensor& vertices, const at::Tensor& faces, const at::Tensor& tri_mesh,
                      const std::optional<at::Tensor>& normals, const std::optional<at::Tensor>& mesh_smooth,
                      const std::optional<at::Tensor>& uvs, at::Tensor& skeleton, int64_t max_leaf, at::Tensor& workspace,
                      bool check) {
  check_gpu(skeleton, "skeleton", at::kDouble);
  const at::OptionalDeviceGuard guard(at::device_of(skeleton));
  const auto on = [&](const at::Tensor& t, const char* name, at::ScalarType dtype) {
    check_gpu(t, name, dtype);
    check_same_device(skeleton, t, name);
  };
  on(vertices, "vertices", at::kDouble), on(faces, "faces", at::kInt), on(tri_mesh, "tri_mesh", at::kInt);
  on(workspace, "workspace", at::kByte);
  if (normals.has_value()) on(*normals, "normals", at::kDouble);
  if (mesh_smooth.has_value()) on(*mesh_smooth, "mesh_smooth", at::kInt);
  if (uvs.has_value()) on(*uvs, "uvs", at::kDouble);
  const int64_t T = check_mesh_build(vertices, faces, tri_mesh, normals, mesh_smooth, uvs, skeleton, max_leaf, workspace);
  // (one synchronous copy of the header: the entry reads it on the host)
  const at::Tensor head = skeleton.narrow(0, 0, RTX_MESH_HDR_WORDS).to(at::kCPU).contiguous();
  const double* h = head.data_ptr<double>();
  if (check) {
    TORCH_CHECK(h[RTX_MH_MAGIC] == RTX_MESH_MAGIC && h[RTX_MH_NTRI] == (double)T,
                "skeleton is not a mesh table of ", T, " triangles (meshes.device_inputs)");
    TORCH_CHECK(h[RTX_MH_WORDS] <= (double)skeleton.numel(), "skeleton has ", skeleton.numel(),
                " words, fewer than its header says (", h[RTX_MH_WORDS], ")");
    const size_t need = rtx_mesh_build_workspace_bytes(T, rtx_mesh_build_nodes(T, (int)max_leaf));
    TORCH_CHECK((size_t)workspace.numel() >= need, "workspace too small: ", workspace.numel(), " < ", need,
                " bytes (rtx_mesh_build_workspace_bytes)");
    if (mesh_smooth.has_value())
      TORCH_CHECK((double)mesh_smooth->size(0) == h[RTX_MH_NMESH], "mesh_smooth must have one flag per mesh (",
                  h[RTX_MH_NMESH], "), got ", mesh_smooth->sizes());
  }
  check_rc(rtx_mesh_build(vertices.data_ptr<double>(), vertices.size(0), faces.data_ptr<int32_t>(),
                          tri_mesh.data_ptr<int32_t>(), T, normals.has_value() ? normals->data_ptr<double>() : nullptr,
                          mesh_smooth.has_value() ? mesh_smooth->data_ptr<int32_t>() : nullptr,
                          uvs.has_value() ? uvs->data_ptr<double>() : nullptr, h, skeleton.data_ptr<double>(),
                          skeleton.numel(), (int)max_leaf, workspace.data_ptr(), (size_t)workspace.numel(),
                          stream_of(skeleton)),
           "rtx_mesh_build");
  at::Tensor status = workspace.narrow(0, 0, 8).view(at::kInt).clone();
  if (check) {
    const at::Tensor st = status.to(at::kCPU);
    const int32_t* w = st.data_ptr<int32_t>();
    TORCH_CHECK(w[1] == 0, "rtx_mesh_build: a face index or a mesh number is out of range");
    TORCH_CHECK((uint32_t)w[0] == RTX_MB_NONE, "rtx_mesh_build: triangle ", (uint32_t)w[0],
                " is degenerate (its normal cannot be normalised)");
  }
  return status;
}

at::Tensor mesh_build_meta(const at::Tensor& vertices, const at::Tensor& faces, const at::Tensor& tri_mesh,
                           const std::optional<at::Tensor>& normals, const std::optional<at::Tensor>& mesh_smooth,
                           const std::optional<at::Tensor>& uvs, at::Tensor& skeleton, int64_t max_leaf,
                           at::Tensor& workspace, bool) {
  check_mesh_build(vertices, faces, tri_mesh, normals, mesh_smooth, uvs, skeleton, max_leaf, workspace);
  return at::empty({2}, skeleton.options().dtype(at::kInt));
}

}  // namespace

TORCH_LIBRARY(rt, m) {
  m.def("camera_rays(Tensor cam, Tensor? lens, int k, int width, int height, int row_block=1, int n_parts=1, "
        "int part=0, int part_run=1) -> (Tensor?, Tensor)");
  m.def("render_tile(Tensor scene, int n_spheres, int width, int height, int row_block, int n_parts, int part, "
        "int max_bounces, int out_kind, Tensor(a!) workspace, Tensor(b!)? stats=None, bool check=True, "
        "int part_run=1) -> Tensor");
  m.def("render_frames(Tensor scenes, int n_spheres, int width, int height, int max_bounces, int out_kind, "
        "Tensor(a!) workspace, Tensor(b!)? stats=None, bool check=True) -> Tensor");
  m.def("trace(Tensor scene, int n_spheres, Tensor origins, Tensor dirs, int max_bounces, int out_kind, "
        "Tensor(a!) workspace, Tensor(b!)? stats=None, bool check=True) -> Tensor");
  m.def("shade_hits(Tensor scene, int n_spheres, int shape, Tensor origins, Tensor dirs, Tensor t, int max_bounces, "
        "int out_kind, Tensor(a!) workspace, Tensor(b!)? stats=None, bool check=True) -> Tensor");
  m.def("intersect(Tensor sphere, Tensor origins, Tensor dirs) -> Tensor");
  m.def("quantize_u8(Tensor color) -> Tensor");
  m.def("assemble_rows(Tensor tiles, int width, int height, int row_block, int out_kind, int root_run=1, "
        "int run=1) -> Tensor");
  m.def("resolve_samples(Tensor samples, int k, int width, int rows, int out_kind) -> Tensor");
  m.def("primary_aovs(Tensor scene, int n_spheres, int width, int height, int row_block, int n_parts, int part, "
        "int part_run, int passes, bool check=True) -> Tensor[]");
  m.def("primary_aovs_rays(Tensor scene, int n_spheres, Tensor origins, Tensor dirs, int passes, "
        "bool check=True) -> Tensor[]");
  m.def("occlusion(Tensor scene, int n_spheres, Tensor id, Tensor position, Tensor normal, Tensor table, Tensor rot, "
        "float max_distance, float light_radius, int passes, bool check=True) -> Tensor[]");
  m.def("trace_glass(Tensor scene, int n_spheres, Tensor glass, Tensor origins, Tensor dirs, int max_bounces, "
        "int out_kind, bool check=True) -> Tensor");
  m.def("trace_lights(Tensor scene, int n_spheres, Tensor lights, Tensor origins, Tensor dirs, int max_bounces, "
        "int out_kind, bool check=True) -> Tensor");
  m.def("trace_mesh(Tensor scene, int n_spheres, Tensor mesh, Tensor lights, Tensor origins, Tensor dirs, "
        "int max_bounces, int out_kind, bool check=True) -> Tensor");
  m.def("trace_mesh_uv(Tensor scene, int n_spheres, Tensor mesh, Tensor lights, Tensor origins, Tensor dirs, "
        "int max_bounces, int out_kind, bool check=True) -> Tensor");
  m.def("mesh_aovs(Tensor scene, int n_spheres, Tensor mesh, Tensor lights, Tensor? shape_ids, Tensor origins, "
        "Tensor dirs, int passes, bool check=True) -> Tensor[]");
  m.def("mesh_build(Tensor vertices, Tensor faces, Tensor tri_mesh, Tensor? normals, Tensor? mesh_smooth, Tensor? uvs, "
        "Tensor(a!) skeleton, int max_leaf, Tensor(b!) workspace, bool check=True) -> Tensor");
  m.def("env_sample(Tensor texels, float[] gain, float turn, Tensor dirs) -> Tensor");
  m.def("trace_lights_env(Tensor scene, int n_spheres, Tensor lights, Tensor origins, Tensor dirs, int max_bounces, "
        "int out_kind, Tensor texels, float[] gain, float turn, bool check=True) -> Tensor");
  m.def("trace_glass_env(Tensor scene, int n_spheres, Tensor glass, Tensor origins, Tensor dirs, int max_bounces, "
        "int out_kind, Tensor texels, float[] gain, float turn, bool check=True) -> Tensor");
  m.def("edge_mask(Tensor color, Tensor id, Tensor hits, Tensor lit, int width, int height, float contrast) -> Tensor");
  m.def("sample_dirs(Tensor sample_scene, int k, int width, int height, Tensor pixels) -> Tensor");
  m.def("resolve_scatter(Tensor samples, int k, Tensor pixels, int width, int height, Tensor(a!) out, "
        "int out_kind) -> ()");
  m.def("status(Tensor(a!) workspace) -> int");
  m.def("workspace_bytes(int n_rays, int max_bounces) -> int", &workspace_bytes);
  // the row-tiled multi-GPU frame (one native call per frame and rank; handles are int64)
  m.def("comm_unique_id() -> Tensor", &comm_unique_id);
  m.def("comm_init(Tensor unique_id, int world, int rank, int device=-1, int max_ctas=0) -> int", &comm_init);
  m.def("comm_destroy(int comm) -> ()", &comm_destroy);
  m.def("tiles_create(int comm, int world, int rank, int root, int width, int height, int row_block, int out_kind, "
        "int slots, Tensor[] send, Tensor[] recv, int part_bytes, int root_run=1, int run=1, int flags=0, "
        "int device=-1) -> int",
        &tiles_create);
  m.def("tiles_submit(int plan, int slot, Tensor scene, int n_spheres, int max_bounces, Tensor(a!) workspace, "
        "Tensor(b!)? frame=None, int flags=0) -> ()",
        &tiles_submit);
  m.def("tiles_finish(int plan, int slot, int device) -> ()", &tiles_finish);
  m.def("tiles_destroy(int plan) -> ()", &tiles_destroy);
}

TORCH_LIBRARY_IMPL(rt, CUDA, m) {
  m.impl("render_tile", &render_tile);
  m.impl("render_frames", &render_frames);
  m.impl("trace", &trace);
  m.impl("shade_hits", &shade_hits);
  m.impl("intersect", &intersect);
  m.impl("quantize_u8", &quantize_u8);
  m.impl("assemble_rows", &assemble_rows);
  m.impl("resolve_samples", &resolve_samples);
  m.impl("primary_aovs", &primary_aovs);
  m.impl("primary_aovs_rays", &primary_aovs_rays);
  m.impl("occlusion", &occlusion);
  m.impl("trace_glass", &trace_glass);
  m.impl("trace_lights", &trace_lights);
  m.impl("trace_mesh", &trace_mesh);
  m.impl("trace_mesh_uv", &trace_mesh_uv);
  m.impl("mesh_build", &mesh_build);
  m.impl("mesh_aovs", &mesh_aovs);
  m.impl("env_sample", &env_sample);
  m.impl("trace_lights_env", &trace_lights_env);
  m.impl("trace_glass_env", &trace_glass_env);
  m.impl("edge_mask", &edge_mask);
  m.impl("sample_dirs", &sample_dirs);
  m.impl("resolve_scatter", &resolve_scatter);
  m.impl("camera_rays", &camera_rays);
  m.impl("status", &status);
}

// Host tensors reach the same functions, whose checks raise RuntimeError ("must be a GPU tensor")
// instead of the dispatcher's "no kernel for CPU".
TORCH_LIBRARY_IMPL(rt, CPU, m) {
  m.impl("render_tile", &render_tile);
  m.impl("render_frames", &render_frames);
  m.impl("trace", &trace);
  m.impl("shade_hits", &shade_hits);
  m.impl("intersect", &intersect);
  m.impl("quantize_u8", &quantize_u8);
  m.impl("assemble_rows", &assemble_rows);
  m.impl("resolve_samples", &resolve_samples);
  m.impl("primary_aovs", &primary_aovs);
  m.impl("primary_aovs_rays", &primary_aovs_rays);
  m.impl("occlusion", &occlusion);
  m.impl("trace_glass", &trace_glass);
  m.impl("trace_lights", &trace_lights);
  m.impl("trace_mesh", &trace_mesh);
  m.impl("trace_mesh_uv", &trace_mesh_uv);
  m.impl("mesh_build", &mesh_build);
  m.impl("mesh_aovs", &mesh_aovs);
  m.impl("env_sample", &env_sample);
  m.impl("trace_lights_env", &trace_lights_env);
  m.impl("trace_glass_env", &trace_glass_env);
  m.impl("edge_mask", &edge_mask);
  m.impl("sample_dirs", &sample_dirs);
  m.impl("resolve_scatter", &resolve_scatter);
  m.impl("camera_rays", &camera_rays);
  m.impl("status", &status);
}

TORCH_LIBRARY_IMPL(rt, Meta, m) {
  m.impl("render_tile", &render_tile_meta);
  m.impl("render_frames", &render_frames_meta);
  m.impl("trace", &trace_meta);
  m.impl("shade_hits", &shade_hits_meta);
  m.impl("intersect", &intersect_meta);
  m.impl("quantize_u8", &quantize_u8_meta);
  m.impl("assemble_rows", &assemble_rows_meta);
  m.impl("resolve_samples", &resolve_samples_meta);
  m.impl("primary_aovs", &primary_aovs_meta);
  m.impl("primary_aovs_rays", &primary_aovs_rays_meta);
  m.impl("occlusion", &occlusion_meta);
  m.impl("trace_glass", &trace_glass_meta);
  m.impl("trace_lights", &trace_lights_meta);
  m.impl("trace_mesh", &trace_mesh_meta);
  m.impl("trace_mesh_uv", &trace_mesh_meta);
  m.impl("mesh_build", &mesh_build_meta);
  m.impl("mesh_aovs", &mesh_aovs_meta);
  m.impl("env_sample", &env_sample_meta);
  m.impl("trace_lights_env", &trace_lights_env_meta);
  m.impl("trace_glass_env", &trace_glass_env_meta);
  m.impl("edge_mask", &edge_mask_meta);
  m.impl("sample_dirs", &sample_dirs_meta);
  m.impl("resolve_scatter", &resolve_scatter_meta);
  m.impl("camera_rays", &camera_rays_meta);
}
