// rtx_internal.h — what the translation units of librtx_hip.so share on the host side (every unit
// includes it; rtx_tiles.hip, which has no device code, only this): the functions one unit defines
// and another calls, declared once, the error and launch checks behind rtx_last_error(), the
// row-tile geometry, and the Params of the two kinds of launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "../../include/rtx_hip.h"

#define RTX_HIDDEN __attribute__((visibility("hidden")))

// rtx_kernels.hip: sets the calling thread's error message (rtx_last_error) and returns code.
RTX_HIDDEN int rtx_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// rtx_kernels.hip: the launch record behind rtx_last_launches (a test hook): one entry per k_render_fast
// launch of the calling thread's current render call, written where the launch names its template
// arguments (rtx_kernels.hip's launch_k, rtx_small.hip's go), so it tells which build ran.
RTX_HIDDEN void rtx_note_launch(int B, int lds, int deep, int stats, int tp, int img, int nsph, int waves, dim3 grid,
                                int n_fetch, int ordered, uint32_t lds_bytes);
// rtx_small.hip: launches k_render_fast<B, true, deep, stats, 0, img>(*params) on s (events e0/e1 as
// hipExtLaunchKernelGGL's); hipErrorInvalidValue, nothing launched, for an instantiation the unit
// does not carry.
RTX_HIDDEN hipError_t rtx_launch_small(int B, int deep, bool stats, bool img, const void* params, dim3 grid,
                                       uint32_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1);

namespace {

// After a kernel launch (or a runtime call) named `what`: RTX_OK, or RTX_E_LAUNCH and the message
// "what: <the HIP error>". refused: an error the launch path itself noted (rtx_launch_small's).
inline int rtx_launched(const char* what, hipError_t refused = hipSuccess) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = refused;
  return e == hipSuccess ? RTX_OK : rtx_fail(RTX_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

__host__ __device__ __forceinline__ int64_t out_bytes_per_pixel(int kind) {
  return kind == RTX_OUT_F32_SOA ? 12 : kind == RTX_OUT_F64_SOA ? 24 : 3;
}

// Rows of the run of `run` parts from part p of the interleaved row tiling (python_ray_tracer_amd/
// tiling.py n_local_rows): run * row_block rows of every cycle, the last cycle's prefix.
__host__ __device__ __forceinline__ int tile_local_rows(int height, int row_block, int n_parts, int p, int run = 1) {
  const int cycle = row_block * n_parts, own = row_block * run;
  const int q = height / cycle, rem = height % cycle - p * row_block;
  return q * own + (rem < 0 ? 0 : rem > own ? own : rem);
}
// The rank that owns block-in-cycle b when rank 0 runs parts [0, root_run) and rank i >= 1 parts
// [root_run + (i - 1) run, root_run + i run): its index, first part and run length.
__host__ __device__ __forceinline__ void run_owner(int b, int root_run, int run, int& rank, int& first, int& len) {
  if (b < root_run) {
    rank = 0, first = 0, len = root_run;
  } else {
    rank = 1 + (b - root_run) / run, first = root_run + (rank - 1) * run, len = run;
  }
}

// A row tile of a frame: n_local_rows rows of the run of part_run parts from `part` of the n_parts-way
// interleave, at most the rows that run owns.
inline bool tile_geometry_ok(int width, int height, int row_block, int n_parts, int part, int part_run,
                             int n_local_rows) {
  return width > 0 && height > 0 && row_block > 0 && n_parts > 0 && part >= 0 && part_run >= 1 &&
         part_run <= n_parts - part && n_local_rows >= 0 &&
         n_local_rows <= tile_local_rows(height, row_block, n_parts, part, part_run);
}

// The Params (rtx_device.h; a template parameter only because rtx_tiles.hip includes this header
// without the device text) of a camera launch over a row tile, and of a launch of n explicit rays
// (mode 1, or 3: with a given level-0 hit). p is value-initialised by the caller.
template <typename P>
void camera_params(P& p, const double* scene, int n_spheres, int width, int height, int row_block, int n_parts,
                   int part, int part_run, int n_local_rows) {
  p.scene = scene;
  p.nsph = n_spheres;
  p.mode = 0;
  p.width = width;
  p.height = height;
  p.row_block = row_block;
  p.n_parts = n_parts;
  p.part = part;
  p.part_run = part_run;
  p.n_rows = n_local_rows;
  p.n = (int64_t)width * n_local_rows;
}
template <typename P>
void ray_params(P& p, const double* scene, int n_spheres, int mode, const double* origins, int64_t origin_stride,
                const double* dirs, int64_t n) {
  p.scene = scene;
  p.nsph = n_spheres;
  p.mode = mode;
  p.org = origins;
  p.org_stride = origin_stride;
  p.dir = dirs;
  p.n = n;
}

// What the launchers of the kernels with a stack of pending rays check alike (rtx_trace_glass, rtx_trace_lights,
// rtx_trace_mesh and their _env and _uv forms), in the two halves that stand before and after a launcher's own
// range checks (sphere and table counts, the bounce cap), so that every entry fails first where it did: RTX_OK, or
// the code rtx_fail returned. `tables`: the launcher's side tables, each with its message for a null pointer.
struct StackTable {
  const void* ptr;
  const char* null_message;
};
inline int stack_call_pointers(const void* scene, std::initializer_list<StackTable> tables, const void* origins,
                               const void* dirs, const void* out, const void* workspace) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  for (const StackTable& t : tables)
    if (!t.ptr) return rtx_fail(RTX_E_ARG, "%s", t.null_message);
  if (!origins || !dirs) return rtx_fail(RTX_E_ARG, "null ray pointer (origins, dirs)");
  if (!out) return rtx_fail(RTX_E_ARG, "null output pointer");
  if (!workspace) return rtx_fail(RTX_E_ARG, "null workspace pointer");
  return RTX_OK;
}
// `need`: the bytes the launcher's size function (`size_fn`, named in the message) asks for n rays.
inline int stack_call_rays(int out_kind, int64_t n, int64_t origin_stride, size_t workspace_bytes, size_t need,
                           const char* size_fn) {
  if (out_kind != RTX_OUT_F32_SOA && out_kind != RTX_OUT_F64_SOA && out_kind != RTX_OUT_U8_HWC)
    return rtx_fail(RTX_E_ARG, "bad out_kind %d", out_kind);
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative ray count");
  if (origin_stride != 0 && origin_stride != n)
    return rtx_fail(RTX_E_ARG, "origin_stride must be 0 (a shared origin) or n");
  if (workspace_bytes < need)
    return rtx_fail(RTX_E_WORKSPACE, "workspace too small: %zu < %zu bytes (%s)", workspace_bytes, need, size_fn);
  return RTX_OK;
}

// The ray, output, status and stack fields that the Params of those kernels share (GlassParams, LightsParams,
// MeshParams), over a workspace that passed stack_call_rays. p is value-initialised by the caller.
template <typename P>
void stack_params(P& p, const double* origins, int64_t origin_stride, const double* dirs, int64_t n, int max_bounces,
                  void* out, int out_kind, void* workspace, int64_t n_workers) {
  p.org = origins;
  p.org_stride = origin_stride;
  p.dir = dirs;
  p.n = n;
  p.max_bounces = max_bounces;
  p.out = out;
  p.out_kind = out_kind;
  p.status = (uint32_t*)workspace + RTX_WS_STATUS;
  p.stack = (double*)((uint8_t*)workspace + RTX_WS_HDR_BYTES);
  p.n_workers = n_workers;
}

}  // namespace
