"""The PyTorch custom-op surface ``torch.ops.rt.*``, built in-tree as
``librt_ops.so`` from ``csrc/rt_ops.cpp`` over the C ABI of ``librtx_hip.so``.

    import python_ray_tracer_amd.ops  # registers torch.ops.rt
    ws = torch.zeros(torch.ops.rt.workspace_bytes(n, B), dtype=torch.uint8, device="cuda")
    rgb = torch.ops.rt.render_tile(blob, S, W, H, 1, 1, 0, B, 0, ws)      # [3, W*H] float32

Ops (each raises RuntimeError on a host tensor, a wrong dtype, a non-contiguous tensor or a short
workspace, like a TORCH_CHECK; each runs under a device guard of its input's device, enqueues on
that device's current HIP stream and returns a new tensor):

* ``rt::render_tile(scene, n_spheres, width, height, row_block, n_parts, part, max_bounces,
  out_kind, workspace, stats=None, check=True, part_run=1)`` — get_ray_directions + raytrace_scene
  fused (base.py:91-141) for one interleaved row tile, or the run of ``part_run`` parts from
  ``part`` (a rank's weighted share, distributed.ROOT_SHARES); out_kind 0 = float32 [3, n],
  1 = float64 [3, n], 2 = uint8 [rows, W, 3].
* ``rt::render_frames(scenes, n_spheres, width, height, max_bounces, out_kind, workspace,
  stats=None, check=True)`` — F whole frames in one launch (``scenes``: [F, L], one packed blob per
  row); [F, 3, W*H] colour or [F, H, W, 3] uint8 (HipRenderer.render_batch).
* ``rt::trace(scene, n_spheres, origins, dirs, max_bounces, out_kind, workspace, stats=None,
  check=True)`` — raytrace_scene on arbitrary rays (base.py:91-121); origins [3] (shared) or [3, n].
* ``rt::shade_hits(scene, n_spheres, shape, origins, dirs, t, max_bounces, out_kind, workspace,
  stats=None, check=True)`` — NumpyShader.create for rays hitting sphere ``shape`` at distances
  ``t`` [n] (shader.py:63-112; HipShader.create).
* ``rt::intersect(sphere, origins, dirs)`` — NumpySphere.intersect (shape.py:28-51).
* ``rt::quantize_u8(color)`` — save_image's quantisation (base.py:143-151) -> [n, 3] uint8.
* ``rt::assemble_rows(tiles, width, height, row_block, out_kind, root_run=1, run=1)`` — the
  multi-GPU row un-permute of ``tiles`` [ranks, part_len]: rank 0's run of ``root_run`` parts, each
  other rank's run of ``run`` (tiling.runs; 1, 1 = one part per rank).
* ``rt::resolve_samples(samples, k, width, rows, out_kind)`` — the box filter of supersampled
  anti-aliasing (HipRenderer(samples=k), rtx_resolve_samples): ``samples`` float64 [3, k*rows*k*width]
  (a float64 render of the same scene and camera position at k*width x k*rows) or [F, 3, ...];
  every sample clipped to [0, 1], the k*k of a pixel summed row by row and divided once;
  [3, rows*width] / [F, 3, rows*width] colour (out_kind 0, 1) or [rows, width, 3] /
  [F, rows, width, 3] uint8 (out_kind 2). Needs no workspace and raises on a short ``samples``.
* ``rt::primary_aovs(scene, n_spheres, width, height, row_block, n_parts, part, part_run, passes,
  check=True)`` and ``rt::primary_aovs_rays(scene, n_spheres, origins, dirs, passes, check=True)`` —
  the primary hit's intermediates as render passes (rtx_primary_aovs; HipRenderer.render_aovs /
  trace_aovs), for a row tile of the camera's frame (local row order, as render_tile) or for explicit
  rays (origins [3] or [3, n]). ``passes`` is a mask of the RTX_AOV_* bits (``_lib.AOV_*``): 1 depth
  float64 [n], 2 id int32 [n], 4 hits int32 [n], 8 position, 16 normal, 32 albedo float64 [3, n],
  64 lit uint8 [n]; the result is a list with one tensor per set bit, in bit order. A pass that is
  not requested is neither computed nor stored. Need no workspace.
* ``rt::occlusion(scene, n_spheres, id, position, normal, table, rot, max_distance, light_radius,
  passes, check=True)`` — the occlusion passes of the primary hits (rtx_occlusion;
  HipRenderer.render_occlusion / trace_occlusion; contract in include/rtx_hip.h): ``id`` int32 [n],
  ``position`` and ``normal`` float64 [3, n] as ``rt::primary_aovs`` returns them, ``table`` the device
  hemisphere table float64 [3, side*side] and ``rot`` the rotation table float64 [2, 64]
  (``occlusion.hemisphere_table``, ``occlusion.rotation_table``), ``max_distance`` in (0, 1e39],
  ``light_radius`` >= 0. ``passes`` is a mask of the RTX_OCC_* bits (``_lib.OCC_*``): 1 ao, 2 soft_lit,
  float32 [n] each; the result is a list with one tensor per set bit, in bit order. An id outside
  0..n_spheres-1 is a miss (ao 1, soft_lit 0). Every tensor's size is checked. Needs no workspace.
* ``rt::trace_glass(scene, n_spheres, glass, origins, dirs, max_bounces, out_kind, check=True)`` —
  raytrace_scene on explicit rays through a scene with solid glass spheres (rtx_trace_glass; contract in
  include/rtx_hip.h): ``glass`` is the device side table float64 [2, n_spheres]
  (``glass.glass_table``: transmission gains, indices of refraction), origins [3] (shared) or [3, n],
  ``max_bounces`` in 0..8; out_kind 0 = float32 [3, n], 1 = float64 [3, n], 2 = uint8 [n, 3]. The op
  allocates its own workspace. With ``check=True`` it reads the status word back (a synchronisation) and
  raises "maximum recursion depth exceeded" for a ray tree that overflowed a lane's stack of pending
  rays. Every tensor's dtype, device, contiguity and size is checked.
* ``rt::trace_lights(scene, n_spheres, lights, origins, dirs, max_bounces, out_kind, check=True)`` —
  raytrace_scene on explicit rays with every point light of a table (rtx_trace_lights; contract in
  include/rtx_hip.h): ``lights`` is the device table float64 [L, 6], L in 1..8
  (``lights.lights_table``: position, intensity * colour), origins [3] (shared) or [3, n],
  ``max_bounces`` in 0..16; out_kind 0 = float32 [3, n], 1 = float64 [3, n], 2 = uint8 [n, 3]. The op
  allocates its own workspace. With ``check=True`` it reads the status word back (a synchronisation) and
  raises "maximum recursion depth exceeded" for a ray tree that overflowed a lane's stack of pending
  rays. Every tensor's dtype, device, contiguity and size is checked.
* ``rt::trace_mesh(scene, n_spheres, mesh, lights, origins, dirs, max_bounces, out_kind, check=True)`` —
  raytrace_scene on explicit rays through the spheres of ``scene`` (``n_spheres`` may be 0) and the triangles
  of ``mesh`` (rtx_trace_mesh; contract in include/rtx_hip.h): ``mesh`` is the device table
  float64 [words] of ``meshes.mesh_table``, ``lights`` the table float64 [L, 6] of ``rt::trace_lights``,
  ``max_bounces`` in 0..16; origins, out_kind, workspace and ``check`` as ``rt::trace_lights``. With
  ``check=True`` the mesh table's header is read back and checked against its length too. Every tensor's
  dtype, device, contiguity and size is checked.
* ``rt::trace_mesh_uv(scene, n_spheres, mesh, lights, origins, dirs, max_bounces, out_kind, check=True)`` —
  ``rt::trace_mesh`` on a table with texture coordinates and texel blocks (rtx_trace_mesh_uv):
  the table ``meshes.mesh_table`` builds when a mesh has an ``ImageTexture``. With ``check=True`` the offsets
  of the two new parts are checked against the table's length as well.
* ``rt::mesh_aovs(scene, n_spheres, mesh, lights, shape_ids, origins, dirs, passes, check=True)`` — the
  primary-hit render passes of a mesh scene for explicit rays (rtx_mesh_aovs; HipRenderer.render_mesh_aovs /
  trace_mesh_aovs; contract in include/rtx_hip.h): ``scene``, ``mesh``, ``lights``, origins and
  dirs as ``rt::trace_mesh`` takes them (a table with a UV part too), ``shape_ids`` int32 [n_spheres + meshes] or
  None (what ``id`` reports per sphere, then per mesh; None: the position in that order). ``passes`` is a mask of
  the RTX_MESH_AOV_* bits (``_lib.MESH_AOV_PASSES``): 1 depth float64 [n], 2 id, 4 hits int32 [n], 8 position,
  16 normal, 32 geometric_normal, 64 albedo float64 [3, n], 128 lit uint8 [n] (bit i: lights row i), 256 triangle
  int32 [n], 512 bary float64 [2, n]; the result is a list with one tensor per set bit, in bit order. A pass
  that is not requested is neither computed nor stored. With ``check=True`` the headers of the blob and of the
  mesh table are read back and ``shape_ids``' length is checked against the table's mesh count. Needs no
  workspace.
* ``rt::mesh_build(vertices, faces, tri_mesh, normals, mesh_smooth, uvs, skeleton, max_leaf, workspace,
  check=True)`` — the table of ``rt::trace_mesh`` / ``rt::trace_mesh_uv`` made on the device (rtx_mesh_build;
  contract in include/rtx_hip.h): the device arrays of ``meshes.device_inputs`` (float64 [V, 3],
  int32 [T, 3], int32 [T], float64 [V, 3] and int32 [M] or None, float64 [T, 6] or None), ``skeleton`` its
  float64 [words] skeleton, filled in place to the values of ``meshes.mesh_table``, ``max_leaf`` the leaf size
  (0: one leaf), ``workspace`` uint8 of at least ``rtx_mesh_build_workspace_bytes``. Returns the build's status
  words, int32 [2]: the lowest degenerate triangle (-1: none) and whether an index was out of range. The
  skeleton's header is read back (one small synchronous copy); with ``check=True`` a skeleton shorter than its
  header says and a workspace that is too small raise here, and so does a degenerate triangle (a
  synchronisation); with ``check=False`` the library's own error codes and the status words speak.
* ``rt::env_sample(texels, gain, turn, dirs)``, ``rt::trace_lights_env(scene, n_spheres, lights, origins, dirs,
  max_bounces, out_kind, texels, gain, turn, check=True)`` and ``rt::trace_glass_env(scene, n_spheres, glass,
  origins, dirs, max_bounces, out_kind, texels, gain, turn, check=True)`` — the environment map (rtx_env_sample,
  rtx_trace_lights_env, rtx_trace_glass_env; contract in include/rtx_hip.h): ``texels`` is the
  device image float32 [H, W, 4] (RGB and a zero word: ``EnvironmentLight.texels``), at most 2^23 texels,
  ``gain`` three finite numbers (intensity * colour), ``turn`` the rotation about +y in turns (degrees / 360).
  ``env_sample`` returns env(D) of ``dirs`` float64 [3, n] as float64 [3, n]: the lookup alone. The other two
  are ``rt::trace_lights`` / ``rt::trace_glass`` (same arguments, checks, workspace and ``check``) where a ray
  that meets no shape returns env(D) instead of black, at every level; a blob of another sphere count (with
  ``check=False``) makes every ray such a ray. Every tensor's dtype, device, contiguity and size is checked.
* ``rt::edge_mask(color, id, hits, lit, width, height, contrast)``, ``rt::sample_dirs(sample_scene,
  k, width, height, pixels)`` and ``rt::resolve_scatter(samples, k, pixels, width, height, out,
  out_kind)`` — the three steps of adaptive anti-aliasing (HipRenderer(samples=k, adaptive=True);
  rtx_edge_mask, rtx_sample_dirs, rtx_resolve_scatter; contract in include/rtx_hip.h): the uint8
  [width*height] mask of the pixels to refine, from a float64 [3, width*height] frame and its ``id`` /
  ``hits`` (int32) and ``lit`` (uint8) passes (``contrast`` >= 0, ``inf`` for the geometric test alone);
  the float64 [3, n*k*k] sample directions of the int32 pixel indices ``pixels`` [n] on the packed
  sample scene (the same scene with a k*width x k*height camera); and the resolve of float64
  [3, n*k*k] samples written over the listed pixels of ``out`` ([3, width*height] colour or
  [height, width, 3] uint8, mutated in place; nothing is returned). Every tensor's size is checked.
* ``rt::camera_rays(cam, lens, k, width, height, row_block=1, n_parts=1, part=0, part_run=1)`` — the
  sample rays of a perspective camera (domain.PerspectiveCamera; rtx_camera_rays, contract in
  include/rtx_hip.h) for a row tile of its frame: ``cam`` is the camera record, a HOST float64
  [24] tensor (``camera.camera_record``; it travels as a kernel argument), ``lens`` the device lens
  table float64 [2, k*k] (``camera.lens_table``) or None. Returns ``(origins, dirs)``, float64
  [3, k*k*width*rows] each in the order of a sample frame's rows (what ``rt::resolve_samples`` reads);
  ``origins`` is None without a lens table (the rays share the origin ``cam[0:3]``, and land on the
  current device). A record with a lens and no table raises. Both tensors' sizes are checked.
* ``rt::status(workspace)`` — reads and clears the sticky RTX_ST_* flags (1 stack overflow,
  2 deferred-list overflow, 4 bad scene); synchronises.
* ``rt::workspace_bytes(n_rays, max_bounces)``.

Error channel of the render ops: with ``check=True`` (the default) a scene blob whose header
disagrees with ``n_spheres`` raises before the launch (one small synchronous header copy), and a
launch that may defer chains past the fast kernel's levels (max_bounces -1 or > 6) reads and clears
the status word afterwards (a synchronisation), raising "maximum recursion depth exceeded" where
HipRenderer raises RecursionError. ``check=False`` keeps the op asynchronous (no host
synchronisation); call ``rt::status(workspace)`` later. ``stats`` and ``workspace`` are declared
as mutated (``Tensor(a!)``, ``Tensor(b!)?``) and every op has a Meta (fake) kernel, so the ops
trace under FakeTensor / torch.compile.

max_bounces -1 is the reference's unbounded recursion. There is no CPU implementation: importing
this module without the built library raises ImportError.
"""

from __future__ import annotations

from pathlib import Path

import torch

from python_ray_tracer_amd.infrastructure.hip import _lib

OPS_LIB = Path(__file__).resolve().parent / "librt_ops.so"
RTX_LIB = Path(__file__).resolve().parent / "librtx_hip.so"  # what librt_ops.so links by $ORIGIN
OPS = ("render_tile", "render_frames", "trace", "shade_hits", "intersect", "quantize_u8", "assemble_rows",
       "resolve_samples", "primary_aovs", "primary_aovs_rays", "occlusion", "trace_glass", "trace_lights", "trace_mesh",
       "trace_mesh_uv", "mesh_build", "mesh_aovs", "env_sample",
       "trace_lights_env", "trace_glass_env", "edge_mask", "sample_dirs", "resolve_scatter", "camera_rays",
       "status", "workspace_bytes",
       # the row-tiled multi-GPU frame (rtx_tiles_*: render, RCCL gather, assembly in one native call)
       "comm_unique_id", "comm_init", "comm_destroy", "tiles_create", "tiles_submit", "tiles_finish",
       "tiles_destroy")


def load() -> None:
    """Register torch.ops.rt (idempotent)."""
    if hasattr(torch.ops, "rt") and hasattr(torch.ops.rt, "workspace_bytes"):
        try:
            torch.ops.rt.workspace_bytes  # noqa: B018 - resolves only once the library is loaded
            return
        except (AttributeError, RuntimeError):
            pass
    # librt_ops.so resolves the C ABI from the librtx_hip.so beside it ($ORIGIN). A variant library
    # named by RTX_HIP_LIB (tools/ab.py builds) would give the ops and HipRenderer two different
    # kernels in one process: refuse to register rather than mix them.
    if _lib.LIB_PATH.resolve() != RTX_LIB.resolve():
        raise ImportError(f"torch.ops.rt links {RTX_LIB}, but RTX_HIP_LIB selects {_lib.LIB_PATH}: the ops and "
                          "HipRenderer would run different libraries; unset RTX_HIP_LIB to use the ops")
    _lib.load()  # the C ABI first: same file, same handle
    if not OPS_LIB.exists():
        raise ImportError(f"{OPS_LIB} not found; build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    torch.ops.load_library(str(OPS_LIB))


load()
