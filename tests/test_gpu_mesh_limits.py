"""The mesh kernels (rtx_trace_mesh, rtx_trace_mesh_uv) where tests/test_gpu_mesh.py and
tests/test_gpu_meshuv.py do not reach.

* A worker's second item: frames and ray sets larger than the pool of workers (taken from the library, never
  from a constant here), at the caps with the fixed pool and at cap 16, whose pool the 256 MiB budget sets.
* The stack of 2B + 2 pending rays filled to its last entry, and overflowed by one: the kernel drops the ray
  and sets RTX_ST_STACK_OVERFLOW, the renderer raises RecursionError and the op RuntimeError. The kernel
  guards every push, so nothing is written out of bounds: the tests read an error channel.
* Incoherent rays in one wave, through a scene near the origin and far from it, large and small; the deepest
  trees (the benchmark's largest table among them); rays aimed at vertices and edges; a box met from six
  sides along its faces, edges and corners with exact arithmetic.

The bars: float64 colour within 1e-12 * max(1, |colour|) of the restatement, every triangle tried for every
ray, and the same uint8 values, no ray excluded; for a scene of size s translated to c the bar is scaled by
max(1, |c| / s) (derived in DESIGN.md §17, not measured). tests/test_mesh_limits_cpu.py pins what each case
exercises and that the tree's emulated pruning changes none of its rays.
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes, scenes, tiling
from tests import mesh_ref as R
from tests import meshuv_ref as U
from tests.test_mesh_limits_cpu import (LAPS, RAYS, RTOL, TIE_LANES, TIE_PIXEL, box_case, lap_case, origins_case, ray_case,
                                        second_lap_rows, tie_case, trace_spec)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _check(got, want, w, h, what="", atol=RTOL):
    """float64 colour within the bar of the restatement's, and the same uint8 values."""
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"{what}: max |gpu - ref| / max(1, |ref|) = {err:.3e} (bar {atol:.2e}, colours up to {want.max():.3f})")
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert err <= atol, (what, err)
    assert np.array_equal(O.to_uint8(got, w, h), O.to_uint8(want, w, h)), what


class _Calls:
    """The renderer's library with its calls counted by name: which entry a render went through."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def _vec(hip, a):
    """Three rows of a host array as a device HipVector3D."""
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(a))).cuda()
    return hip.HipVector3D(dev[0], dev[1], dev[2])


def _entry(uv):
    return "rtx_trace_mesh_uv" if uv else "rtx_trace_mesh"


def _trace(hip, spec, o, d, cap, uv=False, max_leaf=4, r=None):
    """Explicit rays with one origin each through the renderer; through the entry named by ``uv`` alone."""
    r = hip.HipRenderer(cap) if r is None else r
    r.mesh_max_leaf = max_leaf
    lib = r._lib
    r._lib = calls = _Calls(lib)
    try:
        got = r.raytrace_scene(_vec(hip, o), _vec(hip, d), scenes.build_scene(spec)).data.cpu().numpy()
    finally:
        r._lib = lib
    assert [n for n in calls.names if n.startswith("rtx_trace")] == [_entry(uv)], calls.names
    return got


def _op_args(r, scene, spec):
    """(blob, n_spheres, mesh table, lights table, eye, directions) of ``scene``'s own frame for rt::trace_mesh."""
    import python_ray_tracer_amd.ops  # noqa: F401

    blob, S = r.scene_blob(scene)
    mesh = torch.tensor(meshes.mesh_table(scene.shapes)).cuda()
    table = torch.from_numpy(R.table_of(spec)).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    return blob, S, mesh, table, eye, dirs


# ---- frames and ray sets larger than the pool of workers -----------------------------------------------------

@pytest.mark.parametrize("key", [k for k in sorted(LAPS) if k != "lights"])
def test_frames_larger_than_the_pool(hip, key):
    """The full frame equals the same frame in row tiles, none of which reaches a second lap, bit for bit;
    rows of both laps against the restatement; the uint8 and the float32 frame are the float64 frame's."""
    spec, cap, p, rows, want = lap_case(key)
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    uv = LAPS[key][1] is U
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    r._lib = calls = _Calls(r._lib)
    flat = r.render(scene).data.cpu().numpy()
    assert calls.names.count(_entry(uv)) == 1 and flat.shape == (3, W * H)
    full = flat.reshape(3, H, W)
    for part in range(4):
        tile_rows = tiling.tile_rows(H, 8, 4, part)
        assert W * len(tile_rows) < p
        tile = r.render_tile(scene, 8, 4, part).cpu().numpy()
        assert np.array_equal(tile, full[:, tile_rows].reshape(3, -1)), part
    _check(full[:, rows].reshape(3, -1), want, W, len(rows), f"{key}, rows {rows}")
    lap2 = second_lap_rows(key)
    first = [row for row in rows if row not in lap2]
    _check(full[:, first].reshape(3, -1), want[:, :len(first) * W], W, len(first), f"{key}, the workers' first items")
    _check(full[:, lap2].reshape(3, -1), want[:, len(first) * W:], W, len(lap2), f"{key}, the workers' second items")
    u8 = r.render_tile(scene, out="u8")
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
    assert np.array_equal(u8.cpu().numpy(), O.to_uint8(flat, W, H))
    if cap == 3:
        got32 = hip.HipRenderer(cap, color_dtype=torch.float32).render(scene).data
        assert got32.dtype == torch.float32
        assert np.array_equal(got32.cpu().numpy(), flat.astype(np.float32))  # the float64 value rounded once


def test_a_ray_count_that_ends_inside_a_wave_of_the_second_lap(hip):
    spec, cap, p, rows, want = lap_case("mesh")
    W = spec["camera"]["width"]
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S, mesh, table, eye, dirs = _op_args(r, scene, spec)
    n = p + 64 * 3 + 17
    assert p < n < dirs.shape[1] and n % 64 != 0
    out = torch.ops.rt.trace_mesh(blob, S, mesh, table, eye, dirs[:, :n].contiguous(), cap, 1)
    assert tuple(out.shape) == (3, n) and torch.equal(out, full[:, :n])
    row = p // W  # the row in which the second lap begins: its second items that were traced, against the restatement
    end = min(n, (row + 1) * W)
    want_row = R.render(spec, cap, rows=[row])[:, p - row * W:end - row * W]
    _check(out[:, p:end].cpu().numpy(), want_row, end - p, 1, f"the second items {p}..{end} of the first {n} rays")


def test_explicit_rays_with_per_ray_origins_larger_than_the_pool(hip):
    """One origin per ray (org_stride = n) read at i >= n_workers: the frame's rays pulled back along their
    directions; the first rays, the rays that straddle the pool and the last against the restatement."""
    spec, cap, p, o, d, idx, want = origins_case()
    got = _trace(hip, spec, o, d, cap)
    assert got.shape == d.shape and np.isfinite(got).all()
    _check(got[:, idx], want, idx.size, 1, "per-ray origins")
    _check(got[:, idx[idx >= p]], want[:, idx >= p], int((idx >= p).sum()), 1, "per-ray origins, the workers' second items")


# ---- the stack at its capacity and over it -------------------------------------------------------------------

@pytest.mark.parametrize("uv", [False, True], ids=["mesh", "mesh_uv"])
def test_a_stack_filled_to_its_last_entry(hip, uv):
    """Three coincident spheres and a triangle at one distance at B = 1: the tie ray pushes 4 rays into 4
    entries (the last push at sp == cap - 1), nothing is reported, in a frame and at lanes 0, 31, 63 and 101."""
    spec, want, need, e, want_e, need_e = tie_case(3, uv)
    assert need.max() == need_e.max() == 4 == 2 * 1 + 2
    r = hip.HipRenderer(1)
    r._lib = calls = _Calls(r._lib)
    got = r.render(scenes.build_scene(spec)).data.cpu().numpy()
    assert calls.names.count(_entry(uv)) == 1
    r._lib = calls._lib
    _check(got, want, 17, 17, "three coincident spheres and a triangle")
    print(f"the tie ray: {got[:, TIE_PIXEL].tolist()}")
    cam = [float(c) for c in spec["camera"]["position"]]
    o = np.repeat(np.array(cam).reshape(3, 1), e.shape[1], axis=1)
    got_e = _trace(hip, spec, o, e, 1, uv, r=r)
    _check(got_e, want_e, e.shape[1], 1, "the tie ray at lanes 0, 31, 63, 101 and 144")
    for lane in TIE_LANES:
        assert np.array_equal(got_e[:, lane], got[:, TIE_PIXEL])


@pytest.mark.parametrize("uv", [False, True], ids=["mesh", "mesh_uv"])
def test_an_overflowing_render_raises_every_time_and_leaves_nothing_behind(hip, uv):
    """Four coincident spheres and the triangle need 5 entries of 4, one more than the stack (a guard of
    sp <= cap would hold it, one entry past the end): RecursionError, again on the identical render (an
    overflowing key is not remembered as clean), and the same renderer, with the same workspace, then renders
    scenes that fit: the sticky flag was cleared and the stacks hold nothing that matters."""
    spec4, _, need4, e4, _, need_e4 = tie_case(4, uv)
    assert need4.max() == need_e4.max() == 5 == 2 * 1 + 2 + 1
    r = hip.HipRenderer(1)
    over = scenes.build_scene(spec4)
    for _ in range(2):
        with pytest.raises(RecursionError, match="maximum recursion depth exceeded.*more than 4 pending rays at max_bounces=1"):
            r.render(over)
    cam = [float(c) for c in spec4["camera"]["position"]]
    o = np.repeat(np.array(cam).reshape(3, 1), e4.shape[1], axis=1)
    with pytest.raises(RecursionError, match="more than 4 pending rays at max_bounces=1"):
        r.raytrace_scene(_vec(hip, o), _vec(hip, e4), over)
    spec3, want3 = tie_case(3, uv)[:2]
    _check(r.render(scenes.build_scene(spec3)).data.cpu().numpy(), want3, 17, 17, "three coincident spheres after an overflow")
    plain = scenes.mesh_spec(32, 18, 1)
    _check(r.render(scenes.build_scene(plain)).data.cpu().numpy(), R.render(plain, 1), 32, 18, "mesh_spec after an overflow")
    with pytest.raises(RecursionError, match="more than 4 pending rays at max_bounces=1"):  # and after clean renders
        r.render(over)


@pytest.mark.parametrize("uv", [False, True], ids=["mesh", "mesh_uv"])
def test_an_overflow_through_the_op(hip, uv):
    """The lanes that fit are within the bar although lanes of their waves overflow; an overflowed lane lost
    the triangle's reflected ray, which meets the sphere behind the eye: its colour differs."""
    spec, _, _, e, want, need = tie_case(4, uv)
    scene = scenes.build_scene(spec)
    blob, S, mesh, table, eye, _ = _op_args(hip.HipRenderer(1), scene, spec)
    trace = torch.ops.rt.trace_mesh_uv if uv else torch.ops.rt.trace_mesh
    dirs = torch.from_numpy(np.ascontiguousarray(e)).cuda()
    with pytest.raises(RuntimeError, match="maximum recursion depth"):
        trace(blob, S, mesh, table, eye, dirs, 1, 1)
    with pytest.raises(RuntimeError, match="maximum recursion depth"):
        trace(blob, S, mesh, table, eye, dirs, 1, 1, check=True)
    got = trace(blob, S, mesh, table, eye, dirs, 1, 1, check=False).cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    fits = need <= 4
    assert int((~fits).sum()) == len(TIE_LANES) + 1
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    err = float(rel[:, fits].max())
    off = int((rel[:, ~fits] > RTOL).any(axis=0).sum())
    print(f"lanes that fit: max |gpu - ref| = {err:.3e}; {off} of the {int((~fits).sum())} overflowed lanes differ")
    assert err <= RTOL  # only the overflowed lanes may differ
    assert off > 0  # (they dropped a ray)


# ---- incoherent rays, scale and distance, deep trees, edges, the box -----------------------------------------

@pytest.mark.parametrize("name", sorted(RAYS))
def test_rays_against_the_restatement(hip, name):
    """Rays that share no origin and no direction in a wave, through scenes placed near and far, large and
    small, with trees up to the benchmark's, and at vertices and edges: every decision as the restatement
    takes it; at the small tables the leaf size changes no bit."""
    spec, o, d, cap, want, c, atol, uv = ray_case(name)
    n = d.shape[1]
    got = _trace(hip, spec, o, d, cap, uv)
    _check(got, want, n, 1, name, atol)
    if RAYS[name][2] <= 2:
        for leaf in (1, None):
            assert np.array_equal(_trace(hip, spec, o, d, cap, uv, max_leaf=leaf), got), leaf


def test_a_box_from_six_sides_exactly(hip):
    """Axis-parallel rays (two exact zeros, some of them -0.0) through faces, along faces, edges and the
    faces' diagonals, from inside and past the box: the hits and misses tests/test_mesh_limits_cpu.py names."""
    spec, o, d, want_t = box_case()
    want = trace_spec(spec, o, d, 3)
    got = _trace(hip, spec, o, d, 3)
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"box: max err {err:.3e}")
    assert err <= RTOL and np.array_equal(got == 0, want == 0)
    assert np.array_equal(got.any(axis=0), np.array(want_t) != meshes.FARAWAY)
    for leaf in (1, 2, None):
        assert np.array_equal(_trace(hip, spec, o, d, 3, max_leaf=leaf), got), leaf
