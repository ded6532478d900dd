"""Primary-hit render passes of mesh scenes on the GPU: HipRenderer.render_mesh_aovs / trace_mesh_aovs,
rt::mesh_aovs, rtx_mesh_aovs.

Every comparison with the restatement (tests/mesh_aov_ref.py, every triangle tried for every ray) is
np.array_equal, dtype and shape included, with no tolerance: every pass is a decided value or the same
correctly rounded operations in the same order. tests/test_mesh_aov_cpu.py builds the cases and asserts what
each of them shows (the counts of the frames, the ties, the sphere that only a triangle shadows)."""

import copy

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes, scenes, tiling
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import aov_ref
from tests import mesh_aov_ref as A
from tests import mesh_ref as R
from tests.test_mesh_aov_cpu import (FRAMES, NAMES, H, W, bad_argument_calls, deep_rays, frame, ico_tie_rays,
                                     interleaved_scene, quad_shadow_spec, tie_rays)
from tests.test_mesh_limits_cpu import TIE_LANES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def host(passes: dict) -> dict:
    return {k: v.cpu().numpy() for k, v in passes.items()}


def same(got: dict, want: dict, names=NAMES, what=""):
    assert tuple(got) == tuple(names), (what, tuple(got))
    for k in names:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(-1, g.shape[-1]).any(axis=0))[0]
            raise AssertionError(f"{what}: pass {k} differs at {bad.size} rays, first {bad[:8].tolist()}: "
                                 f"{g[..., bad[0]].tolist()} != {w[..., bad[0]].tolist()}")


def _vec(hip, a):
    """Three rows of a host array as a device HipVector3D."""
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(a))).cuda()
    return hip.HipVector3D(dev[0], dev[1], dev[2])


class _Calls:
    """The renderer's library with its calls counted by name: which entry a call went through."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


# ---- frames ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(FRAMES))
def test_frames_against_the_restatement(hip, key):
    spec, want = frame(key)
    r = hip.HipRenderer(3)
    r._lib = calls = _Calls(r._lib)
    got = host(r.render_mesh_aovs(scenes.build_scene(spec)))
    assert calls.names.count("rtx_mesh_aovs") == 1 and not any(n.startswith(("rtx_trace", "rtx_render")) for n in calls.names)
    same(got, want, what=key)


def test_ids_are_indices_into_the_scene_shapes(hip):
    scene, spec, ids = interleaved_scene()
    got = host(hip.HipRenderer(3).render_mesh_aovs(scene))
    same(got, A.of_spec(spec, shape_ids=ids), what="mesh, sphere, mesh, sphere, mesh")
    assert set(np.unique(got["id"])) == {-1, 0, 1, 2, 3, 4}
    shape_index, face_index = meshes.triangle_faces(scene.shapes, got["triangle"])
    tri = got["triangle"] >= 0
    assert np.array_equal(shape_index[tri], got["id"][tri]) and (shape_index[~tri] == -1).all()
    for si in (0, 2, 4):  # the barycentric point of the mesh's own face is the position
        sel = np.nonzero(shape_index == si)[0]
        assert sel.size > 90
        v = np.asarray(scene.shapes[si].vertices, dtype=np.float64)
        f = np.asarray(scene.shapes[si].faces)[face_index[sel]]
        u, w = got["bary"][0, sel], got["bary"][1, sel]
        p = v[f[:, 0]].T * (1 - u - w) + v[f[:, 1]].T * u + v[f[:, 2]].T * w
        assert np.abs(p - got["position"][:, sel]).max() < 1e-9


# ---- ties and shadows, as explicit rays ----------------------------------------------------------------------

def test_a_sphere_and_the_triangle_group_at_one_distance(hip):
    spec, eye, e, want = tie_rays()
    scene = scenes.build_scene(spec)
    got = host(hip.HipRenderer(1).trace_mesh_aovs(scene.camera.position, _vec(hip, e), scene))
    same(got, want, what="three coincident spheres and a triangle")
    for lane in TIE_LANES:
        assert (got["hits"][lane], got["id"][lane], got["triangle"][lane], got["depth"][lane]) == (4, 0, -1, 4.0)
        assert np.array_equal(got["normal"][:, lane], [0.0, 0.0, -1.0])


def test_two_triangles_at_one_distance_give_the_lowest_number(hip):
    spec, o, d, want, shared, wave = ico_tie_rays()
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    got = host(r.trace_mesh_aovs(_vec(hip, o), _vec(hip, d), scene))
    same(got, want, what="rays at the vertices and edges of the flat icosphere")
    assert (got["hits"][shared] == 1).all() and np.array_equal(got["triangle"][shared], want["triangle"][shared])
    one = host(r.trace_mesh_aovs(_vec(hip, o[:, wave]), _vec(hip, d[:, wave]), scene))  # one wave of them
    same(one, {k: np.ascontiguousarray(v[..., wave]) for k, v in want.items()}, what="one wave")
    assert one["triangle"][0] >= 0 and one["id"][31] == -1 and one["id"][63] >= 0 and one["triangle"][63] == -1


def test_a_sphere_that_only_a_triangle_shadows(hip):
    r = hip.HipRenderer(3)
    near = host(r.render_mesh_aovs(scenes.build_scene(quad_shadow_spec(True))))
    far = host(r.render_mesh_aovs(scenes.build_scene(quad_shadow_spec(False))))
    same(near, A.of_spec(quad_shadow_spec(True)), what="the quad between")
    same(far, A.of_spec(quad_shadow_spec(False)), what="the quad aside")
    on = near["id"] == 0
    assert int((on & (near["lit"] == 0)).sum()) == 28 and (far["lit"][on] == 1).all()


# ---- subsets, tiles, cameras, tables --------------------------------------------------------------------------

def test_every_subset_is_the_all_pass_call(hip):
    spec, want = frame("lights")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    full = host(r.render_mesh_aovs(scene))
    same(full, want, what="all ten")
    for names in [(k,) for k in NAMES] + [("depth", "id"), ("id", "depth"), ("bary", "lit", "hits"), NAMES]:
        part = host(r.render_mesh_aovs(scene, passes=names))
        order = tuple(k for k in NAMES if k in names)
        same(part, full, order, names)
    one = host(r.render_mesh_aovs(scene, passes="triangle"))
    same(one, full, ("triangle",))


def test_a_misaligned_lit_plane_through_the_c_entry(hip):
    spec, want = frame("lights")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    blob, S = r.scene_blob(scene)
    table = r._mesh_table(scene, "test")
    dev, lt = r._mesh_device_tables(table)
    dirs = r.get_ray_directions(scene.camera).data
    n = W * H
    eye = blob.data_ptr() + 8 * L.H_CAM
    buf = torch.full((n + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    aligned = torch.empty(n, dtype=torch.uint8, device="cuda")
    for lit in (buf.data_ptr() + 1, aligned.data_ptr()):
        outs = [None] * 7 + [lit, None, None]
        L.check(r._lib.rtx_mesh_aovs(blob.data_ptr(), S, dev.data_ptr(), int(dev.numel()), lt.data_ptr(), int(lt.shape[0]),
                                     None, eye, 0, dirs.data_ptr(), n, *outs, None), "rtx_mesh_aovs")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 4 == 0 and aligned.data_ptr() % 4 == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:n + 1], aligned.cpu().numpy()) and np.array_equal(got[1:n + 1], want["lit"])
    assert got[0] == 0xEE and (got[n + 1:] == 0xEE).all()  # nothing is written around the plane


def test_row_tiles_are_the_rows_of_the_frame(hip):
    spec, want = frame("mesh")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    shaped = {k: v.reshape(v.shape[:-1] + (H, W)) for k, v in want.items()}
    empty = 0
    for rb, P, part, run in ((1, 1, 0, 1), (4, 3, 0, 1), (4, 3, 1, 1), (4, 3, 2, 1), (4, 3, 0, 2), (4, 3, 1, 2), (3, 2, 0, 2),
                             (8, 4, 3, 1), (16, 4, 2, 2)):
        rows = np.asarray(tiling.tile_rows(H, rb, P, part, run), dtype=np.int64)
        empty += len(rows) == 0
        got = host(r.render_mesh_aovs(scene, row_block=rb, n_parts=P, part=part, part_run=run))
        tile = {k: np.ascontiguousarray(v[..., rows, :].reshape(v.shape[:-2] + (len(rows) * W,))) for k, v in shaped.items()}
        same(got, tile, what=(rb, P, part, run))
    assert empty == 2
    r._lib = calls = _Calls(r._lib)
    got = r.render_mesh_aovs(scene, row_block=8, n_parts=4, part=3)  # an empty tile launches nothing
    assert calls.names == [] and tuple(got["position"].shape) == (3, 0) and tuple(got["lit"].shape) == (0,)


def test_a_pinhole_perspective_camera_and_a_lens(hip):
    view = dict(position=[2.5, 1.5, -1.5], target=[0, 0.0, 2.0], fov=50.0)
    spec = scenes.with_camera(scenes.mesh_spec(37, 23, 1), **view)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    origins, dirs = r.camera_rays(scene.camera)
    assert origins is None
    eye = tuple(float(c) for c in spec["camera"]["position"])
    want = A.of_spec(spec, eye, tuple(dirs.cpu().numpy()))
    assert int((want["triangle"] >= 0).sum()) > 100 and int((want["id"] == 0).sum()) > 20
    got = host(r.render_mesh_aovs(scene))
    same(got, want, what="pinhole")
    same(host(r.trace_mesh_aovs(scene.camera.position, dirs, scene)), got, what="trace_mesh_aovs on camera_rays")
    rows = tiling.tile_rows(23, 2, 3, 1)
    tile = host(r.render_mesh_aovs(scene, row_block=2, n_parts=3, part=1, passes=("depth", "triangle")))
    assert np.array_equal(tile["depth"], got["depth"].reshape(23, 37)[rows].reshape(-1))
    assert np.array_equal(tile["triangle"], got["triangle"].reshape(23, 37)[rows].reshape(-1))
    lens = scenes.build_scene(scenes.with_camera(scenes.mesh_spec(19, 11, 1), **view, lens_radius=0.05, focus_distance=3.0))
    with pytest.raises(ValueError, match="lens_radius=0.05"):
        r.render_mesh_aovs(lens)


@pytest.mark.parametrize("key", ["mesh", "textured"])
def test_the_table_variants_change_no_bit(hip, key):
    spec, want = frame(key)
    scene = scenes.build_scene(spec)
    for leaf, build in ((4, "host"), (1, "host"), (None, "host"), (4, "device"), (1, "device")):
        r = hip.HipRenderer(3)
        r.mesh_max_leaf, r.mesh_build = leaf, build
        r._lib = calls = _Calls(r._lib)
        same(host(r.render_mesh_aovs(scene)), want, what=(key, leaf, build))
        assert ("rtx_mesh_build" in calls.names) == (build == "device")


def test_a_deep_tree_with_incoherent_rays(hip):
    spec, o, d, want = deep_rays()
    scene = scenes.build_scene(spec)
    got = host(hip.HipRenderer(1).trace_mesh_aovs(_vec(hip, o), _vec(hip, d), scene))
    same(got, want, what="level 5, 512 incoherent rays")


def test_the_passes_agree_with_the_colour_path(hip):
    spec, want = frame("mesh")
    scene = scenes.build_scene(spec)
    colour = hip.HipRenderer(0).render(scene).data.cpu().numpy()
    ids = hip.HipRenderer(0).render_mesh_aovs(scene, passes="id")["id"].cpu().numpy()
    hit = ids >= 0
    assert np.array_equal(hit, (colour != 0).any(axis=0))  # a miss is black ...
    assert not colour[:, ~hit].any() and colour[:, hit].max(axis=0).min() >= 0.004  # ... and a hit has the ambient term


# ---- the op and the C entry -----------------------------------------------------------------------------------

def _op_args(r, scene, spec):
    import python_ray_tracer_amd.ops  # noqa: F401

    blob, S = r.scene_blob(scene)
    mesh = torch.tensor(meshes.mesh_table(scene.shapes)).cuda()
    table = torch.from_numpy(R.table_of(spec)).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    return blob, S, mesh, table, eye, dirs


def test_the_op_against_the_method(hip):
    scene, spec, ids = interleaved_scene()
    r = hip.HipRenderer(3)
    full = r.render_mesh_aovs(scene)
    blob, S, mesh, table, eye, dirs = _op_args(r, scene, spec)
    dev_ids = torch.from_numpy(ids).cuda()
    out = torch.ops.rt.mesh_aovs(blob, S, mesh, table, dev_ids, eye, dirs, L.MESH_AOV_ALL)
    assert len(out) == 10 and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(out, full.values()))
    per_ray = eye.unsqueeze(1).expand(3, W * H).contiguous()
    depth, lit = torch.ops.rt.mesh_aovs(blob, S, mesh, table, dev_ids, per_ray, dirs, 1 | 128, check=False)
    assert torch.equal(depth, full["depth"]) and torch.equal(lit, full["lit"])
    # no shape_ids: the spheres' numbers, then the meshes'
    ident, = torch.ops.rt.mesh_aovs(blob, S, mesh, table, None, eye, dirs, 2)
    assert np.array_equal(ident.cpu().numpy(), frame("mesh")[1]["id"])
    empty = torch.ops.rt.mesh_aovs(blob, S, mesh, table, None, eye, dirs[:, :0].contiguous(), 8 | 512)
    assert [tuple(t.shape) for t in empty] == [(3, 0), (2, 0)]
    with pytest.raises(RuntimeError, match="shape_ids must have one entry"):
        torch.ops.rt.mesh_aovs(blob, S, mesh, table, dev_ids[:4].contiguous(), eye, dirs, 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.mesh_aovs(blob, S, mesh.cpu(), table, None, eye, dirs, 2)
    # a table whose header does not fit its length: refused on the host with check=True; with check=False the
    # kernel reads it as a table without triangles, and the passes are the spheres' alone
    short = mesh[:-1].contiguous()
    with pytest.raises(RuntimeError, match="mesh table"):
        torch.ops.rt.mesh_aovs(blob, S, short, table, None, eye, dirs, 2)
    got = torch.ops.rt.mesh_aovs(blob, S, short, table, None, eye, dirs, 1 | 2 | 4 | 8 | 16 | 256, check=False)
    plain = copy.deepcopy(spec)
    plain.pop("meshes")
    osc = O.scene_from_spec(plain)
    want = aov_ref.aovs(osc, *aov_ref.frame_rays(osc))
    for t, k in zip(got[:5], ("depth", "id", "hits", "position", "normal")):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    assert (got[5] == -1).all()


def test_the_c_entry_refuses_bad_arguments(hip):
    lib = L.load()
    call, bad = bad_argument_calls(lib)
    for kw, word in bad:
        assert call(**kw) == -1 and word in lib.rtx_last_error(), kw
    assert call(n=0) == 0
    with pytest.raises(L.RtxError, match="no pass requested"):
        L.check(call(outs=[None] * 10), "rtx_mesh_aovs")


def test_render_aovs_of_a_scene_without_a_mesh_is_what_it_was(hip):
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    first = hip.HipRenderer(3).render_aovs(plain)
    r = hip.HipRenderer(3)
    r.render_mesh_aovs(scenes.build_scene(frame("mesh")[0]), passes="depth")
    second = r.render_aovs(plain)
    assert tuple(first) == tuple(second) == hip.AOV_NAMES
    assert all(torch.equal(first[k], second[k]) for k in first)
    osc = O.scene_from_spec(scenes.readme_spec(W, H))
    want = aov_ref.aovs(osc, *aov_ref.frame_rays(osc))
    assert all(np.array_equal(first[k].cpu().numpy(), want[k]) for k in aov_ref.PASSES)
