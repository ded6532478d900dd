"""Triangle meshes on the GPU: mesh scenes through HipRenderer and rt::trace_mesh.

Every render is compared with the NumPy restatement (tests/mesh_ref.py, every triangle tried for every ray)
at the project's bar for float64 colour, |GPU - restatement| <= 1e-12 * max(1, |colour|), and its uint8
frame must be identical, no pixel excluded: tests/test_mesh_cpu.py checks that no pixel of a case sits
within 1e-9 of a quantisation step, that each frame exercises what it is meant to, and that the tree's
pruning changes no frame of the restatement. Which rays exist, which triangle they hit and which light
reaches a hit are decisions the kernel must take bit for bit like the restatement; a wrong one moves a
pixel by far more than the bar. Nothing here provokes an overflow of a lane's stack: the stack filled to
its last entry and one over, a worker's second item and the far, deep and grazing cases are in
tests/test_gpu_mesh_limits.py.
"""

import copy

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import lights, meshes, scenes, tiling
from tests import mesh_ref as R
from tests import ssaa_ref
from tests.test_lights_cpu import step_distance
from tests.test_mesh_cpu import CAPS, CASES, H, W, exact_cases, frame, ico_spec, shader

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _check(got, want, w, h, what=""):
    """float64 colour within the bar of the restatement's, and the same uint8 frame."""
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"{what}: max |gpu - ref| / max(1, |ref|) = {err:.3e} (colours up to {want.max():.3f})")
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert err <= RTOL, (what, err)
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


def _render(hip, spec, cap, max_leaf=4, **kw):
    r = hip.HipRenderer(cap, **kw)
    r.mesh_max_leaf = max_leaf
    r._lib = calls = _Calls(r._lib)
    return r.render(scenes.build_scene(spec)).data.cpu().numpy(), calls.names


def _only_the_mesh_entry(names):
    return names.count("rtx_trace_mesh") == 1 and not any(
        n.startswith("rtx_render_camera") or n in ("rtx_trace_lights", "rtx_trace_rays") for n in names)


FRAMES = ["quad", "ico1_flat", "ico1_smooth", "ico2_flat", "ico2_smooth", "torus", "mesh_only", "two_lights", "tree17",
          "readme_mesh"]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", FRAMES)
def test_frames_against_the_restatement(hip, key, cap):
    spec, want, c = frame(key, cap)
    assert c.tri_primary > 0
    got, names = _render(hip, spec, cap)
    assert _only_the_mesh_entry(names), names
    _check(got, want, W, H, f"{key} B={cap}")


def test_the_mesh_changes_the_frame_and_a_plain_scene_keeps_its_path(hip):
    """The frame is not the spheres' alone, and the scene without its meshes takes the camera launch."""
    spec, want, _ = frame("ico2_smooth")
    plain = copy.deepcopy(spec)
    plain.pop("meshes")
    got, names = _render(hip, plain, 3)
    assert "rtx_trace_mesh" not in names and any(n.startswith("rtx_render_camera") for n in names)
    assert int((O.to_uint8(got, W, H) != O.to_uint8(want, W, H)).any(axis=-1).sum()) > 20


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", ["1x1", "7x5", "67x5"])
def test_frames_that_end_inside_a_wave(hip, key, cap):
    spec, want, _ = frame(key, cap)
    got, names = _render(hip, spec, cap)
    assert _only_the_mesh_entry(names)
    _check(got, want, spec["camera"]["width"], spec["camera"]["height"], f"{key} B={cap}")


# ---- explicit rays: exact cases ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(exact_cases()))
def test_exact_rays(hip, name):
    """Rays built from small dyadic numbers (tests/test_mesh_cpu.py checks what the restatement makes of
    them): a shared edge and a shared vertex shade once, a ray in a triangle's plane or starting on it and a
    triangle beyond FARAWAY are misses, a sphere and a triangle at the same distance both shade."""
    spec, o, d, _ = exact_cases()[name]
    want = R.trace_rays(spec, tuple(o), tuple(d), 3)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    r._lib = calls = _Calls(r._lib)
    od, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    got = r.raytrace_scene(hip.HipVector3D(od[0], od[1], od[2]), hip.HipVector3D(dd[0], dd[1], dd[2]), scene)
    got = got.data.cpu().numpy()
    assert calls.names.count("rtx_trace_mesh") == 1
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"{name}: max err {err:.3e}, colours {got.T.tolist()}")
    assert err <= RTOL and np.array_equal(got == 0, want == 0)
    if name == "in_plane_and_on_it":
        assert not got[:, :3].any() and got[:, 3].all()
    if name == "faraway":
        assert not got.any()
    if name == "tie":  # both shade: the sum of the sphere's colour and the triangle's, each with the other in the scene
        c = R.Counts()
        R.trace_rays(spec, tuple(o), tuple(d), 3, c)
        assert c.ties == 1 and (got >= 2 * 0.004).all()


# ---- invariances, bit for bit between GPU renders -------------------------------------------------------------

@pytest.mark.parametrize("key", ["ico2_smooth", "readme_mesh"])
def test_the_leaf_size_changes_no_bit(hip, key):
    spec, want, _ = frame(key)
    base, _ = _render(hip, spec, 3)
    _check(base, want, W, H, key)
    for leaf in (1, 2, 8, None):
        got, names = _render(hip, spec, 3, max_leaf=leaf)
        assert _only_the_mesh_entry(names) and np.array_equal(got, base), leaf


def _as_triangles(spec, order=None, split=None):
    """``spec`` with its one mesh as explicit triangles, its faces in ``order``, or cut into two meshes of
    equal shaders after ``split`` faces."""
    m = spec["meshes"][0]
    v, f, n = scenes.mesh_arrays(m)
    f = f if order is None else f[order]
    out = copy.deepcopy(spec)
    parts = [f] if split is None else [f[:split], f[split:]]
    out["meshes"] = [{"kind": "triangles", "vertices": v.tolist(), "faces": p.tolist(), "shader": copy.deepcopy(m["shader"]),
                      **({} if n is None else {"normals": n.tolist()})} for p in parts]
    return out


def test_permuted_faces_and_a_split_mesh_change_no_bit(hip):
    """A frame without two triangles at one distance (tri_ties == 0 in the restatement): the numbering of the
    faces and their distribution over meshes of equal shaders change nothing."""
    for key in ("ico2_flat", "ico2_smooth"):
        spec, want, c = frame(key)
        assert c.tri_ties == 0 and c.tri_primary > 20
        base, _ = _render(hip, _as_triangles(spec), 3)
        _check(base, want, W, H, key)
        order = np.random.default_rng(7).permutation(320)
        got, _ = _render(hip, _as_triangles(spec, order=order), 3)
        assert np.array_equal(got, base), key
        two, names = _render(hip, _as_triangles(spec, split=123), 3)
        assert _only_the_mesh_entry(names) and np.array_equal(two, base), key
    # two coincident meshes do not add: the group shades one triangle per ray
    spec, want, _ = frame("ico2_flat")
    twice = _as_triangles(spec)
    twice["meshes"].append(copy.deepcopy(twice["meshes"][0]))
    got, _ = _render(hip, twice, 3)
    assert np.array_equal(got, _render(hip, _as_triangles(spec), 3)[0])


# ---- surfaces -------------------------------------------------------------------------------------------------

def test_tiles_runs_u8_into_and_float32(hip):
    spec, want, _ = frame("readme_mesh")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    full = r.render(scene).data.cpu().numpy()
    _check(full, want, W, H, "readme_mesh")
    full_u8 = r.render_tile(scene, out="u8")
    assert full_u8.dtype == torch.uint8 and tuple(full_u8.shape) == (H, W, 3)
    full_u8 = full_u8.cpu().numpy()
    assert np.array_equal(full_u8, O.to_uint8(want, W, H))
    full = full.reshape(3, H, W)
    rb, P = 4, 3
    seen = np.zeros(H, dtype=int)
    for part in range(P):
        rows = tiling.tile_rows(H, rb, P, part)
        seen[rows] += 1
        tile = r.render_tile(scene, rb, P, part).cpu().numpy()
        assert np.array_equal(tile, full[:, rows].reshape(3, -1)), part
        assert np.array_equal(r.render_tile(scene, rb, P, part, out="u8").cpu().numpy(), full_u8[rows]), part
    assert (seen == 1).all()
    for part, run in ((0, 2), (1, 2), (0, 3)):  # runs of parts as one tile
        rows = tiling.tile_rows(H, rb, P, part, run)
        tile = r.render_tile(scene, rb, P, part, part_run=run).cpu().numpy()
        assert np.array_equal(tile, full[:, rows].reshape(3, -1)), (part, run)
    into = torch.zeros((3, W * H), dtype=torch.float64, device="cuda")
    assert r.render_tile(scene, into=into) is into
    assert np.array_equal(into.cpu().numpy(), full.reshape(3, -1))
    r32 = hip.HipRenderer(3, color_dtype=torch.float32)
    got32 = r32.render(scene).data
    assert got32.dtype == torch.float32
    assert np.array_equal(got32.cpu().numpy(), full.reshape(3, -1).astype(np.float32))  # the float64 value rounded once


def test_supersampled_frame(hip):
    """samples=2: the sample frame traced by the mesh kernel, resolved as for every other scene."""
    spec = scenes.mesh_spec(24, 13, 1)
    sample = R.render(ssaa_ref.spec_at(spec, 2), 3)
    want = ssaa_ref.resolve_ref(sample, 2, 24, 13)
    assert step_distance(want) > 1e-9
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3, samples=2)
    r._lib = calls = _Calls(r._lib)
    got = r.render(scene).data.cpu().numpy()
    assert _only_the_mesh_entry(calls.names) and "rtx_resolve_samples" in calls.names
    _check(got, want, 24, 13, "samples=2")
    rows = tiling.tile_rows(13, 2, 2, 1)
    tile = r.render_tile(scene, 2, 2, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 13, 24)[:, rows].reshape(3, -1))
    assert np.array_equal(r.render_tile(scene, out="u8").cpu().numpy(), ssaa_ref.to_u8(got, 24, 13))


def test_perspective_camera_pinhole_and_lens(hip):
    view = dict(position=[2.5, 1.5, -1.5], target=[0, 0.0, 2.0], fov=50.0)
    spec = scenes.with_camera(scenes.mesh_spec(37, 23, 1), **view)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    origins, dirs = r.camera_rays(scene.camera)  # (tests/test_gpu_camera.py pins them to the restatement)
    assert origins is None
    eye = tuple(float(c) for c in spec["camera"]["position"])
    want = R.trace_rays(spec, eye, tuple(dirs.cpu().numpy()), 3)
    assert step_distance(want) > 1e-9
    r._lib = calls = _Calls(r._lib)
    got = r.render(scene).data.cpu().numpy()
    assert _only_the_mesh_entry(calls.names)
    _check(got, want, 37, 23, "pinhole")
    rows = tiling.tile_rows(23, 2, 3, 1)
    tile = r.render_tile(scene, 2, 3, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 23, 37)[:, rows].reshape(3, -1))
    # a lens at samples=2: per-ray origins
    lens = scenes.with_camera(scenes.mesh_spec(19, 11, 1), **view, lens_radius=0.05, focus_distance=3.0)
    scene = scenes.build_scene(lens)
    r = hip.HipRenderer(3, samples=2)
    origins, dirs = r.camera_rays(scene.camera)
    assert tuple(origins.shape) == (3, 4 * 19 * 11)
    sample = R.trace_rays(lens, tuple(origins.cpu().numpy()), tuple(dirs.cpu().numpy()), 3)
    want = ssaa_ref.resolve_ref(sample, 2, 19, 11)
    assert step_distance(want) > 1e-9
    _check(r.render(scene).data.cpu().numpy(), want, 19, 11, "lens, samples=2")


def test_render_image_pipeline_writes_the_png_of_the_restatement(hip, tmp_path):
    from PIL import Image

    from python_ray_tracer_amd.application import render_image_pipeline

    spec, want, _ = frame("readme_mesh")
    out = tmp_path / "mesh.png"
    render_image_pipeline(scenes.build_scene(spec), out, hip.HipRenderer(3))
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), O.to_uint8(want, W, H))


def test_op_against_the_ctypes_route(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    spec, want, _ = frame("readme_mesh")
    cap = 3
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S = r.scene_blob(scene)
    assert S == 2
    mesh = torch.tensor(meshes.mesh_table(scene.shapes)).cuda()
    table = torch.tensor([[float(c) for c in spec["lights"][0]["position"]] + [1.0, 1.0, 1.0]], dtype=torch.float64).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    out = torch.ops.rt.trace_mesh(blob, S, mesh, table, eye, dirs, cap, 1)
    assert torch.equal(out, full)
    out32 = torch.ops.rt.trace_mesh(blob, S, mesh, table, eye.unsqueeze(1).expand(3, W * H).contiguous(), dirs, cap, 0)
    assert torch.equal(out32, full.to(torch.float32))
    u8 = torch.ops.rt.trace_mesh(blob, S, mesh, table, eye, dirs, cap, 2, check=False)
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), O.to_uint8(want, W, H))
    empty = torch.ops.rt.trace_mesh(blob, S, mesh, table, eye, dirs[:, :0].contiguous(), cap, 1)
    assert tuple(empty.shape) == (3, 0)
    with pytest.raises(RuntimeError, match="max_bounces"):
        torch.ops.rt.trace_mesh(blob, S, mesh, table, eye, dirs, 17, 1)
    with pytest.raises(RuntimeError, match="mesh must be"):
        torch.ops.rt.trace_mesh(blob, S, mesh[:8].contiguous(), table, eye, dirs, cap, 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_mesh(blob, S, mesh.cpu(), table, eye, dirs, cap, 1)
    # a table whose header does not fit its length: refused on the host with check=True; with check=False the
    # kernel reads it as a table without triangles, and the frame is the spheres' alone
    short = mesh[:-1].contiguous()
    with pytest.raises(RuntimeError, match="mesh table"):
        torch.ops.rt.trace_mesh(blob, S, short, table, eye, dirs, cap, 1)
    spheres = torch.ops.rt.trace_mesh(blob, S, short, table, eye, dirs, cap, 1, check=False)
    plain = copy.deepcopy(spec)
    plain.pop("meshes")
    assert np.abs(spheres.cpu().numpy() - O.render(O.scene_from_spec(plain), cap)).max() <= RTOL * 4  # (colours up to about 4)


def test_a_second_render_reads_no_status_word_back(hip):
    """The clean-render memo: the kernel is deterministic, so a render whose status came back clean is not
    read back again; another scene, tile or cap is."""
    spec, _, _ = frame("quad")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    reads = []
    read = r._read_status
    r._read_status = lambda ws: (reads.append(1), read(ws))[1]
    a = r.render(scene).data.cpu().numpy()
    assert len(reads) == 1
    b = r.render(scenes.build_scene(spec)).data.cpu().numpy()  # the same content in new objects
    assert len(reads) == 1 and np.array_equal(a, b)
    r.render_tile(scene, 4, 3, 1)
    assert len(reads) == 2
    r.render(scenes.build_scene(ico_spec(1, True)))
    assert len(reads) == 3
    assert len(r._mesh_tables) == 2  # one upload per content


def test_one_renderer_renders_meshes_lights_and_plain_scenes_in_turn(hip):
    r = hip.HipRenderer(3)
    for key in ("two_lights", "quad", "two_lights"):
        spec, want, _ = frame(key)
        _check(r.render(scenes.build_scene(spec)).data.cpu().numpy(), want, W, H, key)
    plain = scenes.readme_spec(W, H)
    got = r.render(scenes.build_scene(plain)).data.cpu().numpy()
    _check(got, O.render(O.scene_from_spec(plain), 3), W, H, "plain")
    assert lights.lights_table(scenes.build_scene(CASES["two_lights"]()).lights).shape == (3, 6)
    assert shader()["texture"]["kind"] == "const"
