"""Image textures on meshes on the GPU: scenes with an ImageTexture on a TriangleMesh through HipRenderer and
rt::trace_mesh_uv.

Every render is compared with the NumPy restatement (tests/meshuv_ref.py: tests/mesh_ref.py with the image
lookup of include/rtx_hip.h, operation for operation, every triangle tried for every ray) at the project's
bar for float64 colour, |GPU - restatement| <= 1e-12 * max(1, |colour|), and its uint8 frame must be
identical, no pixel excluded: tests/test_meshuv_cpu.py checks that no pixel of a case sits within 1e-9 of a
quantisation step, that each frame exercises what it is meant to (wrapped and negative coordinates, the
torus's seam segment, reflected hits on textured triangles), and that the tree's pruning changes no frame of
the restatement. Nothing here provokes an overflow of a lane's stack: the stack filled to its last entry and one
over, and a worker's second item, through this kernel too, are in tests/test_gpu_mesh_limits.py.
"""

import copy

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes, scenes, tiling
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import meshuv_ref as U
from tests import ssaa_ref
from tests.test_lights_cpu import step_distance
from tests.test_mesh_cpu import CAPS, H, W, shader
from tests.test_mesh_cpu import frame as plain_frame
from tests.test_meshuv_cpu import ONE, exact_cases, frame, image, image_shader, quad_1x1

pytestmark = pytest.mark.gpu

RTOL = 1e-12
TRACE_ENTRIES = ("rtx_trace_mesh", "rtx_trace_mesh_uv", "rtx_trace_lights", "rtx_trace_rays", "rtx_trace_glass",
                 "rtx_trace_lights_env", "rtx_trace_glass_env")


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


def _only_the_uv_entry(names):
    """Once through rtx_trace_mesh_uv and through no other trace entry or camera launch."""
    traced = [n for n in names if n in TRACE_ENTRIES or n.startswith("rtx_render_camera")]
    return traced == ["rtx_trace_mesh_uv"]


# ---- frames against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", ["quad_3x5", "quad_wrap", "torus_mirror", "mixed"])
def test_frames_against_the_restatement(hip, key, cap):
    spec, want, c = frame(key, cap)
    assert c.tex_primary > 0
    got, names = _render(hip, spec, cap)
    assert _only_the_uv_entry(names), names
    _check(got, want, W, H, f"{key} B={cap}")


@pytest.mark.parametrize("cap", CAPS)
def test_a_1x1_image_is_its_colour(hip, cap):
    """Against the restatement, and within the bar of the same mesh in that constant colour through the old
    kernel (the lookup's four equal texels: (c*gx + c*fx)*gy + (c*gx + c*fx)*fy rounds, the constant does not)."""
    spec, want, _ = frame("quad_1x1", cap)
    got, names = _render(hip, spec, cap)
    assert _only_the_uv_entry(names), names
    _check(got, want, W, H, f"1x1 image B={cap}")
    const, names = _render(hip, quad_1x1(False), cap)
    assert names.count("rtx_trace_mesh") == 1 and "rtx_trace_mesh_uv" not in names
    _check(got, const, W, H, f"1x1 image against the constant {ONE} B={cap}")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", ["1x1", "7x5", "67x5"])
def test_frames_that_end_inside_a_wave(hip, key, cap):
    spec, want, _ = frame(key, cap)
    got, names = _render(hip, spec, cap)
    assert _only_the_uv_entry(names), names
    _check(got, want, spec["camera"]["width"], spec["camera"]["height"], f"{key} B={cap}")


# ---- explicit rays: exact cases ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(exact_cases()))
def test_exact_rays(hip, name):
    """Rays built from small dyadic numbers (tests/test_meshuv_cpu.py checks that the restatement shades each
    with the colour named there): a hit at a texel centre takes that texel, one on the boundary between texels
    their mean, and a ray through the edge two triangles with different uvs share the lower-numbered one's."""
    spec, o, d, colours = exact_cases()[name]
    want = U.trace_rays(spec, tuple(o), tuple(d), 3)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    r._lib = calls = _Calls(r._lib)
    od, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    got = r.raytrace_scene(hip.HipVector3D(od[0], od[1], od[2]), hip.HipVector3D(dd[0], dd[1], dd[2]), scene)
    got = got.data.cpu().numpy()
    assert _only_the_uv_entry(calls.names), calls.names
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"{name}: max err {err:.3e}, colours {got.T.tolist()}")
    assert got.shape == (3, len(colours)) and err <= RTOL and (got > 0.004).all()


# ---- invariances, bit for bit between GPU renders -------------------------------------------------------------

def _as_triangles(spec, order=None, split=None):
    """``spec`` with its last mesh as explicit triangles with their uvs, its faces in ``order``, or cut into two
    meshes that share the shader (and so the image) after ``split`` faces."""
    m = spec["meshes"][-1]
    mesh = scenes.mesh_of(m)
    f, uv = mesh.faces, mesh.uvs
    if order is not None:
        f, uv = f[order], uv[order]
    out = copy.deepcopy(spec)
    cuts = [slice(None)] if split is None else [slice(0, split), slice(split, None)]
    out["meshes"] = out["meshes"][:-1] + [
        {"kind": "triangles", "vertices": mesh.vertices.tolist(), "faces": f[c].tolist(), "uvs": uv[c].tolist(),
         "normals": mesh.normals.tolist(), "shader": copy.deepcopy(m["shader"])} for c in cuts]
    return out


def test_the_leaf_size_changes_no_bit(hip):
    for key in ("torus_mirror", "mixed"):
        spec, want, _ = frame(key)
        base, _ = _render(hip, spec, 3)
        _check(base, want, W, H, key)
        for leaf in (1, 2, 8, None):
            got, names = _render(hip, spec, 3, max_leaf=leaf)
            assert _only_the_uv_entry(names) and np.array_equal(got, base), (key, leaf)


def test_permuted_faces_and_a_split_mesh_change_no_bit(hip):
    """A frame without two triangles at one distance (tri_ties == 0 in the restatement): the numbering of the
    faces, moved together with their uvs, and their distribution over two meshes that share the image change
    nothing. A UV part that did not follow the rows' leaf order would."""
    spec, want, c = frame("torus_mirror")
    assert c.tri_ties == 0 and c.tex_primary > 20
    base, _ = _render(hip, _as_triangles(spec), 3)
    _check(base, want, W, H, "torus as triangles")
    order = np.random.default_rng(7).permutation(2 * 16 * 8)
    got, names = _render(hip, _as_triangles(spec, order=order), 3)
    assert _only_the_uv_entry(names) and np.array_equal(got, base)
    two_spec = _as_triangles(spec, split=101)
    table = meshes.mesh_table(scenes.build_scene(two_spec).shapes)
    assert table[meshes.MH_NMESH] == 2 and table.size == table[meshes.MH_TEXELS] + 4 * 4 * 3  # one block for both
    two, names = _render(hip, two_spec, 3)
    assert _only_the_uv_entry(names) and np.array_equal(two, base)


# ---- paths ----------------------------------------------------------------------------------------------------

def test_tiles_runs_u8_into_and_float32(hip):
    spec, want, _ = frame("mixed")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    full = r.render(scene).data.cpu().numpy()
    _check(full, want, W, H, "mixed")
    full_u8 = r.render_tile(scene, out="u8")
    assert full_u8.dtype == torch.uint8 and tuple(full_u8.shape) == (H, W, 3)
    full_u8 = full_u8.cpu().numpy()
    assert np.array_equal(full_u8, O.to_uint8(want, W, H))
    full = full.reshape(3, H, W)
    rb, P = 4, 3
    for part in range(P):
        rows = tiling.tile_rows(H, rb, P, part)
        tile = r.render_tile(scene, rb, P, part).cpu().numpy()
        assert np.array_equal(tile, full[:, rows].reshape(3, -1)), part
        assert np.array_equal(r.render_tile(scene, rb, P, part, out="u8").cpu().numpy(), full_u8[rows]), part
    for part, run in ((0, 2), (1, 2)):  # runs of parts as one tile
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


def _small_textured(w, h):
    return scenes.textured_mesh_spec(w, h, 1, scenes.uv_grid_texels(8, 8))


def test_supersampled_frame(hip):
    spec = _small_textured(24, 13)
    sample = U.render(ssaa_ref.spec_at(spec, 2), 3)
    want = ssaa_ref.resolve_ref(sample, 2, 24, 13)
    assert step_distance(want) > 1e-9
    r = hip.HipRenderer(3, samples=2)
    r._lib = calls = _Calls(r._lib)
    got = r.render(scenes.build_scene(spec)).data.cpu().numpy()
    assert _only_the_uv_entry(calls.names) and "rtx_resolve_samples" in calls.names
    _check(got, want, 24, 13, "samples=2")


def test_perspective_camera_pinhole_and_lens(hip):
    view = dict(position=[2.5, 1.5, -1.5], target=[0, 0.0, 2.0], fov=50.0)
    spec = scenes.with_camera(_small_textured(37, 23), **view)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    origins, dirs = r.camera_rays(scene.camera)  # (tests/test_gpu_camera.py pins them to the restatement)
    assert origins is None
    eye = tuple(float(c) for c in spec["camera"]["position"])
    counts = U.Counts()
    want = U.trace_rays(spec, eye, tuple(dirs.cpu().numpy()), 3, counts)
    assert step_distance(want) > 1e-9 and counts.tex_primary > 0
    r._lib = calls = _Calls(r._lib)
    got = r.render(scene).data.cpu().numpy()
    assert _only_the_uv_entry(calls.names)
    _check(got, want, 37, 23, "pinhole")
    # a lens at samples=2: per-ray origins
    lens = scenes.with_camera(_small_textured(19, 11), **view, lens_radius=0.05, focus_distance=3.0)
    scene = scenes.build_scene(lens)
    r = hip.HipRenderer(3, samples=2)
    origins, dirs = r.camera_rays(scene.camera)
    assert tuple(origins.shape) == (3, 4 * 19 * 11)
    sample = U.trace_rays(lens, tuple(origins.cpu().numpy()), tuple(dirs.cpu().numpy()), 3)
    want = ssaa_ref.resolve_ref(sample, 2, 19, 11)
    assert step_distance(want) > 1e-9
    _check(r.render(scene).data.cpu().numpy(), want, 19, 11, "lens, samples=2")


def test_render_image_pipeline_writes_the_png_of_the_restatement(hip, tmp_path):
    from PIL import Image

    from python_ray_tracer_amd.application import render_image_pipeline

    spec, want, _ = frame("mixed")
    out = tmp_path / "meshuv.png"
    render_image_pipeline(scenes.build_scene(spec), out, hip.HipRenderer(3))
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), O.to_uint8(want, W, H))


def test_op_against_the_ctypes_route_and_a_table_whose_new_offsets_do_not_fit(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    spec, want, _ = frame("quad_3x5")
    cap = 3
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S = r.scene_blob(scene)
    assert S == 2
    host = meshes.mesh_table(scene.shapes)
    mesh = torch.tensor(host).cuda()
    table = torch.tensor([[float(c) for c in spec["lights"][0]["position"]] + [1.0, 1.0, 1.0]], dtype=torch.float64).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    trace = torch.ops.rt.trace_mesh_uv
    assert torch.equal(trace(blob, S, mesh, table, eye, dirs, cap, 1), full)
    assert torch.equal(trace(blob, S, mesh, table, eye.unsqueeze(1).expand(3, W * H).contiguous(), dirs, cap, 0),
                       full.to(torch.float32))
    u8 = trace(blob, S, mesh, table, eye, dirs, cap, 2, check=False)
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), O.to_uint8(want, W, H))
    assert tuple(trace(blob, S, mesh, table, eye, dirs[:, :0].contiguous(), cap, 1).shape) == (3, 0)
    with pytest.raises(RuntimeError, match="max_bounces"):
        trace(blob, S, mesh, table, eye, dirs, 17, 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        trace(blob, S, mesh.cpu(), table, eye, dirs, cap, 1)
    # new offsets that do not fit the table: refused on the host with check=True; with check=False the kernel
    # reads "no image" and the textured mesh's texture colour is black, as on the same mesh in constant black
    black = copy.deepcopy(spec)
    black["meshes"][0]["shader"] = shader((0.0, 0.0, 0.0))
    want_black = U.render(black, cap)
    mats_at = int(host[meshes.MH_MATS])
    for word, value in ((meshes.MH_UVS, float(host.size - 5)), (meshes.MH_TEXELS, float(host.size + 1)),
                        (mats_at + L.M_TR, float(host.size - 44)), (mats_at + L.M_TG, 4.0)):
        bad = host.copy()
        bad[word] = value
        with pytest.raises(ValueError, match="mesh table"):
            meshes.check_table(bad)
        dev = torch.tensor(bad).cuda()
        if word in (meshes.MH_UVS, meshes.MH_TEXELS):
            with pytest.raises(RuntimeError, match="mesh table"):
                trace(blob, S, dev, table, eye, dirs, cap, 1)
        got = trace(blob, S, dev, table, eye, dirs, cap, 1, check=False).cpu().numpy()
        _check(got, want_black, W, H, f"word {word} = {value}: no image")


# ---- untextured scenes and the memo ---------------------------------------------------------------------------

def test_an_untextured_mesh_scene_keeps_the_old_entry(hip):
    spec, want, _ = plain_frame("readme_mesh")
    with_uv = copy.deepcopy(spec)
    with_uv["meshes"][0]["uv"] = True  # coordinates without an image change nothing
    for s in (spec, with_uv):
        got, names = _render(hip, s, 3)
        assert names.count("rtx_trace_mesh") == 1 and "rtx_trace_mesh_uv" not in names
        _check(got, want, W, H, "readme_mesh")


def test_a_second_render_reads_no_status_word_back(hip):
    spec, _, _ = frame("quad_3x5")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    reads = []
    read = r._read_status
    r._read_status = lambda ws: (reads.append(1), read(ws))[1]
    a = r.render(scene).data.cpu().numpy()
    assert len(reads) == 1
    b = r.render(scenes.build_scene(spec)).data.cpu().numpy()  # the same content in new objects
    assert len(reads) == 1 and np.array_equal(a, b) and len(r._mesh_tables) == 1  # one upload per content
    other = copy.deepcopy(spec)
    other["meshes"][0]["shader"] = image_shader(image(3, 5)[::-1])  # another image: another table, another render
    c = r.render(scenes.build_scene(other)).data.cpu().numpy()
    assert len(reads) == 2 and len(r._mesh_tables) == 2 and not np.array_equal(a, c)
