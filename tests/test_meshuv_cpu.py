"""Texture coordinates and image textures on meshes without a GPU: OBJ ``vt``, the generators' coordinates,
the table's UV part and texel blocks, the refusals, the NumPy restatement (tests/meshuv_ref.py) and the
preconditions of every frame tests/test_gpu_meshuv.py renders."""

import copy
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import mesh_ref as R
from tests import meshuv_ref as U
from tests.test_lights_cpu import step_distance
from tests.test_mesh_cpu import CAPS, CASES, GAINS, H, REPO, W, exact_spec, shader
from tests.test_mesh_cpu import frame as plain_frame

QUAD = [[-4, -0.5, -1], [-4, -0.5, 7], [4, -0.5, 7], [4, -0.5, -1]]  # a floor that fills most of the frame


def image(w, h):
    """``w`` x ``h`` texels (an array [h, w, 3]) of w * h distinct colours."""
    k = np.arange(w * h, dtype=np.float64).reshape(h, w)
    n = float(w * h)
    return np.stack([(k + 1.0) / (n + 1.0), ((7.0 * k) % n + 1.0) / (n + 1.0), ((11.0 * k) % n + 1.0) / (n + 1.0)], axis=-1)


def image_shader(texels, gains=GAINS):
    return scenes._shader(*gains, {"kind": "image", "texels": np.asarray(texels, dtype=np.float64)})


def quad_3x5():
    """Case 1: the README scene's two spheres over a quad with uvs 0..1 under a 3 x 5 image."""
    spec = scenes.readme_spec(W, H)
    spec["spheres"].pop(2)
    spec["meshes"] = [{"kind": "quad", "corners": QUAD, "uv": True, "shader": image_shader(image(3, 5))}]
    return spec


def quad_wrap():
    """Case 2: the same quad with uvs from -1.5 to 2.5 under a 2 x 2 image: four repeats on each axis."""
    spec = quad_3x5()
    lo, hi = -1.5, 2.5
    st = [[lo, lo], [hi, lo], [hi, hi], [lo, hi]]
    spec["meshes"] = [{"kind": "triangles", "vertices": QUAD, "faces": [[0, 1, 2], [0, 2, 3]],
                       "uvs": [[st[0], st[1], st[2]], [st[0], st[2], st[3]]], "shader": image_shader(image(2, 2))}]
    return spec


ONE = (0.75, 0.25, 0.5)


def quad_1x1(textured=True):
    """Case 3: a 1 x 1 image, and the same mesh in that colour."""
    spec = quad_3x5()
    spec["meshes"][0]["shader"] = image_shader(np.array(ONE).reshape(1, 1, 3)) if textured else shader(ONE)
    return spec


def torus_mirror():
    """Case 4: a smooth textured torus beside the README scene's mirror-like spheres, on its ground sphere."""
    spec = scenes.readme_spec(W, H)
    spec["meshes"] = [{"kind": "torus", "R": 0.5, "r": 0.17, "nu": 16, "nv": 8, "smooth": True, "uv": True,
                       "translation": [0.7, -0.33, 0.9], "shader": image_shader(image(4, 4))}]
    return spec


def mixed():
    """Case 5: two textured meshes with images of different sizes, a checker mesh without uvs, a sphere with
    an image texture and two coloured point lights."""
    spec = torus_mirror()
    spec["spheres"].pop(2)
    spec["spheres"][1]["shader"] = image_shader(image(6, 3))
    spec["meshes"].insert(0, {"kind": "quad", "corners": QUAD, "uv": True, "shader": image_shader(image(3, 5))})
    spec["meshes"].append({"kind": "box", "lo": [-1.6, -0.5, 1.4], "hi": [-1.0, 0.1, 2.0], "shader": shader(checker=True)})
    spec["lights"][0] = {"kind": "point", "position": [5, 10, -10], "intensity": 0.8, "color": [1.0, 0.9, 0.8]}
    spec["lights"].insert(1, {"kind": "point", "position": [-1.33, 8.16, 7.23], "intensity": 0.6, "color": [0.4, 0.6, 1.0]})
    return spec


UV_CASES = {
    "quad_3x5": quad_3x5,
    "quad_wrap": quad_wrap,
    "quad_1x1": quad_1x1,
    "torus_mirror": torus_mirror,
    "mixed": mixed,
    "1x1": lambda: scenes.textured_mesh_spec(1, 1, 1, scenes.uv_grid_texels(8, 8)),
    "7x5": lambda: scenes.textured_mesh_spec(7, 5, 1, scenes.uv_grid_texels(8, 8)),
    "67x5": lambda: scenes.textured_mesh_spec(67, 5, 1, scenes.uv_grid_texels(8, 8)),
}
_frames: dict = {}


def frame(key, cap=3):
    """(spec, the restatement's frame float64 [3, n], its counts), computed once."""
    if (key, cap) not in _frames:
        spec = UV_CASES[key]()
        counts = U.Counts()
        _frames[key, cap] = (spec, U.render(spec, cap, counts=counts), counts)
    return _frames[key, cap]


def table_of(spec, max_leaf=4):
    return M.mesh_table(scenes.build_scene(spec).shapes, max_leaf)


# ---- the OBJ loader -------------------------------------------------------------------------------------------

OBJ = """# a square and a pentagon with texture coordinates: both corner forms, negative vt indices, a third number
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vt 1 0 0.5
vt 1 1
vt 0 1
vn 0 0 1
f 1/1 2/2 3/3
f 1/1/1 3/-2/1 4/-1/1
v 2 0 0
v 3 0 0
v 3.5 1 0
v 2.5 2 0
v 1.5 1 0
vt 0.25 0.5
f 5/1 6/2 7/3 8/4 9/-1
"""


def test_load_obj_reads_vt_in_both_corner_forms_negative_indices_and_a_fan(tmp_path):
    path = tmp_path / "uv.obj"
    path.write_text(OBJ)
    m = M.load_obj(path, "shader")
    assert m.vertices.shape == (9, 3) and m.faces.shape == (5, 3) and m.normals is None
    assert m.uvs.shape == (5, 3, 2) and m.uvs.dtype == np.float64
    assert np.array_equal(m.uvs[0], [[0, 0], [1, 0], [1, 1]])  # v/vt; the third number of a vt is ignored
    assert np.array_equal(m.uvs[1], [[0, 0], [1, 1], [0, 1]])  # v/vt/vn with negative vt indices
    fan = [[0, 0], [1, 0], [1, 1], [0, 1], [0.25, 0.5]]  # -1 is the fifth vt by then
    assert np.array_equal(m.uvs[2:], [[fan[0], fan[i], fan[i + 1]] for i in (1, 2, 3)])
    assert np.array_equal(m.faces[2:], [[4, 5, 6], [4, 6, 7], [4, 7, 8]])
    # smooth changes the vertices (here: the file's vn), never the per-corner uvs
    s = M.load_obj(path, None, smooth=True)
    assert np.array_equal(s.uvs, m.uvs) and np.array_equal(s.faces, m.faces) and s.normals is not None
    assert "uvs" in repr(m)


@pytest.mark.parametrize("text", ["v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3\n",  # one corner without vt
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3//1\n",  # ... with v//vn
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/2\n",  # a vt that does not exist
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/-2\n",  # ... counted back
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0\nf 1/1 2/1 3/1\n",  # a vt of one number
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n"])
def test_load_obj_keeps_no_uvs_unless_every_corner_has_one(tmp_path, text):
    path = tmp_path / "part.obj"
    path.write_text(text)
    m = M.load_obj(path, None)
    assert m.uvs is None and m.faces.shape == (1, 3) and "uvs" not in repr(m)


# ---- the generators -------------------------------------------------------------------------------------------

def test_generators_texture_coordinates():
    q = M.quad(QUAD, None, uv=True)
    corner = {0: (0, 0), 1: (1, 0), 2: (1, 1), 3: (0, 1)}
    assert q.uvs.shape == (2, 3, 2) and np.array_equal(q.uvs, [[corner[i] for i in f] for f in q.faces])
    b = M.box([0, 0, 0], [1, 2, 3], None, uv=True)
    assert b.uvs.shape == (12, 3, 2)
    for k in range(6):  # every face: 0..1, the quad's coordinates
        assert np.array_equal(b.uvs[2 * k:2 * k + 2], q.uvs)
    nu, nv = 5, 4
    t = M.torus(1.0, 0.25, nu, nv, None, smooth=True, uv=True)
    assert t.uvs.shape == (2 * nu * nv, 3, 2) and t.uvs.min() == 0.0 and t.uvs.max() == 1.0
    # per corner: s = i / nu and t = j / nv of the corner's own segment, so the last segment ends at 1, not at 0
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i, j = i.ravel(), j.ravel()
    assert np.array_equal(t.uvs[:nu * nv, 0], np.stack([i / nu, j / nv], 1))
    assert np.array_equal(t.uvs[:nu * nv, 1], np.stack([(i + 1) / nu, (j + 1) / nv], 1))
    assert np.array_equal(t.uvs[:nu * nv, 2], np.stack([(i + 1) / nu, j / nv], 1))
    assert np.array_equal(t.uvs[nu * nv:, 1], np.stack([i / nu, (j + 1) / nv], 1))
    last = t.uvs[:nu * nv][i == nu - 1]
    assert (last[:, 1, 0] == 1.0).all() and (last[:, 0, 0] == (nu - 1) / nu).all()
    # the seam needs no split vertex: the last segment's far corners are the first segment's vertices (the ring
    # i = 0), which carry s = 0 in the first segment's faces and s = 1 here
    assert (t.faces[:nu * nv][i == nu - 1][:, 1] < nv).all() and (t.uvs[:nu * nv][i == 0][:, 0, 0] == 0.0).all()


def test_generators_without_uv_return_what_they_returned():
    for make in (lambda **kw: M.quad(QUAD, "s", **kw), lambda **kw: M.box([0, 0, 0], [1, 2, 3], "s", **kw),
                 lambda **kw: M.torus(1.0, 0.25, 5, 4, "s", True, **kw)):
        a, b, c = make(), make(uv=False), make(uv=True)
        assert a.uvs is None and b.uvs is None and c.uvs is not None
        for x in (b, c):
            assert np.array_equal(a.vertices, x.vertices) and np.array_equal(a.faces, x.faces)
            assert (a.normals is None) == (x.normals is None) and (a.normals is None or np.array_equal(a.normals, x.normals))
    assert M.icosphere(1, None).uvs is None
    placed = M.quad(QUAD, None, uv=True).placed(2.0, (1, 2, 3))
    assert np.array_equal(placed.uvs, M.quad(QUAD, None, uv=True).uvs)


def test_per_vertex_uvs_are_expanded_per_corner():
    from python_ray_tracer_amd.domain import TriangleMesh

    st = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64)
    m = TriangleMesh(QUAD, [[0, 1, 2], [0, 2, 3]], None, None, st)
    assert m.uvs.shape == (2, 3, 2) and np.array_equal(m.uvs, M.quad(QUAD, None, uv=True).uvs)


# ---- the table ------------------------------------------------------------------------------------------------

def _parts(table):
    T, Mn = int(table[M.MH_NTRI]), int(table[M.MH_NMESH])
    rows = table[int(table[M.MH_TRIS]):][:T * M.TRI_WORDS].reshape(T, M.TRI_WORDS)
    mats = table[int(table[M.MH_MATS]):][:Mn * L.MAT_WORDS].reshape(Mn, L.MAT_WORDS)
    u = int(table[M.MH_UVS])
    return rows, mats, table[u:u + T * M.UV_WORDS].reshape(T, M.UV_WORDS)


@pytest.mark.parametrize("max_leaf", [1, 2, 4, 8, None])
def test_the_uv_part_follows_the_rows_leaf_order_and_the_blocks_are_the_images(max_leaf):
    spec = mixed()
    scene = scenes.build_scene(spec)
    table = table_of(spec, max_leaf)
    M.check_table(table)
    rows, mats, uv = _parts(table)
    meshes = [s for s in scene.shapes if hasattr(s, "faces")]
    want = np.concatenate([np.zeros((len(m.faces), 6)) if m.uvs is None else m.uvs.reshape(-1, 6) for m in meshes])
    num = rows[:, M.T_NUM].astype(int)
    assert sorted(num) == list(range(len(want))) and np.array_equal(uv, want[num])
    assert (uv[rows[:, M.T_MESH] == 2] == 0).all() and uv[rows[:, M.T_MESH] == 1].any()  # the checker box has none
    # the header: the two parts after the nodes, in this order, to the table's end
    nodes_end = int(table[M.MH_NODES]) + int(table[M.MH_NNODES]) * L.NODE_WORDS
    assert table[M.MH_UVS] == nodes_end and table[M.MH_TEXELS] == nodes_end + 6 * len(want)
    assert table[M.MH_WORDS] == table.size == table[M.MH_TEXELS] + 3 * (3 * 5 + 4 * 4) and not table[10:16].any()
    # the material rows: the block's offset in the table, the width, the height; row 0 of the image first
    for mi, (w, h) in ((0, (3, 5)), (1, (4, 4))):
        assert mats[mi, L.M_TEX] == L.TEX_IMAGE and (mats[mi, L.M_TG], mats[mi, L.M_TB]) == (w, h)
        off = int(mats[mi, L.M_TR])
        assert np.array_equal(table[off:off + 3 * w * h].reshape(h, w, 3), image(w, h))
    assert mats[0, L.M_TR] == table[M.MH_TEXELS] and mats[1, L.M_TR] == mats[0, L.M_TR] + 45
    assert mats[2, L.M_TEX] == L.TEX_CHECKER


def test_a_shared_image_is_stored_once_and_the_digest_sees_uvs_and_images():
    spec = quad_3x5()
    spec["meshes"].append({"kind": "box", "lo": [0, 0, 0], "hi": [1, 1, 1], "uv": True, "shader": image_shader(image(3, 5))})
    table = table_of(spec)
    M.check_table(table)
    _, mats, _ = _parts(table)
    assert mats[0, L.M_TR] == mats[1, L.M_TR] == table[M.MH_TEXELS] and table.size == table[M.MH_TEXELS] + 45
    # another image of the same size, or other coordinates: another table (the cache is keyed by content)
    other = copy.deepcopy(spec)
    other["meshes"][1]["shader"] = image_shader(image(3, 5)[::-1])
    t2 = table_of(other)
    assert t2.size == table.size + 45 and not np.array_equal(t2[:table.size], table)
    moved = scenes.build_scene(spec)
    moved.shapes[-1].uvs = moved.shapes[-1].uvs * 0.5
    t3 = M.mesh_table(moved.shapes)
    assert t3.size == table.size and not np.array_equal(t3, table)
    assert np.array_equal(table_of(spec), table)


def test_uvs_without_an_image_texture_change_no_byte():
    for key in ("quad", "mesh_only", "readme_mesh"):
        spec = CASES[key]()
        with_uv = copy.deepcopy(spec)
        for m in with_uv["meshes"]:
            if m["kind"] in ("quad", "box", "torus"):
                m["uv"] = True
        a, b = table_of(spec), table_of(with_uv)
        assert any(s.uvs is not None for s in scenes.build_scene(with_uv).shapes if hasattr(s, "faces"))
        assert a.tobytes() == b.tobytes() and a[M.MH_UVS] == 0 and a[M.MH_TEXELS] == 0, key
        assert not M.has_image(scenes.build_scene(with_uv).shapes)
    assert M.has_image(scenes.build_scene(quad_3x5()).shapes)


def test_check_table_refuses_new_offsets_that_do_not_fit():
    table = table_of(mixed())
    M.check_table(table)
    mats_at = int(table[M.MH_MATS])
    for word, value in ((M.MH_UVS, 3.0), (M.MH_UVS, float(table.size)), (M.MH_UVS, table[M.MH_UVS] + 0.5),
                        (M.MH_TEXELS, 0.0), (M.MH_TEXELS, float(table.size + 1)), (M.MH_UVS, 0.0),
                        (mats_at + L.M_TR, float(table.size - 3)), (mats_at + L.M_TR, 20.0), (mats_at + L.M_TG, 0.0),
                        (mats_at + L.M_TB, 2.0 ** 21), (mats_at + L.M_TG, 2.5), (M.MH_UVS, np.inf), (M.MH_TEXELS, np.nan),
                        (mats_at + L.M_TR, np.inf), (mats_at + L.M_TG, np.nan)):
        bad = table.copy()
        bad[word] = value
        with pytest.raises(ValueError, match="mesh table"):
            M.check_table(bad)
    with pytest.raises(ValueError, match="mesh table"):
        M.check_table(table[:-1])


# ---- refusals, all before any device use ------------------------------------------------------------------------

class _NoDevice:
    """Stands where the renderer keeps its library and its device: any use of either fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after a use of the library or the device ({name})")


def _renderer(monkeypatch):
    """A HipRenderer that never saw its constructor (tests/test_mesh_cpu.py's, restated)."""
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer

    def no_gpu(*a, **k):
        raise AssertionError("the refusal came after a torch.cuda call")

    for name in ("current_device", "set_device", "current_stream", "is_current_stream_capturing"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    r = object.__new__(HipRenderer)
    r.__dict__.update(_lib=_NoDevice(), device=_NoDevice(), max_bounces=3, samples=1, adaptive=False,
                      color_dtype=torch.float64, mesh_max_leaf=4, _light_tables=_NoDevice(), _glass_tables=_NoDevice(),
                      _mesh_tables=_NoDevice(), _scene_cache=_NoDevice())
    return r


def test_every_new_refusal_comes_before_any_gpu_use(monkeypatch):
    from python_ray_tracer_amd.infrastructure.hip import HipVector3D, ImageTexture

    r = _renderer(monkeypatch)
    d = HipVector3D(np.array([0.0]), np.array([0.0]), np.array([1.0]))

    def refused(change, what):
        for call in (r.render, r.render_tile, lambda s: r.raytrace_scene(s.camera.position, d, s)):
            scene = scenes.build_scene(quad_3x5())
            change(scene.shapes[-1])
            with pytest.raises(ValueError, match=what):
                call(scene)

    def set_uvs(value):
        def change(mesh):
            mesh.uvs = value
        return change

    def poke(index, value):
        def change(mesh):
            mesh.uvs[index] = value
        return change

    def huge_image(mesh):
        mesh.shader.diffuse_color = ImageTexture(np.ones((2, 2, 3)))
        mesh.shader.diffuse_color.texels = np.broadcast_to(np.ones(3), (1025, 1024, 3))  # (no memory: a view)

    refused(set_uvs(None), "mesh 0.*ImageTexture.*texture coordinates")
    refused(set_uvs(np.zeros((2, 3, 3))), "mesh 0: uvs must be")
    refused(set_uvs(np.zeros((3, 3, 2))), "mesh 0: uvs must be")
    refused(set_uvs(np.zeros((4, 2))), "mesh 0: uvs must be")  # (per vertex is expanded by the constructor alone)
    refused(poke((1, 2, 0), np.nan), "mesh 0.*not finite")
    refused(poke((0, 0, 1), np.inf), "mesh 0.*not finite")
    refused(poke((1, 1, 1), 1024.5), "mesh 0.*1024")
    refused(poke((0, 2, 0), -1025.0), "mesh 0.*1024")
    refused(huge_image, "mesh 0.*RTX_MAX_TEXELS")
    # the limit itself is allowed, and bad uvs are refused on a mesh without an image too
    scene = scenes.build_scene(quad_3x5())
    scene.shapes[-1].uvs[0, 0] = (1024.0, -1024.0)
    assert r._mesh_table(scene, "render").uv
    plain = scenes.build_scene(CASES["quad"]())
    plain.shapes[-1].uvs = np.full((2, 3, 2), np.nan)
    with pytest.raises(ValueError, match="not finite"):
        r.render(plain)
    assert not r._mesh_table(scenes.build_scene(CASES["quad"]()), "render").uv


# ---- the restatement ------------------------------------------------------------------------------------------

def test_the_lookup_by_hand():
    """A 3 x 2 image under the coordinates ``quad`` gives its first triangle: texel centres, a boundary, the
    repeat on both axes and negative coordinates."""
    img = image(3, 2)
    st = M.quad(QUAD, None, uv=True).uvs[:1].reshape(1, 6)  # (0, 0), (1, 0), (1, 1): s = u + v, t = v

    def at(s, t):
        return np.array(U.lookup(img, st, np.array([float(s) - float(t)]), np.array([float(t)]))).ravel()

    assert np.array_equal(at(0.5, 0.25), img[1, 1]) and np.array_equal(at(0.5, 0.75), img[0, 1])  # t = 0: the bottom row
    assert np.allclose(at(1 / 3, 0.25), (img[1, 0] + img[1, 1]) / 2, rtol=0, atol=1e-15)
    assert np.array_equal(at(0.5, 0.5), (img[0, 1] + img[1, 1]) * 0.5)  # fy = 0.5 exactly
    assert np.array_equal(at(0.5, 0.0), (img[1, 1] + img[0, 1]) * 0.5)  # the bottom edge: the top row wraps in
    assert np.allclose(at(0.0, 0.25), (img[1, 2] + img[1, 0]) / 2, rtol=0, atol=1e-15)  # the left edge: column 2 wraps in
    assert np.array_equal(at(-0.5, -0.75), at(0.5, 0.25)) and np.array_equal(at(2.5, 1.25), at(0.5, 0.25))
    c = U.Counts()
    U.lookup(img, st, np.array([-0.75]), np.array([0.75]), c)  # s = 0, t = 0.75
    assert (c.wrapped_x, c.wrapped_y, c.negative, c.fractional) == (1, 0, 1, 1)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", sorted(CASES))
def test_restatement_is_the_mesh_restatement_where_no_mesh_has_an_image(key, cap):
    spec, want, counts = plain_frame(key, cap)
    c = U.Counts()
    assert np.array_equal(U.render(spec, cap, counts=c), want)
    assert c.rays == counts.rays and c.tri_primary == counts.tri_primary and c.tex_primary == c.tex_reflected == 0


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", sorted(UV_CASES))
def test_pruning_changes_no_frame(key, cap):
    spec, want, _ = frame(key, cap)
    for leaf in (1, 4):
        assert np.array_equal(U.render(spec, cap, prune=R.Pruner(table_of(spec, leaf))), want), leaf


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", sorted(UV_CASES))
def test_no_pixel_of_a_gpu_case_sits_on_a_quantisation_step(key, cap):
    assert step_distance(frame(key, cap)[1]) > 1e-9


def test_preconditions_of_the_gpu_cases():
    c = frame("quad_3x5")[2]
    assert c.tex_primary > 300 and c.tex_reflected > 0 and c.fractional > 300 and c.meshes_hit == {0}
    got = O.to_uint8(frame("quad_3x5")[1], W, H).reshape(-1, 3)
    assert len(np.unique(got, axis=0)) > 100  # the image shows: far more colours than a constant floor has
    c = frame("quad_wrap")[2]
    assert c.tex_primary > 300 and c.wrapped_x > 0 and c.wrapped_y > 0 and c.negative > 0
    # the 1 x 1 image is its colour everywhere: the restatement's frame is the constant mesh's, bit for bit
    c = frame("quad_1x1")[2]
    assert c.tex_primary > 300
    for cap in CAPS:
        assert np.array_equal(frame("quad_1x1", cap)[1], R.render(quad_1x1(False), cap))
    c = frame("torus_mirror")[2]
    assert c.tex_primary > 20 and c.tex_reflected > 0 and c.seam_hits > 0 and c.smooth_hits > 0 and c.sphere_to_tri > 0
    assert c.tri_ties == 0  # (the permutation test: no two triangles at one distance)
    c = frame("mixed")[2]
    spec = mixed()
    assert c.meshes_hit == {0, 1} and R.table_of(spec).shape == (2, 6) and c.tri_primary > 300
    assert spec["spheres"][1]["shader"]["texture"]["kind"] == "image" and spec["meshes"][2].get("uv") is None
    osc = O.scene_from_spec(spec)
    d = O.ray_directions(osc.cam, W, H)
    near = np.minimum.reduce([O.intersect(sp, *osc.cam, *d) for sp in osc.spheres])
    assert ((O.intersect(osc.spheres[1], *osc.cam, *d) == near) & (near != O.FARAWAY)).sum() > 10  # the textured sphere shows
    g = U.group_of(spec)
    t, num, *_ = R.nearest_triangle(g.g, *osc.cam, *d)
    assert ((g.g.mesh[num] == 2) & (t != O.FARAWAY) & (t < near)).sum() > 5  # ... and so does the checker box
    for key in ("1x1", "7x5", "67x5"):
        assert frame(key)[2].rays > 0
    assert frame("7x5")[2].tex_primary > 0 and frame("67x5")[2].tex_primary > 0
    assert frame("quad_3x5", 0)[2].rays == W * H and frame("quad_3x5", 0)[2].tex_reflected == 0


# ---- explicit rays: exact cases ---------------------------------------------------------------------------------

TEXELS_2X2 = np.array([[[0.5, 0.25, 1.0], [0.25, 0.5, 0.125]], [[1.0, 0.5, 0.25], [0.125, 0.75, 0.5]]])


def exact_cases():
    """name -> (spec, origins [3, n], directions [3, n], the constant colour each ray's hit must shade with).
    A quad over [-1, 1]^2 at z = 2 under a 2 x 2 image of dyadic colours, rays along +z from dyadic points."""
    quad = [[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]]  # uv (0,0) (1,0) (1,1) (0,1): s grows with y, t with x
    z = lambda *pts: (np.array([[x, y, -2.0] for x, y in pts]).T, np.array([[0.0, 0.0, 1.0]] * len(pts)).T)  # noqa: E731
    T = TEXELS_2X2
    textured = exact_spec([{"kind": "quad", "corners": quad, "uv": True, "shader": image_shader(T)}])
    # two triangles that share the diagonal, the first all in the bottom-left texel, the second in the top-right
    a, b = [0.25, 0.25], [0.75, 0.75]
    split = exact_spec([{"kind": "triangles", "vertices": quad, "faces": [[0, 1, 2], [0, 2, 3]],
                         "uvs": [[a, a, a], [b, b, b]], "shader": image_shader(T)}])
    return {
        # s = (y + 1) / 2, t = (x + 1) / 2: texel centres at +-0.5
        "centres": (textured, *z((-0.5, -0.5), (-0.5, 0.5), (0.5, -0.5), (0.5, 0.5)), [T[1, 0], T[1, 1], T[0, 0], T[0, 1]]),
        # on the boundary between two texels: their mean (fx = 0.5, then fy = 0.5, then all four)
        "boundaries": (textured, *z((-0.5, 0.0), (0.0, -0.5), (0.0, 0.0)),
                       [(T[1, 0] + T[1, 1]) / 2, (T[1, 0] + T[0, 0]) / 2, (T[0, 0] + T[0, 1] + T[1, 0] + T[1, 1]) / 4]),
        # a ray through the edge the two triangles share takes the lower-numbered triangle's coordinates
        "shared_edge": (split, *z((0.0, 0.0), (0.5, 0.5), (-0.25, 0.5), (0.5, -0.25)), [T[1, 0], T[1, 0], T[1, 0], T[0, 1]]),
    }


@pytest.mark.parametrize("name", sorted(exact_cases()))
def test_exact_rays_of_the_restatement(name):
    spec, o, d, colours = exact_cases()[name]
    c = U.Counts()
    got = U.trace_rays(spec, tuple(o), tuple(d), 3, c)
    assert c.tex_primary == len(colours) and np.isfinite(got).all()
    for k, colour in enumerate(colours):  # the same hit on the same mesh in that constant colour, bit for bit
        const = copy.deepcopy(spec)
        const["meshes"][0]["shader"] = shader(tuple(float(x) for x in colour))
        want = R.trace_rays(const, tuple(o[:, k:k + 1]), tuple(d[:, k:k + 1]), 3)
        assert np.array_equal(got[:, k:k + 1], want), (name, k)
    if name == "shared_edge":
        assert c.tri_ties == 2
    if name == "centres":
        assert c.fractional == 0


# ---- the C ABI and the op without a GPU ---------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_and_the_header_words():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"\brtx_trace_mesh_uv\(", text) and "rtx_trace_mesh_uv" in L.EXPORTS
    assert hasattr(L.load(), "rtx_trace_mesh_uv") and L._SIGS["rtx_trace_mesh_uv"] == L._SIGS["rtx_trace_mesh"]
    assert f"RTX_MH_UVS = {M.MH_UVS}" in text and f"RTX_MH_TEXELS = {M.MH_TEXELS}" in text
    assert f"RTX_UV_WORDS = {M.UV_WORDS}" in text and f"RTX_MESH_UV_MAX = {int(M.UV_MAX)}" in text
    assert 8 <= M.MH_UVS < M.MH_TEXELS < M.HDR_WORDS and M.MAX_TEXELS == L.MAX_TEXELS
    assert L.ABI_VERSION == 3 and "#define RTX_ABI_VERSION 3" in text


def test_argument_checks_need_no_gpu():
    lib = L.load()
    p = ctypes.c_void_p(4096)

    def call(scene=p, S=3, mesh=p, words=1000, table=p, nl=2, origins=p, stride=0, dirs=p, n=8, B=3, out=p, kind=1, ws=p,
             ws_bytes=1 << 30):
        return lib.rtx_trace_mesh_uv(scene, S, mesh, words, table, nl, origins, stride, dirs, n, B, out, kind, ws,
                                     ws_bytes, None)

    for kw, what in (({"scene": None}, b"null scene"), ({"mesh": None}, b"null mesh"), ({"table": None}, b"null lights"),
                     ({"origins": None}, b"null ray"), ({"dirs": None}, b"null ray"), ({"out": None}, b"null output"),
                     ({"ws": None}, b"null workspace"), ({"S": -1}, b"n_spheres"), ({"S": 1025}, b"n_spheres"),
                     ({"words": 15}, b"mesh_words"), ({"words": 1 << 31}, b"mesh_words"), ({"nl": 0}, b"n_lights"),
                     ({"nl": 9}, b"n_lights"), ({"B": -1}, b"max_bounces"), ({"B": 17}, b"max_bounces"),
                     ({"kind": 3}, b"out_kind"), ({"n": -1}, b"negative"), ({"stride": 5}, b"origin_stride")):
        assert call(**kw) == -1 and what in lib.rtx_last_error(), kw
    need = lib.rtx_mesh_workspace_bytes(8, 3)
    assert call(ws_bytes=need - 1) == -3 and b"workspace too small" in lib.rtx_last_error()
    assert call(n=0) == 0 and call(n=0, S=0, B=16, nl=8, kind=2, ws_bytes=L.WS_HDR_BYTES) == 0


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "trace_mesh_uv" in ops.OPS
    assert str(torch.ops.rt.trace_mesh_uv.default._schema) == \
        ("rt::trace_mesh_uv(Tensor scene, int n_spheres, Tensor mesh, Tensor lights, Tensor origins, Tensor dirs, "
         "int max_bounces, int out_kind, bool check=True) -> Tensor")
    S, n = 3, 77

    def args(dev="meta", **kw):
        a = dict(scene=torch.zeros(L.HDR_WORDS + S * (L.GEOM_WORDS + L.MAT_WORDS), dtype=torch.float64, device=dev),
                 S=S, mesh=torch.zeros(500, dtype=torch.float64, device=dev),
                 lights=torch.zeros(3, 6, dtype=torch.float64, device=dev),
                 origins=torch.zeros(3, dtype=torch.float64, device=dev),
                 dirs=torch.zeros(3, n, dtype=torch.float64, device=dev), B=3, kind=1)
        a.update(kw)
        return tuple(a.values())

    for kind, shape, dtype in ((0, (3, n), torch.float32), (1, (3, n), torch.float64), (2, (n, 3), torch.uint8)):
        out = torch.ops.rt.trace_mesh_uv(*args(kind=kind))
        assert out.device.type == "meta" and tuple(out.shape) == shape and out.dtype == dtype
    meta = dict(device="meta", dtype=torch.float64)
    for bad, what in (({"mesh": torch.zeros(15, **meta)}, "mesh must be"), ({"lights": torch.zeros(9, 6, **meta)}, "lights"),
                      ({"dirs": torch.zeros(n, 3, **meta)}, "dirs"), ({"origins": torch.zeros(3, n + 1, **meta)}, "origins"),
                      ({"B": 17}, "max_bounces"), ({"kind": 3}, "out_kind"), ({"S": 4}, "too short")):
        with pytest.raises(RuntimeError, match=what):
            torch.ops.rt.trace_mesh_uv(*args(**bad))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_mesh_uv(*args(dev="cpu"))


def test_the_renderer_picks_the_entry_by_the_table(monkeypatch):
    """_trace_mesh without a kernel: a table with a UV part goes to rtx_trace_mesh_uv, any other to rtx_trace_mesh."""
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer, base

    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    calls = []

    class Lib:
        def rtx_mesh_workspace_bytes(self, n, B):
            return 64

        def rtx_trace_mesh(self, *a):
            calls.append("rtx_trace_mesh")
            return 0

        def rtx_trace_mesh_uv(self, *a):
            calls.append("rtx_trace_mesh_uv")
            return 0

    r = object.__new__(HipRenderer)
    t = torch.zeros(16, dtype=torch.float64)
    r.__dict__.update(_lib=Lib(), device=torch.device("cpu"), max_bounces=3, _mesh_ws=torch.zeros(64, dtype=torch.uint8),
                      _mesh_clean={}, _mesh_tables={"k": t}, _light_tables={b"l": torch.zeros(1, 6, dtype=torch.float64)},
                      _graph_pins={}, _stream=lambda: 0)
    monkeypatch.setattr(r, "_read_status", lambda ws: 0, raising=False)
    r._trace_mesh(t, 0, base._MeshTable(None, None, ("k", b"l"), True), 0, 0, t, 4, t, 1)
    r._trace_mesh(t, 0, base._MeshTable(None, None, ("k", b"l")), 0, 0, t, 4, t, 1)
    assert calls == ["rtx_trace_mesh_uv", "rtx_trace_mesh"]


def test_specs_and_build_scene():
    from python_ray_tracer_amd.infrastructure.hip import ImageTexture

    g = scenes.uv_grid_texels(16, 8)
    assert g.shape == (8, 16, 3) and g.dtype == np.float64 and 0.0 <= g.min() and g.max() <= 1.0
    assert g[0, 0, 1] > g[-1, 0, 1] and g[0, -1, 0] > g[0, 0, 0]  # green grows upwards (row 0 is the top), red rightwards
    with pytest.raises(ValueError, match="uv_grid_texels"):
        scenes.uv_grid_texels(0, 4)
    spec = scenes.textured_mesh_spec(64, 36)
    assert [m["kind"] for m in spec["meshes"]] == ["quad", "icosphere", "torus"]
    assert [m.get("uv", False) for m in spec["meshes"]] == [True, False, True]
    scene = scenes.build_scene(spec)
    quad, ico, torus = scene.shapes[2:]
    assert isinstance(quad.shader.diffuse_color, ImageTexture) and quad.shader.diffuse_color is not torus.shader.diffuse_color
    assert quad.uvs.shape == (2, 3, 2) and ico.uvs is None and torus.uvs.shape == (1024, 3, 2) and torus.normals is not None
    table = M.mesh_table(scene.shapes)
    M.check_table(table)
    assert table[M.MH_UVS] > 0 and table.size == table[M.MH_TEXELS] + 64 * 64 * 3  # the shared image once
    # a spec's "uvs" for kind "triangles"
    tri = {"kind": "triangles", "vertices": QUAD, "faces": [[0, 1, 2]], "uvs": [[[0, 0], [1, 0], [1, 1]]], "shader": shader()}
    assert np.array_equal(scenes.mesh_of(tri).uvs, [[[0, 0], [1, 0], [1, 1]]])
    # the plain mesh spec is what it was
    assert all("uv" not in m for m in scenes.mesh_spec(8, 8)["meshes"])
    assert all(s.uvs is None for s in scenes.build_scene(scenes.mesh_spec(8, 8, 1)).shapes[2:])
