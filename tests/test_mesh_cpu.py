"""Triangle meshes without a GPU: the OBJ loader, the generators, the refusals, the device table and its
tree, the NumPy restatement (tests/mesh_ref.py) with and without the tree's pruning, and the
preconditions of every frame tests/test_gpu_mesh.py renders."""

import copy
import ctypes
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.domain import Shape, TriangleMesh
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import lights_ref
from tests import mesh_ref as R
from tests.test_lights_cpu import step_distance

REPO = Path(__file__).resolve().parent.parent
W, H = 48, 27
GAINS = (0.8, 1.0, 0.5, 0.05, 1.0)


def shader(color=(0.2, 0.6, 1.0), gains=GAINS, checker=False):
    return scenes._shader(*gains, scenes._checker() if checker else scenes._const(*color))


def quad_spec(w=W, h=H):
    """The README scene on a two-triangle checkered quad in place of its ground sphere."""
    spec = scenes.readme_spec(w, h)
    ground = spec["spheres"].pop(2)
    spec["meshes"] = [{"kind": "quad", "corners": [[-40, -0.5, -10], [-40, -0.5, 60], [40, -0.5, 60], [40, -0.5, -10]],
                       "shader": ground["shader"]}]
    return spec


def ico_spec(level, smooth):
    """A reflective icosphere between the README scene's spheres, on its ground sphere."""
    spec = scenes.readme_spec(W, H)
    spec["meshes"] = [{"kind": "icosphere", "level": level, "smooth": smooth, "scale": 0.4,
                       "translation": [-0.05, 0.0, 1.9], "shader": shader()}]
    return spec


def torus_spec():
    """A 16 x 8 torus that stands on its side over the ground: the light passes through its hole on to the
    ground, and its far side lies in the shadow of its near side."""
    spec = scenes.readme_spec(W, H)
    del spec["spheres"][1]
    v, f, n = scenes.mesh_arrays({"kind": "torus", "R": 0.45, "r": 0.16, "nu": 16, "nv": 8})
    v = v[:, [0, 2, 1]] * np.array([1.0, 1.0, -1.0])  # about the z axis (a rotation: the winding stays)
    spec["meshes"] = [{"kind": "triangles", "vertices": v.tolist(), "faces": f.tolist(), "scale": 1.0,
                       "translation": [-0.35, 0.15, 1.0], "shader": shader((1.0, 0.6, 0.1))}]
    return spec


def mesh_only_spec():
    spec = quad_spec()
    spec["spheres"] = []
    spec["meshes"].append({"kind": "box", "lo": [0.3, -0.5, 1.2], "hi": [1.0, 0.25, 1.9], "shader": shader()})
    spec["meshes"].append(torus_spec()["meshes"][0])
    return spec


def two_lights_spec():
    spec = scenes.mesh_spec(W, H, 1)
    spec["lights"].insert(1, {"kind": "point", "position": [-1.33, 8.16, 7.23], "intensity": 0.6,
                              "color": [1.0, 0.7, 0.4]})
    spec["lights"].insert(2, {"kind": "point", "position": [0.18, 9.4, 3.89], "intensity": 0.4, "color": [0.4, 0.6, 1.0]})
    return spec


def tree_spec():
    """17 spheres (a culling tree in the shadow searches) around an icosphere."""
    spec = scenes.random_spec(16, 1, W, H)
    spec["meshes"] = [{"kind": "icosphere", "level": 1, "smooth": True, "scale": 0.5, "translation": [0.0, 0.3, 2.0],
                       "shader": shader((0.9, 0.9, 0.2))}]
    return spec


CASES = {
    "quad": quad_spec,
    "ico1_flat": lambda: ico_spec(1, False),
    "ico1_smooth": lambda: ico_spec(1, True),
    "ico2_flat": lambda: ico_spec(2, False),
    "ico2_smooth": lambda: ico_spec(2, True),
    "torus": torus_spec,
    "mesh_only": mesh_only_spec,
    "two_lights": two_lights_spec,
    "tree17": tree_spec,
    "readme_mesh": lambda: scenes.mesh_spec(W, H, 1),
    "1x1": lambda: scenes.mesh_spec(1, 1, 1),
    "7x5": lambda: scenes.mesh_spec(7, 5, 1),
    "67x5": lambda: scenes.mesh_spec(67, 5, 1),
}
CAPS = (0, 3)
_frames: dict = {}


def frame(key, cap=3):
    """(spec, the restatement's frame float64 [3, n], its counts), computed once."""
    if (key, cap) not in _frames:
        spec = CASES[key]()
        counts = R.Counts()
        _frames[key, cap] = (spec, R.render(spec, cap, counts=counts), counts)
    return _frames[key, cap]


def table_of(spec, max_leaf=4):
    return M.mesh_table(scenes.build_scene(spec).shapes, max_leaf)


# ---- the OBJ loader -------------------------------------------------------------------------------------------

OBJ = """# a square pyramid: every index form, a negative index, a pentagon
mtllib nothing.mtl
o pyramid
v 0 0 0
v 1 0 0
v 1 0 1
v 0 0 1
v 0.5 1 0.5
vt 0 0
vn 0 -1 0
vn 0 0.4472135955 -0.894427191
s off
f 1 2 5
f 2/1 3/1 5/1
f 3//2 4//2 5//2
f 4/1/2 1/1/2 -1/1/2
f 1 4 3 2
v 2 0 0
v 3 0 0
v 3.5 0 1
v 2.5 0 2
v 1.5 0 1
f -5 -4 -3 -2 -1
usemtl none
"""


def test_load_obj_index_forms_negative_indices_and_polygons(tmp_path):
    path = tmp_path / "pyramid.obj"
    path.write_text(OBJ)
    m = M.load_obj(path, "shader")
    assert isinstance(m, TriangleMesh) and isinstance(m, Shape) and m.shader == "shader" and m.normals is None
    assert m.vertices.shape == (10, 3) and m.faces.shape == (4 + 2 + 3, 3)
    assert np.array_equal(m.faces[:4], [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])  # -1 is the fifth vertex
    assert np.array_equal(m.faces[4:6], [[0, 3, 2], [0, 2, 1]])  # a quad: a fan from its first corner
    assert np.array_equal(m.faces[6:], [[5, 6, 7], [5, 7, 8], [5, 8, 9]])  # a pentagon, negative indices
    assert np.array_equal(m.vertices[4], [0.5, 1, 0.5]) and np.array_equal(m.vertices[9], [1.5, 0, 1])
    # without vn for every corner, smooth=True computes area-weighted normals
    s = M.load_obj(path, None, smooth=True)
    assert s.normals.shape == s.vertices.shape and np.array_equal(s.faces, m.faces)
    assert np.allclose(np.linalg.norm(s.normals, axis=1), 1.0)
    assert np.allclose(s.normals[5:], [0, -1, 0])  # the pentagon's winding faces down
    assert np.allclose(s.normals, M.vertex_normals(m.vertices, m.faces))


def test_load_obj_with_a_normal_at_every_corner(tmp_path):
    path = tmp_path / "tri.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvn 0 0 1\nvn 0 0.6 0.8\n"
                    "f 1//1 2//1 3//1\nf 2//1 4//2 3/9/2\n")
    s = M.load_obj(path, None, smooth=True)
    # vertex 3 carries two normals: it is split
    assert s.vertices.shape == (5, 3) and s.normals.shape == (5, 3) and s.faces.shape == (2, 3)
    assert np.array_equal(s.normals[s.faces[0]], [[0, 0, 1]] * 3)
    assert np.array_equal(s.normals[s.faces[1]], [[0, 0, 1], [0, 0.6, 0.8], [0, 0.6, 0.8]])
    flat = M.load_obj(path, None)
    assert flat.normals is None and flat.vertices.shape == (4, 3)
    assert np.array_equal(flat.faces, [[0, 1, 2], [1, 3, 2]])


@pytest.mark.parametrize("text, what", [("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "out of range"),
                                        ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", "out of range"),
                                        ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n", "out of range"),
                                        ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x\n", "bad vertex index"),
                                        ("v 0 0\n", "three numbers"), ("v 0 0 zero\n", "bad v record"),
                                        ("v 0 0 0\nv 1 0 0\nf 1 2\n", "three corners"),
                                        ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\n", "normal index")])
def test_load_obj_refuses(tmp_path, text, what):
    path = tmp_path / "bad.obj"
    path.write_text(text)
    with pytest.raises(ValueError, match=what):
        M.load_obj(path, None)


# ---- the generators -------------------------------------------------------------------------------------------

def _edge_use(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def _outward(mesh, centre_of):
    v, f = mesh.vertices, mesh.faces
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    c = v[f].mean(axis=1)
    return ((n * (c - centre_of(c))).sum(axis=1) > 0).all()


def test_generators_count_their_triangles_and_are_closed():
    for level in range(4):
        m = M.icosphere(level, None)
        assert m.faces.shape == (20 * 4 ** level, 3) and (_edge_use(m.faces) == 2).all()
        assert np.allclose(np.linalg.norm(m.vertices, axis=1), 1.0) and _outward(m, lambda c: 0.0)
        assert m.vertices.shape[0] == 10 * 4 ** level + 2  # Euler: V - E + F = 2
    assert M.icosphere(6, None).faces.shape[0] == 81920
    b = M.box([-1, 0, 2], [1, 3, 2.5], None)
    assert b.faces.shape == (12, 3) and b.vertices.shape == (8, 3) and (_edge_use(b.faces) == 2).all()
    assert _outward(b, lambda c: np.array([0.0, 1.5, 2.25]))
    t = M.torus(1.0, 0.25, 16, 8, None, smooth=True)
    assert t.faces.shape == (256, 3) and (_edge_use(t.faces) == 2).all() and t.vertices.shape == (128, 3)
    ring = lambda c: np.stack([c[:, 0], 0 * c[:, 1], c[:, 2]], 1) / np.hypot(c[:, 0], c[:, 2])[:, None]  # noqa: E731
    assert _outward(t, ring) and np.allclose(np.linalg.norm(t.normals, axis=1), 1.0)
    q = M.quad([[0, 0, 0], [0, 0, 1], [1, 0, 1], [1, 0, 0]], None)
    assert q.faces.shape == (2, 3) and sorted(_edge_use(q.faces)) == [1, 1, 1, 1, 2]
    s = M.icosphere(1, None, smooth=True)
    assert np.array_equal(s.normals, s.vertices)
    for bad in (-1, 8, 1.5, True):
        with pytest.raises(ValueError, match="level"):
            M.icosphere(bad, None)
    with pytest.raises(ValueError, match="nu and nv"):
        M.torus(1.0, 0.2, 2, 8, None)


def test_placed_returns_a_copy():
    m = M.icosphere(0, "s", smooth=True)
    p = m.placed(scale=0.5, translation=(1, 2, 3))
    assert p is not m and p.shader == "s" and np.array_equal(p.faces, m.faces) and np.array_equal(p.normals, m.normals)
    assert np.array_equal(p.vertices, m.vertices * 0.5 + np.array([1.0, 2.0, 3.0]))
    assert np.allclose(np.linalg.norm(m.vertices, axis=1), 1.0)  # the original is untouched
    assert np.array_equal(m.placed().vertices, m.vertices)


# ---- the refusals of the table --------------------------------------------------------------------------------

def _mesh(vertices=((0, 0, 0), (1, 0, 0), (0, 1, 0)), faces=((0, 1, 2),), normals=None, sh=None):
    from python_ray_tracer_amd.infrastructure.hip import HipRGBColor, HipShader, Texture

    return TriangleMesh(vertices, faces, sh or HipShader(*GAINS, Texture(HipRGBColor(1, 0, 0))), normals)


def test_mesh_table_refuses():
    from python_ray_tracer_amd.infrastructure.hip import HipShader, ImageTexture

    nan = float("nan")
    for mesh, what in ((_mesh(vertices=((0, 0, 0), (1, 0, nan), (0, 1, 0))), "not finite"),
                       (_mesh(vertices=((0, 0, 0), (1, 0, np.inf), (0, 1, 0))), "not finite"),
                       (_mesh(faces=((0, 1, 3),)), "face index"), (_mesh(faces=((0, -1, 2),)), "face index"),
                       (_mesh(faces=np.zeros((0, 3), dtype=int)), "no faces"),
                       (_mesh(faces=((0, 1, 1),)), "degenerate"),
                       (_mesh(vertices=((0, 0, 0), (1, 0, 0), (2, 0, 0))), "degenerate"),
                       (_mesh(normals=((0, 0, 1), (0, 0, 1))), "normals must be"),
                       (_mesh(normals=((0, 0, 1), (0, 0, 1), (0, nan, 1))), "normal is not finite"),
                       (_mesh(vertices=((0, 0), (1, 0), (0, 1))), "vertices must be"),
                       (_mesh(faces=((0, 1, 2, 0),)), "faces must be")):
        with pytest.raises(ValueError, match=what):
            M.mesh_table([mesh])
    glassy = _mesh()
    glassy.shader.transmission_gain = 0.5
    with pytest.raises(ValueError, match="transmission_gain"):
        M.mesh_table([glassy])
    with pytest.raises(ValueError, match="ImageTexture"):
        M.mesh_table([_mesh(sh=HipShader(*GAINS, ImageTexture(np.ones((2, 2, 3)))))])
    for leaf in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_leaf"):
            M.mesh_table([_mesh()], leaf)
    with pytest.raises(ValueError, match="no TriangleMesh"):
        M.mesh_table([])
    # too many triangles: one triangle, F times (the check comes before any row is built)
    many = _mesh(faces=np.tile([[0, 1, 2]], ((1 << 20) + 1, 1)))
    with pytest.raises(ValueError, match="at most 1048576 triangles"):
        M.mesh_table([many])


def test_is_mesh_scene_and_check_bounces():
    scene = scenes.build_scene(quad_spec())
    assert M.is_mesh_scene(scene.shapes) and not M.is_mesh_scene(scene.shapes[:2]) and not M.is_mesh_scene([])
    assert [M.check_bounces(b) for b in (0, 3, 16)] == [0, 3, 16]
    for bad in (None, -1, 17, 2.5, True):
        with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
            M.check_bounces(bad)


# ---- the table and its tree -----------------------------------------------------------------------------------

def _parts(table):
    T, nm, N = (int(table[i]) for i in (M.MH_NTRI, M.MH_NMESH, M.MH_NNODES))
    rows = table[int(table[M.MH_TRIS]):][:T * M.TRI_WORDS].reshape(T, M.TRI_WORDS)
    mats = table[int(table[M.MH_MATS]):][:nm * L.MAT_WORDS].reshape(nm, L.MAT_WORDS)
    nodes = table[int(table[M.MH_NODES]):][:N * L.NODE_WORDS].reshape(N, L.NODE_WORDS)
    return rows, mats, nodes


@pytest.mark.parametrize("max_leaf", [1, 2, 4, 8, None])
@pytest.mark.parametrize("key", ["readme_mesh", "ico2_flat", "mesh_only"])
def test_table_invariants(key, max_leaf):
    spec = CASES[key]()
    shapes = scenes.build_scene(spec).shapes
    table = M.mesh_table(shapes, max_leaf)
    M.check_table(table)
    assert not table.flags.writeable and M.mesh_table(shapes, max_leaf) is table  # cached by content
    rows, mats, nodes = _parts(table)
    T, N = rows.shape[0], nodes.shape[0]
    g = R.group_of(spec)
    assert T == g.v0.shape[0] and mats.shape[0] == len(spec["meshes"])
    # the rows are the group's triangles, each once, with their numbers
    num = rows[:, M.T_NUM].astype(int)
    assert sorted(num) == list(range(T))
    for a, b in ((g.v0, M.T_V0), (g.e1, M.T_E1), (g.e2, M.T_E2), (g.ng, M.T_NG), (g.n0, M.T_N0), (g.n1, M.T_N1),
                 (g.n2, M.T_N2)):
        assert np.array_equal(rows[:, b:b + 3], a[num])
    assert np.array_equal(rows[:, M.T_MESH], g.mesh[num]) and np.array_equal(rows[:, M.T_SMOOTH] != 0, g.smooth[num])
    assert np.allclose(np.linalg.norm(rows[:, M.T_NG:M.T_NG + 3], axis=1), 1.0, atol=1e-15)
    # every triangle is in exactly one leaf, inside its leaf's box
    first, cnt, skip = (nodes[:, i].astype(int) for i in (L.N_FIRST, L.N_COUNT, L.N_SKIP))
    lo, hi = nodes[:, L.N_LOX:L.N_LOZ + 1], nodes[:, L.N_HIX:L.N_HIZ + 1]
    seen = np.zeros(T, dtype=int)
    for i in np.nonzero(cnt)[0]:
        assert cnt[i] <= (T if max_leaf is None else max_leaf)
        seen[first[i]:first[i] + cnt[i]] += 1
        r = rows[first[i]:first[i] + cnt[i]]
        corners = np.concatenate([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9]])
        assert (corners >= lo[i]).all() and (corners <= hi[i]).all()
    assert (seen == 1).all()
    if max_leaf is None:
        assert N == 1 and cnt[0] == T
    # depth first with skip links: the nodes after i and before skip[i] are its subtree, inside its box;
    # a skip link lands on the next sibling subtree or on the end
    assert skip[0] == N and (skip > np.arange(N)).all() and (skip <= N).all()
    for i in range(N):
        sub = slice(i + 1, skip[i])
        assert (lo[sub] >= lo[i]).all() and (hi[sub] <= hi[i]).all() and (skip[sub] <= skip[i]).all()
        if cnt[i] == 0:  # an inner node: two children, the second where the first one's subtree ends
            assert skip[i] > i + 2 and skip[skip[i + 1]] == skip[i]
        else:
            assert skip[i] == i + 1
    assert (nodes[:, L.N_MARGIN] >= M.MARGIN).all()
    far = (np.maximum(np.abs(lo), np.abs(hi)) ** 2).sum(axis=1)
    assert np.array_equal(nodes[:, L.N_MARGIN], M.MARGIN * (1.0 + far))


def test_check_table_refuses_a_header_that_does_not_fit():
    table = table_of(quad_spec())
    M.check_table(table)
    for word, value in ((M.MH_MAGIC, 1.0), (M.MH_NTRI, 1e6), (M.MH_NTRI, 0.0), (M.MH_NNODES, 99.0), (M.MH_WORDS, 5.0),
                        (M.MH_NODES, float(table.size)), (M.MH_TRIS, 0.0), (M.MH_NMESH, 0.0)):
        bad = table.copy()
        bad[word] = value
        with pytest.raises(ValueError, match="mesh table"):
            M.check_table(bad)
    with pytest.raises(ValueError, match="mesh table"):
        M.check_table(table[:-1])


# ---- the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 3])
def test_restatement_is_the_lights_restatement_where_no_triangle_is_in_sight(cap):
    """A triangle behind the camera takes part in nothing: the frame is tests/lights_ref.py's, bit for bit."""
    spec = scenes.readme_spec(W, H)
    want = lights_ref.render(spec, cap, table=R.table_of(spec))
    spec["meshes"] = [{"kind": "triangles", "vertices": [[0, 0, -50], [1, 0, -50], [0, 1, -50]], "faces": [[0, 1, 2]],
                       "shader": shader()}]
    assert np.array_equal(R.render(spec, cap), want)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", sorted(CASES))
def test_pruning_changes_no_frame(key, cap):
    spec, want, _ = frame(key, cap)
    for leaf in (1, 4):
        assert np.array_equal(R.render(spec, cap, prune=R.Pruner(table_of(spec, leaf))), want), leaf


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("key", sorted(CASES))
def test_no_pixel_of_a_gpu_case_sits_on_a_quantisation_step(key, cap):
    assert step_distance(frame(key, cap)[1]) > 1e-9


def test_preconditions_of_the_gpu_cases():
    c = frame("quad")[2]
    assert c.tri_primary > 300 and c.sphere_shadows_tri > 0 and c.sphere_to_tri > 0 and c.tri_to_sphere > 0
    for key in ("ico1_flat", "ico1_smooth", "ico2_flat", "ico2_smooth"):
        c = frame(key)[2]
        assert c.tri_primary > 20 and c.sphere_to_tri > 0 and c.tri_to_sphere > 0 and c.tri_shadows_sphere > 0, key
        assert (c.smooth_hits > 0) == key.endswith("smooth"), key
    assert len(CASES["ico1_flat"]()["meshes"]) == 1 and R.group_of(CASES["ico2_flat"]()).v0.shape[0] == 320
    assert R.group_of(CASES["ico1_smooth"]()).v0.shape[0] == 80
    c = frame("torus")[2]
    assert R.group_of(CASES["torus"]()).v0.shape[0] == 256 and c.self_shadow > 0 and c.tri_shadows_sphere > 0
    c = frame("mesh_only")[2]
    assert not CASES["mesh_only"]()["spheres"] and c.tri_primary > 300 and c.self_shadow > 0 and c.tri_to_sphere == 0
    c = frame("two_lights")[2]
    assert R.table_of(CASES["two_lights"]()).shape == (3, 6) and c.tri_primary > 300 and c.smooth_hits > 0
    c = frame("tree17")[2]
    assert len(CASES["tree17"]()["spheres"]) == 17 and c.tri_primary > 0 and c.tri_shadows_sphere + c.sphere_shadows_tri > 0
    for key in ("1x1", "7x5", "67x5"):
        assert frame(key)[2].rays > 0
    assert frame("7x5")[2].tri_primary > 0 and frame("67x5")[2].tri_primary > 0
    # the frames of the permutation test: no two triangles at one distance
    assert frame("ico2_flat")[2].tri_ties == 0 and frame("ico2_smooth")[2].tri_ties == 0
    # at cap 0 nothing is reflected
    assert frame("quad", 0)[2].rays == W * H


def test_rows_of_the_restatement_are_the_rows_of_the_frame():
    spec, want, _ = frame("readme_mesh")
    rows = [5, 26, 0]
    assert np.array_equal(R.render(spec, 3, rows=rows), want.reshape(3, H, W)[:, rows].reshape(3, -1))


def test_triangle_mesh_intersect_agrees_with_the_restatement():
    from python_ray_tracer_amd.infrastructure.hip import HipVector3D

    spec = ico_spec(2, False)
    mesh = scenes.build_scene(spec).shapes[-1]
    g = R.group_of(spec)
    osc = O.scene_from_spec(spec)
    d = O.ray_directions(osc.cam, W, H)
    t = mesh.intersect(HipVector3D(*osc.cam), HipVector3D(*d))
    want = R.nearest_triangle(g, *osc.cam, *d)[0]
    assert t.shape == (W * H,) and np.array_equal(t, want) and 20 < (t != M.FARAWAY).sum() < W * H
    one = mesh.intersect(HipVector3D(-0.05, 0.0, -2.0), HipVector3D(0.0, 0.0, 1.0))
    assert one.shape == (1,) and 3.4 < one[0] < 3.6
    assert mesh.diffusecolor(HipVector3D(0.0, 0.0, 0.0)).components() == (0.2, 0.6, 1.0)


# ---- explicit rays: exact cases ---------------------------------------------------------------------------------

def exact_spec(meshes, spheres=()):
    """A scene of dyadic numbers: every quantity of the rays below is exact."""
    return {"spheres": list(spheres), "meshes": meshes,
            "lights": [{"kind": "point", "position": [-2.0, 4.0, -1.0]},
                       {"kind": "dome", "intensity": 0.125, "color": [1, 1, 1]}],
            "camera": {"position": [0.0, 0.0, -2.0], "width": 2, "height": 2}}


def exact_cases():
    """name -> (spec, origins [3, n], directions [3, n], what the group's t must be per ray or None)."""
    sh = shader((0.5, 0.25, 1.0))
    fan = [[0, 0, 2]] + [[np.cos(a), np.sin(a), 2] for a in np.arange(6) * (np.pi / 3)]
    z = lambda *rays: np.array(rays, dtype=np.float64).T  # noqa: E731
    cases = {
        # the interior of the edge both triangles of a quad share: one hit, shaded once
        "shared_edge": (exact_spec([{"kind": "quad", "corners": [[-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2]],
                                     "shader": sh}]),
                        z([0, 0, -2], [0.5, 0.5, -2], [-0.25, -0.25, -2]), z([0, 0, 1], [0, 0, 1], [0, 0, 1]), [4, 4, 4]),
        # a vertex that six triangles share
        "shared_vertex": (exact_spec([{"kind": "triangles", "vertices": fan,
                                       "faces": [[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)], "shader": sh}]),
                          z([0, 0, -2]), z([0, 0, 1]), [4]),
        # a ray in the triangle's plane (det == 0), one that starts on it (t == 0) and one that leaves it
        "in_plane_and_on_it": (exact_spec([{"kind": "triangles", "vertices": [[-1, -1, 2], [1, -1, 2], [0, 1, 2]],
                                            "faces": [[0, 1, 2]], "shader": sh}]),
                               z([-4, 0, 2], [0, 0, 2], [0, 0, 2], [0, 0, 1]), z([1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 0, 1]),
                               [M.FARAWAY, M.FARAWAY, M.FARAWAY, 1]),
        # a triangle beyond FARAWAY, and a huge one just before it
        "faraway": (exact_spec([{"kind": "triangles", "vertices": [[-1e39, -1e39, 2e39], [1e39, -1e39, 2e39], [0, 1e39, 2e39]],
                                 "faces": [[0, 1, 2]], "shader": sh}]),
                    z([0, 0, -2]), z([0, 0, 1]), [M.FARAWAY]),
        # a sphere and a triangle at t = 4 exactly: both shade, the sphere first
        "tie": (exact_spec([{"kind": "triangles", "vertices": [[-1, -1, 2], [1, -1, 2], [0, 1, 2]], "faces": [[0, 1, 2]],
                             "shader": sh}],
                           [{"center": [0, 0, 3], "radius": 1.0, "shader": shader((1.0, 0.5, 0.25))}]),
                z([0, 0, -2]), z([0, 0, 1]), [4]),
    }
    return cases


@pytest.mark.parametrize("name", sorted(exact_cases()))
def test_exact_rays_of_the_restatement(name):
    spec, o, d, want_t = exact_cases()[name]
    g = R.group_of(spec)
    t, num, _, _, share = R.nearest_triangle(g, *o, *d)
    assert np.array_equal(t, np.array(want_t, dtype=np.float64)), t
    c = R.Counts()
    col = R.trace_rays(spec, tuple(o), tuple(d), 3, c)
    assert np.isfinite(col).all()
    if name == "shared_edge":
        assert list(share) == [2, 2, 2] and list(num) == [0, 0, 0] and c.tri_ties == 3
        # shaded once: the colour of the same hit on the first triangle alone
        one = copy.deepcopy(spec)
        one["meshes"][0] = {"kind": "triangles", "vertices": [[-1, -1, 2], [-1, 1, 2], [1, 1, 2]], "faces": [[0, 1, 2]],
                            "shader": one["meshes"][0]["shader"]}
        assert np.array_equal(R.trace_rays(one, tuple(o), tuple(d), 3), col)
    if name == "shared_vertex":
        assert share[0] == 6 and num[0] == 0
    if name == "in_plane_and_on_it":
        assert not col[:, :3].any() and col[:, 3].all()
    if name == "faraway":
        assert not col.any()
    if name == "tie":
        assert c.ties == 1 and O.intersect(O.scene_from_spec(spec).spheres[0], 0.0, 0.0, -2.0, *d)[0] == 4.0
        # both shade: at least twice the ambient term
        assert (col >= 2 * 0.004).all()


# ---- the C ABI and the op without a GPU ---------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entries():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    for name in ("rtx_trace_mesh", "rtx_mesh_workspace_bytes"):
        assert re.search(rf"\b{name}\(", text) and name in L.EXPORTS and hasattr(L.load(), name)
    assert "RTX_MAX_TRIANGLES = 1 << 20" in text and M.MAX_TRIANGLES == L.MAX_TRIANGLES == 1 << 20
    assert f"RTX_MESH_MAGIC {M.MAGIC}" in text and f"RTX_TRI_WORDS = {M.TRI_WORDS}" in text
    assert f"RTX_MESH_HDR_WORDS = {M.HDR_WORDS}" in text and M.MAX_BOUNCES == L.MESH_MAX_BOUNCES == 16
    for name in ("V0", "E1", "E2", "NG", "MESH", "SMOOTH", "N0", "N1", "N2", "NUM"):
        assert re.search(rf"RTX_T_{name} = {getattr(M, 'T_' + name)}\b", text), name
    order = re.search(r"enum \{ RTX_MH_MAGIC = 0, (.*?) \};", text).group(1).replace("RTX_", "").split(", ")
    assert [getattr(M, n) for n in order] == list(range(1, 8))


def test_workspace_is_bounded_by_the_pool_of_workers():
    ws = L.load().rtx_mesh_workspace_bytes
    for B in range(17):
        per = (2 * B + 2) * 10 * 8  # a worker's stack: 2B + 2 pending rays of 10 words
        assert ws(1, B) == L.WS_HDR_BYTES + 64 * per and ws(64, B) == ws(1, B) and ws(65, B) == L.WS_HDR_BYTES + 128 * per
        assert ws(0, B) == L.WS_HDR_BYTES
        big = ws(1 << 40, B)
        assert big == ws(1 << 24, B) and big - L.WS_HDR_BYTES <= 256 << 20  # does not grow with the frame
    assert ws(10, -1) == 0 and ws(10, 17) == 0 and ws(-1, 3) == 0


def test_argument_checks_need_no_gpu():
    """Every bad argument returns an error code with a message before any HIP call, and zero rays
    return RTX_OK without a launch: the pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)

    def call(scene=p, S=3, mesh=p, words=1000, table=p, nl=2, origins=p, stride=0, dirs=p, n=8, B=3, out=p, kind=1, ws=p,
             ws_bytes=1 << 30):
        return lib.rtx_trace_mesh(scene, S, mesh, words, table, nl, origins, stride, dirs, n, B, out, kind, ws, ws_bytes,
                                  None)

    assert call(scene=None) == -1 and b"null scene" in lib.rtx_last_error()
    assert call(mesh=None) == -1 and b"null mesh" in lib.rtx_last_error()
    assert call(table=None) == -1 and b"null lights" in lib.rtx_last_error()
    for kw in ({"origins": None}, {"dirs": None}):
        assert call(**kw) == -1 and b"null ray" in lib.rtx_last_error(), kw
    assert call(out=None) == -1 and b"null output" in lib.rtx_last_error()
    assert call(ws=None) == -1 and b"null workspace" in lib.rtx_last_error()
    for S in (-1, 1025):
        assert call(S=S) == -1 and b"n_spheres" in lib.rtx_last_error(), S
    for words in (0, 15, -1, 1 << 31):
        assert call(words=words) == -1 and b"mesh_words" in lib.rtx_last_error(), words
    for nl in (0, -1, 9):
        assert call(nl=nl) == -1 and b"n_lights" in lib.rtx_last_error(), nl
    for B in (-1, 17, 333):
        assert call(B=B) == -1 and b"max_bounces" in lib.rtx_last_error(), B
    for kind in (-1, 3):
        assert call(kind=kind) == -1 and b"out_kind" in lib.rtx_last_error(), kind
    assert call(n=-1) == -1 and b"negative" in lib.rtx_last_error()
    assert call(stride=5) == -1 and b"origin_stride" in lib.rtx_last_error()
    need = lib.rtx_mesh_workspace_bytes(8, 3)
    assert call(ws_bytes=need - 1) == -3 and b"workspace too small" in lib.rtx_last_error()
    # zero rays: nothing to launch; a scene of no sphere is accepted
    assert call(n=0) == 0 and call(n=0, S=0, B=0, kind=2, ws_bytes=L.WS_HDR_BYTES) == 0 and call(n=0, B=16, nl=8) == 0


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "trace_mesh" in ops.OPS
    assert str(torch.ops.rt.trace_mesh.default._schema) == \
        ("rt::trace_mesh(Tensor scene, int n_spheres, Tensor mesh, Tensor lights, Tensor origins, Tensor dirs, "
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
        out = torch.ops.rt.trace_mesh(*args(kind=kind))
        assert out.device.type == "meta" and tuple(out.shape) == shape and out.dtype == dtype
    out = torch.ops.rt.trace_mesh(*args(S=0, scene=torch.zeros(L.HDR_WORDS, dtype=torch.float64, device="meta"), B=16))
    assert tuple(out.shape) == (3, n)
    meta = dict(device="meta", dtype=torch.float64)
    for bad, what in (({"mesh": torch.zeros(15, **meta)}, "mesh must be"), ({"mesh": torch.zeros(5, 100, **meta)}, "mesh must be"),
                      ({"mesh": torch.zeros(500, device="meta", dtype=torch.float32)}, "mesh must be"),
                      ({"lights": torch.zeros(3, 5, **meta)}, "lights"), ({"lights": torch.zeros(9, 6, **meta)}, "lights"),
                      ({"dirs": torch.zeros(n, 3, **meta)}, "dirs"), ({"origins": torch.zeros(3, n + 1, **meta)}, "origins"),
                      ({"B": -1}, "max_bounces"), ({"B": 17}, "max_bounces"), ({"kind": 3}, "out_kind"),
                      ({"S": -1}, "n_spheres"), ({"S": 4}, "too short"), ({"scene": torch.zeros(2, 200, **meta)}, "1-D")):
        with pytest.raises(RuntimeError, match=what):
            torch.ops.rt.trace_mesh(*args(**bad))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_mesh(*args(dev="cpu"))


# ---- the renderer without a GPU -------------------------------------------------------------------------------

class _NoDevice:
    """Stands where the renderer keeps its library and its device: any use of either fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after a use of the library or the device ({name})")


def _renderer(monkeypatch, **kw):
    """A HipRenderer that never saw its constructor (which needs the GPU), with the fields the host
    refusals read; every torch.cuda call and every use of the library or the device fails."""
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer

    def no_gpu(*a, **k):
        raise AssertionError("the refusal came after a torch.cuda call")

    for name in ("current_device", "set_device", "current_stream", "is_current_stream_capturing"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    r = object.__new__(HipRenderer)
    fields = dict(_lib=_NoDevice(), device=_NoDevice(), max_bounces=3, samples=1, adaptive=False, color_dtype=torch.float64,
                  mesh_max_leaf=4, _light_tables=_NoDevice(), _glass_tables=_NoDevice(), _mesh_tables=_NoDevice(),
                  _scene_cache=_NoDevice())
    fields.update(kw)
    r.__dict__.update(fields)
    return r


def test_every_refusal_of_the_renderer_comes_before_any_gpu_use(monkeypatch):
    from python_ray_tracer_amd.domain import EnvironmentLight
    from python_ray_tracer_amd.infrastructure.hip import HipShader, HipVector3D, ImageTexture

    scene = scenes.build_scene(scenes.mesh_spec(W, H, 1))
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    r = _renderer(monkeypatch)
    o = scene.camera.position
    d = HipVector3D(np.array([0.0]), np.array([0.0]), np.array([1.0]))
    with pytest.raises(ValueError, match="render_batch.*TriangleMesh.*one by one"):
        r.render_batch([plain, scene])
    with pytest.raises(ValueError, match=r"submit_tiles.*TriangleMesh.*TileGather\(native=False\)"):
        r.submit_tiles(None, 0, scene, 1, 1, 0, None)
    with pytest.raises(ValueError, match="shade_hits.*TriangleMesh.*render the scene"):
        r.shade_hits(scene.shapes[0], scene, o, d, np.array([1.0]))
    with pytest.raises(ValueError, match="blob.*TriangleMesh.*packs the scene itself"):
        r.render_tile(scene, blob=torch.zeros(8, dtype=torch.float64), n_spheres=2)
    for name, call in (("render_aovs", r.render_aovs), ("render_occlusion", r.render_occlusion),
                       ("trace_aovs", lambda s: r.trace_aovs(o, d, s)),
                       ("trace_occlusion", lambda s: r.trace_occlusion(o, d, s))):
        with pytest.raises(ValueError, match=f"{name}.*TriangleMesh.*passes"):
            call(scene)
    for call in (r.render, r.render_tile, lambda s: r.raytrace_scene(o, d, s)):
        for cap in (None, 17):
            r.max_bounces = cap
            with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
                call(scene)
    r.max_bounces = 3
    r.adaptive, r.samples = True, 2
    with pytest.raises(ValueError, match="TriangleMesh.*adaptive=False"):
        r.render(scene)
    with pytest.raises(ValueError, match="edge_mask.*TriangleMesh"):
        r.edge_mask(scene)
    r.adaptive, r.samples = False, 1
    for call in (r.render, lambda s: r.raytrace_scene(o, d, s)):
        glassy = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        glassy.shapes[0].shader.transmission_gain = 0.9  # a glass sphere in a mesh scene
        with pytest.raises(ValueError, match="TriangleMesh and a transmissive shader"):
            call(glassy)
        env = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        env.lights.append(EnvironmentLight(np.ones((2, 4, 3))))
        with pytest.raises(ValueError, match="TriangleMesh and an EnvironmentLight"):
            call(env)
        textured = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        textured.shapes[-1].shader = HipShader(*GAINS, ImageTexture(np.ones((2, 2, 3))))
        with pytest.raises(ValueError, match="ImageTexture"):
            call(textured)
        bad = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        bad.shapes[-1].vertices[0, 0] = np.inf
        with pytest.raises(ValueError, match="not finite"):
            call(bad)
    # a scene without a mesh never asks for a table
    assert r._mesh_table(plain, "render") is None


class _CountingWorkspace(torch.Tensor):
    """A CPU workspace that counts the reads of its header (``ws[:8]``: the status word's read-back)."""

    reads = 0

    def __getitem__(self, index):
        if index == slice(None, 8):
            type(self).reads += 1
        return super().__getitem__(index)


_STACK_ROUTES = {  # route -> (library entry, the clean-key record of its kernel, pending rays at max_bounces=3)
    "glass": ("rtx_trace_glass", "_glass_clean", 16),
    "lights": ("rtx_trace_lights", "_lights_clean", 8),
    "env_lights": ("rtx_trace_lights_env", "_lights_clean", 8),
    "env_glass": ("rtx_trace_glass_env", "_glass_clean", 16),
    "mesh": ("rtx_trace_mesh", "_mesh_clean", 8),
    "mesh_uv": ("rtx_trace_mesh_uv", "_mesh_clean", 8),
}


@pytest.mark.parametrize("route", sorted(_STACK_ROUTES))
def test_an_overflowed_stack_raises_recursion_error(monkeypatch, route):
    """The status word's host handling, without a kernel, on every route to a kernel with a stack of pending
    rays: the trace method reads the status once, raises RecursionError for the overflow flag (4 B + 4 pending
    rays for the glass kernels, 2 B + 2 for the others) and clears it; a clean render of a key is remembered, in
    the record of the kernel underneath, and not read back again; a failed one is not remembered."""
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer, base

    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    entry, record, pending = _STACK_ROUTES[route]
    calls = []

    class Lib:
        def __getattr__(self, name):
            if name.endswith("_workspace_bytes"):
                return lambda n, B: 64

            def call(*a):
                calls.append(name)
                return 0

            return call

    class Workspace(_CountingWorkspace):
        reads = 0

    r = object.__new__(HipRenderer)
    ws = torch.zeros(64, dtype=torch.uint8).as_subclass(Workspace)
    t = torch.zeros(16, dtype=torch.float64)
    r.__dict__.update(_lib=Lib(), device=torch.device("cpu"), max_bounces=3, _glass_ws=ws, _lights_ws=ws, _mesh_ws=ws,
                      _glass_clean={}, _lights_clean={}, _mesh_clean={}, _mesh_tables={"k": t},
                      _light_tables={b"l": torch.zeros(1, 6, dtype=torch.float64)},
                      _env_images={"d": torch.zeros(2, 4, 3, dtype=torch.float64)}, _graph_pins={}, _stream=lambda: 0)
    glass_table, lights_table = base._GlassTable(t, b"g"), base._LightsTable(None, b"l")
    env = base._EnvLight(types.SimpleNamespace(digest="d", texels=None), (1.0, 1.0, 1.0), 0.0)
    table, trace = {
        "glass": (glass_table, r._trace_glass),
        "lights": (lights_table, r._trace_lights),
        "env_lights": (base._EnvTable(env, lights_table, ("d", b"l")), r._trace_env),
        "env_glass": (base._EnvTable(env, glass_table, ("d", b"g")), r._trace_env),
        "mesh": (base._MeshTable(None, None, ("k", b"l")), r._trace_mesh),
        "mesh_uv": (base._MeshTable(None, None, ("k", b"l"), True), r._trace_mesh),
    }[route]
    assert r._tracer(table) == trace
    status = ws[:8].view(torch.int32)  # (not a counted read: the count starts below)
    Workspace.reads = 0
    trace(t, 0, table, 0, 0, t, 4, t, 1, key="frame")
    trace(t, 0, table, 0, 0, t, 4, t, 1, key="frame")  # clean before: no read-back
    assert calls == [entry, entry] and Workspace.reads == 1
    records = {name: dict(getattr(r, name)) for name in ("_glass_clean", "_lights_clean", "_mesh_clean")}
    assert records.pop(record) == {"frame": True} and not any(records.values())
    status[1] = L.ST_STACK_OVERFLOW
    with pytest.raises(RecursionError, match=f"more than {pending} pending rays at max_bounces=3"):
        trace(t, 0, table, 0, 0, t, 4, t, 1, key="other")
    assert calls == [entry] * 3 and Workspace.reads == 2
    assert int(status[1]) == 0 and "other" not in getattr(r, record)  # the sticky flag is cleared, nothing remembered


def test_the_new_methods_live_in_the_base_class():
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer, base

    assert base._MeshScenes in HipRenderer.__mro__
    for name in ("_mesh_table", "_mesh_workspace", "_trace_mesh"):
        assert name in vars(base._MeshScenes) and name not in vars(HipRenderer)


def test_scene_key_packs_the_spheres_alone():
    from python_ray_tracer_amd.infrastructure.hip.scene_pack import pack_scene, scene_key

    spec = scenes.mesh_spec(W, H, 1)
    with_mesh = scenes.build_scene(spec)
    spec.pop("meshes")
    without = scenes.build_scene(spec)
    assert scene_key(with_mesh) == scene_key(without) and np.array_equal(pack_scene(with_mesh), pack_scene(without))
    only = scenes.build_scene(mesh_only_spec())
    blob = pack_scene(only)
    assert blob.shape == (L.HDR_WORDS,) and blob[L.H_NSPH] == 0 and blob[L.H_MAGIC] == L.MAGIC
    only.shapes = []
    with pytest.raises(TypeError, match="empty iterable"):  # a scene of no shape at all: as before
        scene_key(only)


def test_specs_and_build_scene():
    spec = scenes.mesh_spec(64, 36)
    assert [m["kind"] for m in spec["meshes"]] == ["quad", "icosphere", "torus"] and len(spec["spheres"]) == 2
    assert spec["meshes"][0]["shader"]["texture"]["kind"] == "checker"
    scene = scenes.build_scene(spec)
    assert [type(s).__name__ for s in scene.shapes] == ["HipSphere", "HipSphere"] + ["TriangleMesh"] * 3
    assert [len(s.faces) for s in scene.shapes[2:]] == [2, 320, 1024] and scene.shapes[3].normals is not None
    assert len(scenes.build_scene(scenes.mesh_spec(8, 8, 4)).shapes[3].faces) == 5120
    assert "meshes" not in scenes.readme_spec(8, 8)
    with pytest.raises(ValueError, match="unknown mesh kind"):
        scenes.build_scene({**spec, "meshes": [{"kind": "teapot", "shader": shader()}]})


def test_the_row_tile_gather_of_a_mesh_scene_goes_through_render_tile(monkeypatch):
    """render_image_pipeline on several ranks: tile_gather_for asks for the render_tile(into=) path, never the
    native plan (submit_tiles refuses a mesh scene); a plain scene keeps the default."""
    import torch.distributed as dist

    from python_ray_tracer_amd import distributed

    made = []

    class Gather:
        def __init__(self, renderer, width, height, **kw):
            made.append(kw["native"])

    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(distributed, "TileGather", Gather)
    distributed.tile_gather_for(types.SimpleNamespace(), scenes.build_scene(quad_spec()))
    distributed.tile_gather_for(types.SimpleNamespace(), scenes.build_scene(scenes.readme_spec(W, H)))
    assert made == [False, None]
