"""Primary-hit render passes of mesh scenes (rtx_mesh_aovs, HipRenderer.render_mesh_aovs): what
needs no GPU. The restatement (tests/mesh_aov_ref.py) is pinned to tests/aov_ref.py where no triangle is in
sight and to ``mesh_ref.render`` through ``mesh_ref._shade``; the tree's emulated pruning changes none of its
frames; the cases tests/test_gpu_mesh_aov.py runs are built here, with what each of them must show asserted;
the renderer's refusals come before any use of the GPU; the C entry's and the op's argument checks."""

import copy
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.domain import Scene3D
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import aov_ref
from tests import mesh_aov_ref as A
from tests import mesh_ref as R
from tests.test_mesh_cpu import ico_spec, mesh_only_spec, shader
from tests.test_mesh_limits_cpu import TIE_LANES, edge_rays, tie_case

REPO = Path(__file__).resolve().parent.parent
W, H = 50, 22  # 1,100 rays: no multiple of 64 or 256, so the last wave is ragged
NAMES = A.PASSES


def lights_mesh_spec():
    """mesh_spec under the two extra coloured lights of scenes.lights_spec."""
    spec = scenes.mesh_spec(W, H, 1)
    spec["lights"] += copy.deepcopy(scenes.lights_spec(W, H)["lights"][-2:])
    return spec


FRAMES = {
    "mesh": lambda: scenes.mesh_spec(W, H, 1),
    "textured": lambda: scenes.textured_mesh_spec(W, H, 1, texels=scenes.uv_grid_texels(16, 16)),
    "lights": lights_mesh_spec,
    "mesh_only": mesh_only_spec,
}


def frame(key):
    """(spec, the restatement's passes of its whole frame), computed once and read-only."""
    return A.frame(key, FRAMES[key])


def interleaved_scene():
    """(scene, spec, shape_ids): mesh_spec's scene with its shapes as mesh, sphere, mesh, sphere, mesh, built
    from the Scene3D's own objects: the relative order of the spheres and of the meshes is the spec's."""
    spec = scenes.mesh_spec(W, H, 1)
    scene = scenes.build_scene(spec)
    sph = [s for s in scene.shapes if not isinstance(s, M.TriangleMesh)]
    msh = [s for s in scene.shapes if isinstance(s, M.TriangleMesh)]
    assert len(sph) == 2 and len(msh) == 3
    shapes = [msh[0], sph[0], msh[1], sph[1], msh[2]]
    return Scene3D(shapes, scene.lights, scene.camera), spec, M.shape_ids(shapes)


_cases: dict = {}


def tie_rays():
    """(spec, eye, directions [3, n], the restatement's passes): tests/test_mesh_limits_cpu.py's three coincident
    spheres and a triangle at t = 4, its frame's rays with the tie ray at TIE_LANES as well."""
    if "tie" not in _cases:
        spec, _, _, e = tie_case(3)[:4]
        eye = tuple(float(c) for c in spec["camera"]["position"])
        _cases["tie"] = (spec, eye, e, A.of_spec(spec, eye, e))
    return _cases["tie"]


ICO_AT, ICO_SCALE = (-0.05, 0.0, 1.9), 0.4


def ico_tie_rays():
    """(spec, origins [3, n], directions [3, n], the passes, the rays whose primary hit two or more triangles
    share, a wave of 64 of them with a miss at lane 31 and a sphere's hit at lane 63): rays at the vertices and
    the edges of the flat level-2 icosphere of tests/test_mesh_cpu.py's ico_spec."""
    if "ico" not in _cases:
        spec = ico_spec(2, False)
        o, d = edge_rays(spec, ICO_AT, ICO_SCALE, 14)
        a = A.of_spec(spec, o, d)
        share = R.nearest_triangle(R.group_of(spec), *o, *d)[4]
        shared = np.nonzero((a["triangle"] >= 0) & (share > 1))[0]
        miss = np.nonzero(a["id"] < 0)[0]
        sphere = np.nonzero((a["id"] >= 0) & (a["triangle"] < 0))[0]
        wave = np.resize(shared, 64)
        wave[31], wave[63] = miss[0], sphere[0]
        _cases["ico"] = (spec, o, d, a, shared, wave)
    return _cases["ico"]


def quad_shadow_spec(between: bool):
    """One sphere under a light, and a quad between the two (or moved far aside): only the quad can shadow."""
    x = 0.0 if between else 50.0
    return {"spheres": [{"center": [0, 0, 3], "radius": 1.0, "shader": shader((1.0, 0.5, 0.25))}],
            "meshes": [{"kind": "quad", "corners": [[x - 2, 5, 1], [x - 2, 5, 5], [x + 2, 5, 5], [x + 2, 5, 1]],
                        "shader": shader()}],
            "lights": [{"kind": "point", "position": [0.0, 10.0, 3.0]},
                       {"kind": "dome", "intensity": 0.125, "color": [1, 1, 1]}],
            "camera": {"position": [0.0, 1.0, -2.0], "width": 24, "height": 13}}


def deep_rays():
    """(spec, origins, directions, the passes): 512 incoherent rays, origins inside and outside the shapes,
    through a level-5 icosphere (20,480 of the scene's 20,736 triangles; 16,383 nodes at leaves of 4)."""
    if "deep" not in _cases:
        from tests.test_mesh_limits_cpu import PLACEMENTS, random_rays, spec_of

        c, s = PLACEMENTS["near"]
        spec = spec_of(5, c, s)
        o, d = random_rays(c, s, 512, 12)
        _cases["deep"] = (spec, o, d, A.of_spec(spec, o, d))
    return _cases["deep"]


def same(a: dict, b: dict, names=NAMES, what=""):
    for k in names:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


# ---- the restatement ------------------------------------------------------------------------------------------

def test_a_mesh_behind_the_camera_leaves_the_passes_of_the_spheres():
    spec = scenes.readme_spec(W, H)
    osc = O.scene_from_spec(spec)
    want = aov_ref.aovs(osc, *aov_ref.frame_rays(osc))
    spec["meshes"] = [{"kind": "icosphere", "level": 1, "scale": 0.5, "translation": [0.0, -20.0, -40.0], "shader": shader()}]
    got = A.of_spec(spec)
    assert int((want["id"] >= 0).sum()) > 400 and int((want["lit"] == 0).sum()) > 10
    same(got, want, aov_ref.PASSES)
    assert (got["triangle"] == -1).all() and not got["bary"].any()
    assert np.array_equal(got["geometric_normal"], got["normal"])


def test_shading_the_passes_gives_the_frame():
    """Every non-tie pixel of the frame: position, normal and Q from geometric_normal fed into
    mesh_ref._shade at cap 0 give mesh_ref.render(spec, max_bounces=0), difference exactly 0."""
    spec, a = frame("mesh")
    want = R.render(spec, max_bounces=0)
    scene, g, table = O.scene_from_spec(spec), R.group_of(spec), R.table_of(spec)
    S = len(scene.spheres)
    d = np.stack(O.ray_directions(scene.cam, scene.width, scene.height))
    got = np.zeros_like(want)
    assert (a["hits"] <= 1).all()  # (no tie in this frame: every pixel is compared)
    tri_mesh = np.where(a["triangle"] >= 0, g.mesh[np.maximum(a["triangle"], 0)], -1)
    groups = [(si, sp, -1, a["id"] == si) for si, sp in enumerate(scene.spheres)]
    groups += [(-1, mat, mi, tri_mesh == mi) for mi, mat in enumerate(g.mats)]
    seen = 0
    for si, mat, mi, sel in groups:
        idx = np.nonzero(sel)[0]
        assert idx.size > 0
        seen += idx.size
        P = tuple(a["position"][c, idx] for c in range(3))
        N = tuple(a["normal"][c, idx] for c in range(3))
        Q = tuple(a["position"][c, idx] + a["geometric_normal"][c, idx] * 0.0001 for c in range(3))
        V = O._norm(*(scene.cam[c] - P[c] for c in range(3)))
        part = R._shade(scene, g, table, si, mat, mi, P, N, Q, V, tuple(d[c, idx] for c in range(3)), 0, False, None, 0,
                        None)
        for c in range(3):
            got[c, idx] = part[c]
    assert seen == int((a["id"] >= 0).sum()) == 750 and S == 2
    assert np.array_equal(got, want)
    # the colour path sees a hit exactly where the passes do: a miss is black, a hit has the ambient term
    assert np.array_equal(a["id"] >= 0, (want != 0).any(axis=0))
    assert not want[:, a["id"] < 0].any() and want[:, a["id"] >= 0].max(axis=0).min() >= 0.004


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("key", sorted(FRAMES))
def test_pruning_changes_no_pass(key, leaf):
    spec, a = frame(key)
    table = M.mesh_table(scenes.build_scene(spec).shapes, leaf)
    got = A.of_spec(spec, prune=R.Pruner(table))
    same(got, a, ("depth", "triangle", "lit"), (key, leaf))
    same(got, a, NAMES, (key, leaf))


def test_pruning_changes_no_pass_of_the_ray_cases():
    for leaf in (1, 4):
        spec, eye, e, a = tie_rays()
        same(A.of_spec(spec, eye, e, prune=R.Pruner(M.mesh_table(scenes.build_scene(spec).shapes, leaf))), a)
        spec, o, d, a = ico_tie_rays()[:4]
        same(A.of_spec(spec, o, d, prune=R.Pruner(M.mesh_table(scenes.build_scene(spec).shapes, leaf))), a)


# ---- what the GPU cases must show ----------------------------------------------------------------------------

def test_preconditions_of_the_frames():
    spec, a = frame("mesh")
    S = len(spec["spheres"])
    tri = a["triangle"] >= 0
    assert a["depth"].shape == (W * H,) and (W * H) % 64 != 0
    assert int(tri.sum()) == 334 and [int((a["id"] == S + i).sum()) for i in range(3)] == [130, 105, 99]
    assert int(((a["id"] >= 0) & ~tri).sum()) == 416 and int((a["id"] < 0).sum()) == 350
    c = R.Counts()
    R.render(spec, 0, counts=c)
    assert (c.tri_primary, c.smooth_hits, c.sphere_shadows_tri, c.self_shadow) == (334, 204, 29, 9)
    assert c.ties == 0 and c.tri_ties == 0 and c.tri_shadows_sphere == 0 and (a["hits"] <= 1).all()
    assert int((tri & (a["lit"] == 0)).sum()) == 44 and not (~tri & (a["id"] >= 0) & (a["lit"] == 0)).any()
    g = R.group_of(spec)
    smooth = tri & g.smooth[np.maximum(a["triangle"], 0)]
    assert int(smooth.sum()) == 204
    assert (np.abs(a["normal"][:, smooth] - a["geometric_normal"][:, smooth]).max(axis=0) > 1e-3).sum() > 150
    assert np.array_equal(a["normal"][:, tri & ~smooth], a["geometric_normal"][:, tri & ~smooth])
    assert (a["depth"][a["id"] < 0] == O.FARAWAY).all() and set(np.unique(a["lit"])) == {0, 1}
    assert (a["bary"][:, tri] >= 0).all() and (a["bary"][:, tri].sum(axis=0) <= 1).all() and not a["bary"][:, ~tri].any()
    # the textured frame: the albedo of the image-textured meshes is the lookup's, not a constant
    tspec, t = frame("textured")
    for k in ("depth", "id", "triangle", "normal", "lit", "bary"):
        assert np.array_equal(t[k], a[k]), k
    on_image = (t["id"] == S) | (t["id"] == S + 2)
    assert int(on_image.sum()) == 130 + 99 and np.unique(t["albedo"][:, on_image], axis=1).shape[1] > 100
    assert np.array_equal(t["albedo"][:, ~on_image], a["albedo"][:, ~on_image])
    # three lights: more than a bit
    lspec, li = frame("lights")
    assert R.table_of(lspec).shape == (3, 6)
    values = set(int(v) for v in np.unique(li["lit"]))
    assert len(values) >= 3 and any(v & ~1 for v in values) and max(values) <= 7, values
    assert np.array_equal(li["lit"] & 1, a["lit"]) and np.array_equal(li["depth"], a["depth"])
    # meshes alone
    mspec, mo = frame("mesh_only")
    assert mspec["spheres"] == [] and int((mo["triangle"] >= 0).sum()) > 300 and ((mo["id"] >= 0) == (mo["triangle"] >= 0)).all()
    assert set(np.unique(mo["id"])) == {-1, 0, 1, 2} and 0 < int((mo["lit"] == 0).sum()) < int((mo["id"] >= 0).sum())


def test_preconditions_of_the_interleaved_scene():
    scene, spec, ids = interleaved_scene()
    assert ids.tolist() == [1, 3, 0, 2, 4] and ids.dtype == np.int32
    a = A.of_spec(spec, shape_ids=ids)
    base = frame("mesh")[1]
    assert set(np.unique(a["id"])) == {-1, 0, 1, 2, 3, 4}
    assert np.array_equal(a["id"], np.where(base["id"] >= 0, ids[np.maximum(base["id"], 0)], -1))
    shape_index, face_index = M.triangle_faces(scene.shapes, a["triangle"])
    tri = a["triangle"] >= 0
    assert np.array_equal(shape_index[tri], a["id"][tri]) and (shape_index[~tri] == -1).all() and (face_index[~tri] == -1).all()
    g = R.group_of(spec)
    for si in (0, 2, 4):  # the face's own vertices give the row's v0 and the barycentric point the position
        sel = np.nonzero(shape_index == si)[0]
        mesh = scene.shapes[si]
        f = np.asarray(mesh.faces)[face_index[sel]]
        v = np.asarray(mesh.vertices, dtype=np.float64)
        assert np.array_equal(v[f[:, 0]], g.v0[a["triangle"][sel]])
        u, w = a["bary"][0, sel], a["bary"][1, sel]
        p = v[f[:, 0]].T * (1 - u - w) + v[f[:, 1]].T * u + v[f[:, 2]].T * w
        assert np.abs(p - a["position"][:, sel]).max() < 1e-9


def test_preconditions_of_the_ties_and_the_shadowed_sphere():
    spec, eye, e, a = tie_rays()
    for lane in TIE_LANES:
        assert (a["hits"][lane], a["id"][lane], a["triangle"][lane], a["depth"][lane]) == (4, 0, -1, 4.0)
        assert np.array_equal(a["normal"][:, lane], [0.0, 0.0, -1.0]) and not a["bary"][:, lane].any()
    assert int((a["hits"] == 4).sum()) == len(TIE_LANES) + 1 and int((a["triangle"] >= 0).sum()) > 10
    spec, o, d, a, shared, wave = ico_tie_rays()
    assert shared.size >= 64, shared.size
    g = R.group_of(spec)
    t, _, _ = R._tri_tests(g, np.arange(g.v0.shape[0]), *o[:, shared], *d[:, shared])
    assert ((t == a["depth"][shared]).sum(axis=0) >= 2).all()  # two or more triangles at the nearest distance ...
    assert np.array_equal(np.argmax(t == a["depth"][shared], axis=0), a["triangle"][shared])  # ... the lowest number
    assert (a["hits"][shared] == 1).all()
    assert a["triangle"][wave[0]] >= 0 and a["id"][wave[31]] == -1 and a["id"][wave[63]] >= 0 and a["triangle"][wave[63]] == -1
    # a sphere that only a triangle shadows
    near, far = A.of_spec(quad_shadow_spec(True)), A.of_spec(quad_shadow_spec(False))
    on = near["id"] == 0
    assert np.array_equal(on, far["id"] == 0) and int(on.sum()) > 30
    assert int((on & (near["lit"] == 0)).sum()) == 28 and (far["lit"][on] == 1).all()
    c = R.Counts()
    R.render(quad_shadow_spec(True), 0, counts=c)
    assert c.tri_shadows_sphere == 28
    # the deep tree
    spec, o, d, a = deep_rays()
    table = M.mesh_table(scenes.build_scene(spec).shapes, 4)
    assert int(table[M.MH_NTRI]) == 20736 and int(table[M.MH_NNODES]) == 16383
    assert int((a["triangle"] >= 0).sum()) > 100 and int((a["id"] == 0).sum()) > 5 and int((a["id"] < 0).sum()) > 50


# ---- the helper, the renderer without a GPU ------------------------------------------------------------------

def test_triangle_faces_and_shape_ids():
    scene, spec, ids = interleaved_scene()
    F = [len(scene.shapes[i].faces) for i in (0, 2, 4)]
    assert F == [2, 80, 1024]
    num = np.array([[-1, 0, 1], [2, 81, 82], [F[0] + F[1] + F[2] - 1, -1, 2 + 79]], dtype=np.int32)
    shape_index, face_index = M.triangle_faces(scene.shapes, num)
    assert shape_index.tolist() == [[-1, 0, 0], [2, 2, 4], [4, -1, 2]]
    assert face_index.tolist() == [[-1, 0, 1], [0, 79, 0], [1023, -1, 79]]
    assert shape_index.shape == num.shape and shape_index.dtype == face_index.dtype == np.int64
    for bad in ([sum(F)], [-2]):
        with pytest.raises(ValueError, match="outside"):
            M.triangle_faces(scene.shapes, np.array(bad))
    with pytest.raises(ValueError, match="integers"):
        M.triangle_faces(scene.shapes, np.array([0.5]))
    empty = M.triangle_faces(scene.shapes, np.zeros(0, dtype=np.int32))
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    assert M.shape_ids(plain.shapes).tolist() == [0, 1, 2]
    assert M.triangle_faces(plain.shapes, np.array([-1]))[0].tolist() == [-1]


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
                  _scene_cache=_NoDevice(), _mesh_shape_ids=_NoDevice())
    fields.update(kw)
    r.__dict__.update(fields)
    return r


def test_every_refusal_of_the_new_methods_comes_before_any_gpu_use(monkeypatch):
    from python_ray_tracer_amd.domain import EnvironmentLight
    from python_ray_tracer_amd.infrastructure import hip
    from python_ray_tracer_amd.infrastructure.hip import HipVector3D

    assert hip.MESH_AOV_NAMES == NAMES == tuple(L.MESH_AOV_PASSES)
    assert [L.MESH_AOV_PASSES[k] for k in NAMES] == [1 << b for b in range(10)] and L.MESH_AOV_ALL == 1023
    scene = scenes.build_scene(scenes.mesh_spec(W, H, 1))
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    r = _renderer(monkeypatch)
    o = scene.camera.position
    d = HipVector3D(np.array([0.0]), np.array([0.0]), np.array([1.0]))
    calls = (("render_mesh_aovs", lambda s, **kw: r.render_mesh_aovs(s, **kw)),
             ("trace_mesh_aovs", lambda s, **kw: r.trace_mesh_aovs(o, d, s, **kw)))
    for name, call in calls:
        with pytest.raises(ValueError, match=f"{name}.*no TriangleMesh.*render_aovs"):
            call(plain)
        for bad in ("uv", ("depth", "colour"), ()):
            with pytest.raises(ValueError, match="passes: need one or more of"):
                call(scene, passes=bad)
        r.samples = 2
        with pytest.raises(ValueError, match=f"{name}.*samples=2"):
            call(scene)
        r.samples = 1
        for cap in (None, 17):
            r.max_bounces = cap
            with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
                call(scene)
        r.max_bounces = 3
        glassy = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        glassy.shapes[0].shader.transmission_gain = 0.9
        with pytest.raises(ValueError, match=f"{name}.*TriangleMesh and a transmissive shader"):
            call(glassy)
        env = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        env.lights.append(EnvironmentLight(np.ones((2, 4, 3))))
        with pytest.raises(ValueError, match=f"{name}.*TriangleMesh and an EnvironmentLight"):
            call(env)
        bad = scenes.build_scene(scenes.mesh_spec(W, H, 1))
        bad.shapes[-1].vertices[0, 0] = np.inf
        with pytest.raises(ValueError, match="not finite"):
            call(bad)
        r.mesh_build = "device"
        with pytest.raises(ValueError, match="not finite"):
            call(bad)
        r.mesh_build = "host"
    lens = scenes.build_scene(scenes.with_camera(scenes.mesh_spec(W, H, 1), position=[2.5, 1.5, -1.5], target=[0, 0.0, 2.0],
                                                 fov=50.0, lens_radius=0.05, focus_distance=3.0))
    with pytest.raises(ValueError, match="lens_radius=0.05"):  # (as render_aovs refuses it: the camera's own check)
        r.render_mesh_aovs(lens)
    # the methods that refuse a mesh scene still do, and two of them say where its passes are
    for name, call in (("render_aovs", r.render_aovs), ("trace_aovs", lambda s: r.trace_aovs(o, d, s))):
        with pytest.raises(ValueError, match=f"{name}.*TriangleMesh.*passes.*render_mesh_aovs / trace_mesh_aovs"):
            call(scene)
    with pytest.raises(ValueError, match="render_occlusion.*TriangleMesh.*passes") as info:
        r.render_occlusion(scene)
    assert "render_mesh_aovs" not in str(info.value)


# ---- the C ABI and the op without a GPU ---------------------------------------------------------------------

def bad_argument_calls(lib):
    """Every RTX_E_ARG of rtx_mesh_aovs as (keyword arguments, a word of its message), and the call itself:
    returns before any HIP call, so the pointers are never dereferenced."""
    p = ctypes.c_void_p(4096)

    def call(scene=p, S=3, mesh=p, words=1000, table=p, nl=2, ids=p, origins=p, stride=0, dirs=p, n=8, outs=None):
        outs = [p] * 10 if outs is None else outs
        return lib.rtx_mesh_aovs(scene, S, mesh, words, table, nl, ids, origins, stride, dirs, n, *outs, None)

    bad = [({"scene": None}, b"null scene"), ({"mesh": None}, b"null mesh"), ({"table": None}, b"null lights"),
           ({"origins": None}, b"null ray"), ({"dirs": None}, b"null ray"), ({"outs": [None] * 10}, b"no pass requested"),
           ({"S": -1}, b"n_spheres"), ({"S": 1025}, b"n_spheres"), ({"words": 15}, b"mesh_words"), ({"words": -1}, b"mesh_words"),
           ({"words": 1 << 31}, b"mesh_words"), ({"nl": 0}, b"n_lights"), ({"nl": 9}, b"n_lights"), ({"n": -1}, b"negative"),
           ({"stride": 5}, b"origin_stride")]
    return call, bad


def test_header_library_and_argument_checks():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"int rtx_mesh_aovs\(const double\* scene, int n_spheres, const double\* mesh, int64_t mesh_words, "
                     r"const double\* lights,\s*int n_lights, const int32_t\* shape_ids, const double\* origins, "
                     r"int64_t origin_stride,\s*const double\* dirs, int64_t n, double\* depth, int32_t\* id, int32_t\* hits, "
                     r"double\* position,\s*double\* normal, double\* geometric_normal, double\* albedo, uint8_t\* lit, "
                     r"int32_t\* triangle,\s*double\* bary, void\* stream\);", text)
    for b, name in enumerate(NAMES):
        assert re.search(rf"RTX_MESH_AOV_{name.upper()} = {1 << b}\b", text), name
    assert "RTX_MESH_AOV_ALL = 1023" in text and "#define RTX_ABI_VERSION 3" in text or "RTX_ABI_VERSION = 3" in text
    i32, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert L._SIGS["rtx_mesh_aovs"] == (i32, [p, i32, p, i64, p, i32, p, p, i64, p, i64] + [p] * 11)
    assert "rtx_mesh_aovs" in L.EXPORTS and L.ABI_VERSION == 3
    lib = L.load()
    call, bad = bad_argument_calls(lib)
    for kw, word in bad:
        assert call(**kw) == -1 and word in lib.rtx_last_error(), kw
    p0 = ctypes.c_void_p(4096)
    assert call(n=0) == 0 and call(n=0, S=0, ids=None, nl=8, outs=[None] * 9 + [p0]) == 0  # zero rays: nothing is launched


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "mesh_aovs" in ops.OPS
    assert str(torch.ops.rt.mesh_aovs.default._schema) == \
        ("rt::mesh_aovs(Tensor scene, int n_spheres, Tensor mesh, Tensor lights, Tensor? shape_ids, Tensor origins, "
         "Tensor dirs, int passes, bool check=True) -> Tensor[]")
    S, n = 3, 77

    def args(dev="meta", **kw):
        a = dict(scene=torch.zeros(L.HDR_WORDS + S * (L.GEOM_WORDS + L.MAT_WORDS), dtype=torch.float64, device=dev),
                 S=S, mesh=torch.zeros(500, dtype=torch.float64, device=dev),
                 lights=torch.zeros(3, 6, dtype=torch.float64, device=dev),
                 ids=torch.zeros(S + 2, dtype=torch.int32, device=dev),
                 origins=torch.zeros(3, dtype=torch.float64, device=dev),
                 dirs=torch.zeros(3, n, dtype=torch.float64, device=dev), passes=L.MESH_AOV_ALL)
        a.update(kw)
        return tuple(a.values())

    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    kinds = [((n,), f64), ((n,), i32), ((n,), i32), ((3, n), f64), ((3, n), f64), ((3, n), f64), ((3, n), f64), ((n,), u8),
             ((n,), i32), ((2, n), f64)]
    for mask in (L.MESH_AOV_ALL, 1, 2 | 128, 512, 256 | 32 | 4, 64 | 16):
        out = torch.ops.rt.mesh_aovs(*args(passes=mask))
        want = [kinds[b] for b in range(10) if mask >> b & 1]
        assert [(tuple(t.shape), t.dtype) for t in out] == want and all(t.device.type == "meta" for t in out), mask
    out = torch.ops.rt.mesh_aovs(*args(S=0, scene=torch.zeros(L.HDR_WORDS, dtype=f64, device="meta"), ids=None, passes=3))
    assert [tuple(t.shape) for t in out] == [(n,), (n,)]
    meta = dict(device="meta", dtype=f64)
    for bad, what in (({"passes": 0}, "passes"), ({"passes": 1024}, "passes"), ({"mesh": torch.zeros(15, **meta)}, "mesh must be"),
                      ({"lights": torch.zeros(9, 6, **meta)}, "lights"), ({"dirs": torch.zeros(n, 3, **meta)}, "dirs"),
                      ({"origins": torch.zeros(3, n + 1, **meta)}, "origins"), ({"S": -1}, "n_spheres"), ({"S": 4}, "too short"),
                      ({"ids": torch.zeros(S, dtype=i32, device="meta")}, "shape_ids"),
                      ({"ids": torch.zeros(S + 2, dtype=torch.int64, device="meta")}, "shape_ids")):
        with pytest.raises(RuntimeError, match=what):
            torch.ops.rt.mesh_aovs(*args(**bad))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.mesh_aovs(*args(dev="cpu"))
