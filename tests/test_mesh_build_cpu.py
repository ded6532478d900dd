"""The device build of the mesh table without a GPU (HipRenderer.mesh_build = "device", rtx_mesh_build;
DESIGN.md §19): ``meshes.device_inputs`` against ``meshes.mesh_table``, the renderer's refusals, the
library's pure entries and argument checks, and the preconditions of the cases that
tests/test_gpu_mesh_build.py builds on the device, checked with the host builder so that each case holds
what it claims."""

import ctypes

import numpy as np
import pytest

from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.domain import TriangleMesh
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests.test_mesh_cpu import GAINS, H, W, _mesh, _renderer

LEAVES = (1, 2, 4, 8, None)


def _shader():
    from python_ray_tracer_amd.infrastructure.hip import HipRGBColor, HipShader, Texture

    return HipShader(*GAINS, Texture(HipRGBColor(1, 0, 0)))


def _meshes_of(spec):
    return [sh for sh in scenes.build_scene(spec).shapes if isinstance(sh, TriangleMesh)]


def quad_case():
    """T = 2: one node at every leaf size but 1."""
    return [M.quad([[-4, -0.5, -1], [-4, -0.5, 7], [4, -0.5, 7], [4, -0.5, -1]], _shader())]


def box_case():
    """A cube about the origin and a quad inside it whose corners' x are 0 and the smallest negative number: the
    centres' extents are equal on all three axes (the cut goes along x, the first), the cube's centres along
    x are -1, 0 and 1, the quad's (-5e-324 + 0) * 0.5 = -0.0: equal to 0, so the quad's triangles (numbers 12
    and 13) sort behind the cube's eight."""
    d = -5e-324
    return [M.box((-1, -1, -1), (1, 1, 1), _shader()),
            M.quad([[d, -0.5, -0.5], [0.0, 0.5, -0.5], [d, 0.5, 0.5], [0.0, -0.5, 0.5]], _shader())]


def strip_case():
    """A strip of 9 triangles: at leaf 4 the root's halves are 5 and 4 long, one cut, its neighbour not."""
    v = [(float(i), float(i % 2), 0.0) for i in range(11)]
    return [TriangleMesh(v, [(i, i + 1, i + 2) for i in range(9)], _shader())]


def twice_case():
    """One mesh twice: every centre is tied with its twin's, so the order is by triangle number."""
    ico = M.icosphere(0, _shader())
    return [ico, ico]


CASES = {"quad": quad_case, "box": box_case, "strip": strip_case, "twice": twice_case,
         "ico1": lambda: _meshes_of(scenes.mesh_spec(W, H, 1)),  # a flat quad, a smooth icosphere, a smooth torus
         "textured": lambda: _meshes_of(scenes.textured_mesh_spec(W, H))}  # a UV part, one texel block for two meshes


def _parts(table):
    T, nm, N = (int(table[i]) for i in (M.MH_NTRI, M.MH_NMESH, M.MH_NNODES))
    rows = table[int(table[M.MH_TRIS]):][:T * M.TRI_WORDS].reshape(T, M.TRI_WORDS)
    mats = table[int(table[M.MH_MATS]):][:nm * L.MAT_WORDS].reshape(nm, L.MAT_WORDS)
    nodes = table[int(table[M.MH_NODES]):][:N * L.NODE_WORDS].reshape(N, L.NODE_WORDS)
    return rows, mats, nodes


def _centres(shapes):
    """The triangles' centres in group order, as mesh_table_entry computes them."""
    rows = M.triangle_rows(shapes)[0]
    v0, e1, e2 = rows[:, M.T_V0:M.T_V0 + 3], rows[:, M.T_E1:M.T_E1 + 3], rows[:, M.T_E2:M.T_E2 + 3]
    corners = np.stack([v0, v0 + e1, v0 + e2])
    return (corners.min(axis=0) + corners.max(axis=0)) * 0.5


# ---- device_inputs against mesh_table -------------------------------------------------------------------------

@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", list(CASES))
def test_device_inputs_hold_what_the_host_table_holds(name, leaf):
    shapes = CASES[name]()
    table = M.mesh_table(shapes, leaf)
    d = M.device_inputs(shapes, leaf)
    sk = d.skeleton
    assert sk.dtype == np.float64 and sk.shape == table.shape
    assert np.array_equal(sk[:M.HDR_WORDS], table[:M.HDR_WORDS])
    rows, mats, nodes = _parts(table)
    srows, smats, snodes = _parts(sk)
    assert np.array_equal(smats, mats)
    for w in (L.N_FIRST, L.N_COUNT, L.N_SKIP):
        assert np.array_equal(snodes[:, w], nodes[:, w])
    M.check_table(sk)
    # what the build writes is zero
    assert not srows.any() and not snodes[:, [*range(L.N_LOX, L.N_HIZ + 1), L.N_MARGIN]].any()
    image = M.has_image(shapes)
    assert image == (name == "textured") == bool(table[M.MH_UVS]) == (d.uvs is not None)
    if image:
        at, x = int(table[M.MH_UVS]), int(table[M.MH_TEXELS])
        assert x < table.size and np.array_equal(sk[x:], table[x:]) and not sk[at:x].any()
    # the arrays: the rows in group order are the faces' vertices, meshes, normals and coordinates
    T = rows.shape[0]
    by_number = rows[np.argsort(rows[:, M.T_NUM])]
    assert d.faces.dtype == np.int32 and d.faces.shape == (T, 3) and d.tri_mesh.dtype == np.int32
    assert d.vertices.dtype == np.float64 and d.vertices.flags.c_contiguous and d.faces.flags.c_contiguous
    assert np.array_equal(d.vertices[d.faces[:, 0]], by_number[:, M.T_V0:M.T_V0 + 3])
    assert np.array_equal(d.vertices[d.faces[:, 1]] - d.vertices[d.faces[:, 0]], by_number[:, M.T_E1:M.T_E1 + 3])
    assert np.array_equal(d.tri_mesh, by_number[:, M.T_MESH])
    smooth = by_number[:, M.T_SMOOTH] == 1
    assert smooth.any() == (d.normals is not None) == (d.smooth is not None)
    if smooth.any():
        assert d.smooth.dtype == np.int32 and np.array_equal(d.smooth[d.tri_mesh] == 1, smooth)
        for k, at in enumerate((M.T_N0, M.T_N1, M.T_N2)):
            assert np.array_equal(d.normals[d.faces[smooth, k]], by_number[smooth, at:at + 3])
    if image:
        uvs = table[int(table[M.MH_UVS]):][:T * M.UV_WORDS].reshape(T, M.UV_WORDS)
        assert np.array_equal(d.uvs, uvs[np.argsort(rows[:, M.T_NUM])])
    assert d.max_leaf == (0 if leaf is None else leaf)
    first = np.concatenate([[0], np.cumsum([len(m.faces) for m in shapes])[:-1]])
    assert np.array_equal(d.first_triangle, first)
    # cached by content, under mesh_table's key
    again, key = M.device_inputs_entry(shapes, leaf)
    assert again is d and key == M.mesh_table_entry(shapes, leaf)[1]


def test_device_inputs_refuses_with_mesh_tables_messages():
    from python_ray_tracer_amd.infrastructure.hip import HipShader, ImageTexture

    nan = float("nan")
    for mesh, what in ((_mesh(vertices=((0, 0, 0), (1, 0, nan), (0, 1, 0))), "not finite"),
                       (_mesh(faces=((0, 1, 3),)), "face index"), (_mesh(faces=((0, -1, 2),)), "face index"),
                       (_mesh(faces=np.zeros((0, 3), dtype=int)), "no faces"),
                       (_mesh(normals=((0, 0, 1), (0, 0, 1))), "normals must be"),
                       (_mesh(normals=((0, 0, 1), (0, 0, 1), (0, nan, 1))), "normal is not finite"),
                       (_mesh(vertices=((0, 0), (1, 0), (0, 1))), "vertices must be"),
                       (_mesh(faces=((0, 1, 2, 0),)), "faces must be")):
        for build in (M.mesh_table, M.device_inputs):
            with pytest.raises(ValueError, match=what) as err:
                build([mesh])
            if build is M.mesh_table:
                text = str(err.value)
        assert str(err.value) == text  # the same words
    glassy = _mesh()
    glassy.shader.transmission_gain = 0.5
    with pytest.raises(ValueError, match="transmission_gain"):
        M.device_inputs([glassy])
    with pytest.raises(ValueError, match="ImageTexture"):
        M.device_inputs([_mesh(sh=HipShader(*GAINS, ImageTexture(np.ones((2, 2, 3)))))])
    for leaf in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_leaf"):
            M.device_inputs([_mesh()], leaf)
    with pytest.raises(ValueError, match="no TriangleMesh"):
        M.device_inputs([])
    many = _mesh(faces=np.tile([[0, 1, 2]], ((1 << 20) + 1, 1)))
    with pytest.raises(ValueError, match="at most 1048576 triangles"):
        M.device_inputs([many])
    # a degenerate face is the device's to find; the host's words for it come from the status word
    for mesh in (_mesh(faces=((0, 1, 1),)), _mesh(vertices=((0, 0, 0), (1, 0, 0), (2, 0, 0)))):
        d = M.device_inputs([_mesh(), mesh])
        with pytest.raises(ValueError) as err:
            M.mesh_table([_mesh(), mesh])
        assert str(M.degenerate_face_error(d, 1)) == str(err.value) and "mesh 1: face 0 is degenerate" in str(err.value)


def test_tree_ranges_are_the_host_trees():
    rng = np.random.default_rng(5)
    for T in (1, 2, 3, 5, 9, 17, 100, 321):
        lo = rng.normal(size=(T, 3))
        for leaf in LEAVES:
            _, s, e = M.build_tree(lo, lo + 0.1, leaf)
            s2, e2 = M.tree_ranges(T, leaf)
            assert np.array_equal(s, s2) and np.array_equal(e, e2)


# ---- the renderer ---------------------------------------------------------------------------------------------

def test_the_renderer_refuses_another_mesh_build_before_the_library_and_the_gpu(monkeypatch):
    """``mesh_build`` is an attribute with a checked assignment (the constructor's signature is pinned by
    tests/test_host_cpu.py): a renderer whose library and device fail on any use takes the two values, refuses
    every other, and one that never saw its constructor builds on the host."""
    r = _renderer(monkeypatch)
    assert r.mesh_build == "host"
    for bad in ("gpu", "Device", None, 1, "", ["device"]):
        with pytest.raises(ValueError, match='mesh_build must be "host" or "device"'):
            r.mesh_build = bad
        assert r.mesh_build == "host"
    r.mesh_build = "device"
    assert r.mesh_build == "device"
    r.mesh_build = "host"
    assert r.mesh_build == "host"


def test_device_mode_refuses_where_host_mode_does_before_any_gpu_use(monkeypatch):
    from python_ray_tracer_amd.domain import EnvironmentLight

    r = _renderer(monkeypatch)
    r.mesh_build = "device"
    scene = scenes.build_scene(scenes.mesh_spec(W, H, 1))
    with pytest.raises(ValueError, match="render_aovs.*TriangleMesh.*passes"):
        r.render_aovs(scene)
    r.max_bounces = None
    with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
        r.render(scene)
    r.max_bounces = 3
    env = scenes.build_scene(scenes.mesh_spec(W, H, 1))
    env.lights.append(EnvironmentLight(np.ones((2, 4, 3))))
    with pytest.raises(ValueError, match="TriangleMesh and an EnvironmentLight"):
        r.render(env)
    bad = scenes.build_scene(scenes.mesh_spec(W, H, 1))
    bad.shapes[-1].vertices[0, 0] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        r.render(bad)
    # the tables: the inputs in the host table's place, under the host table's key
    host = _renderer(monkeypatch)._mesh_table(scene, "render")
    dev = r._mesh_table(scene, "render")
    assert isinstance(dev.host, M.DeviceInputs) and isinstance(host.host, np.ndarray)
    assert dev.key == host.key and dev.uv == host.uv is False
    textured = scenes.build_scene(scenes.textured_mesh_spec(W, H))
    assert r._mesh_table(textured, "render").uv is True


# ---- the preconditions of the GPU cases -----------------------------------------------------------------------

def test_the_twice_case_has_equal_centres_in_one_segment():
    c = _centres(twice_case())
    assert np.array_equal(c[:20], c[20:])  # every triangle's twin, 20 numbers on, in the root's segment
    table = M.mesh_table(twice_case(), 4)
    rows = _parts(table)[0]
    # ... and the host puts a triangle before its twin: by number
    num = rows[:, M.T_NUM].astype(int)
    where = np.argsort(num)
    assert (where[:20] < where[20:]).all()


def test_the_box_case_has_a_centre_of_minus_zero_and_equal_extents():
    c = _centres(box_case())
    ext = c.max(axis=0) - c.min(axis=0)
    assert ext[0] == ext[1] == ext[2] == 2.0  # the first axis wins: x
    x = c[:, 0]
    minus = (x == 0) & np.signbit(x)
    plus = (x == 0) & ~np.signbit(x)
    assert list(np.nonzero(minus)[0]) == [12, 13] and plus.sum() == 8
    # the host's order at one leaf: -1, -1, the eight zeros and then the two minus zeros by number, 1, 1
    rows = _parts(M.mesh_table(box_case(), None))[0]
    assert list(rows[:, M.T_NUM]) == list(range(14))
    rows = _parts(M.mesh_table(box_case(), 8))[0]
    num = rows[:, M.T_NUM].astype(int)
    keys = x[num]
    assert (np.diff(keys[:7]) >= 0).all() and (np.diff(keys[7:]) >= 0).all()
    zeros = [n for n in num if x[n] == 0]
    assert zeros == sorted(zeros) and zeros[-2:] == [12, 13]  # an order that takes -0.0 below 0.0 puts them first


def test_the_strip_case_has_a_cut_segment_beside_an_uncut_one():
    s, e = M.tree_ranges(9, 4)
    length = e - s
    by_start = {(int(a), int(b)) for a, b in zip(s, e)}
    assert (0, 5) in by_start and (5, 9) in by_start  # the second level's segments
    assert (0, 3) in by_start and (3, 5) in by_start  # the first is cut
    assert not any(a == 5 and b < 9 for a, b in by_start) and length.max() == 9  # its neighbour is a leaf


# ---- the library ----------------------------------------------------------------------------------------------

def test_the_library_exports_the_build_entries():
    lib = L.load()
    for name in ("rtx_mesh_build", "rtx_mesh_build_nodes", "rtx_mesh_build_workspace_bytes"):
        assert name in L.EXPORTS and ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    assert L.MB_NONE == 0xFFFFFFFF


def test_node_counts_and_workspace_sizes():
    lib = L.load()
    for T in [*range(1, 200), 1346, 6146, 82946, 1 << 20]:
        for leaf in (None, 1, 2, 3, 4, 7, 8, 64):
            N = M.tree_ranges(T, leaf)[0].shape[0]
            assert lib.rtx_mesh_build_nodes(T, leaf or 0) == N, (T, leaf)
    assert [lib.rtx_mesh_build_nodes(*a) for a in ((0, 4), (-1, 4), ((1 << 20) + 1, 4), (10, -1))] == [0, 0, 0, 0]
    ws = lib.rtx_mesh_build_workspace_bytes
    assert [ws(*a) for a in ((0, 1), (-3, 1), ((1 << 20) + 1, 1), (10, 0), (10, 21))] == [0, 0, 0, 0, 0]
    sizes = [ws(T, lib.rtx_mesh_build_nodes(T, 4)) for T in (1, 2, 100, 6146, 82946, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] < 512 << 20
    assert ws(100, 200) > ws(100, 1)


def build_argument_errors(lib):
    """Every listed argument error of rtx_mesh_build returns RTX_E_ARG (-1) before any HIP call: the device
    pointers below are never dereferenced."""
    p = ctypes.c_void_p(4096)
    d = M.device_inputs(strip_case(), 4)
    T, words = 9, d.skeleton.size
    N = int(d.skeleton[M.MH_NNODES])
    need = lib.rtx_mesh_build_workspace_bytes(T, N)

    def call(verts=p, nv=11, faces=p, tri_mesh=p, T=T, normals=None, smooth=None, uvs=None, head=d.skeleton, table=p,
             words=words, leaf=4, ws=p, ws_bytes=need):
        head_p = None if head is None else np.ascontiguousarray(head[:M.HDR_WORDS]).ctypes.data
        rc = lib.rtx_mesh_build(verts, nv, faces, tri_mesh, T, normals, smooth, uvs, head_p, table, words, leaf, ws,
                                ws_bytes, None)
        return rc, lib.rtx_last_error().decode()

    def header(**words_):
        h = d.skeleton[:M.HDR_WORDS].copy()
        for k, v in words_.items():
            h[getattr(M, k)] = v
        return h

    bad = [dict(verts=None), dict(faces=None), dict(tri_mesh=None), dict(head=None), dict(table=None), dict(ws=None),
           dict(normals=p), dict(smooth=p), dict(T=0), dict(T=(1 << 20) + 1), dict(T=8), dict(nv=0), dict(leaf=-1),
           dict(words=words - 1), dict(words=M.HDR_WORDS - 1), dict(words=1 << 31), dict(ws_bytes=need - 1),
           dict(ws_bytes=0), dict(leaf=2), dict(leaf=0),  # (the skeleton is leaf 4's: another tree's node count)
           dict(head=header(MH_MAGIC=1.0)), dict(head=header(MH_NNODES=N + 1)), dict(head=header(MH_NODES=words)),
           dict(head=header(MH_TRIS=words - 10)), dict(head=header(MH_UVS=words - 1)), dict(head=header(MH_NMESH=0))]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg, (kw, rc, msg)
    assert "fewer than its header says" in call(words=words - 1)[1]
    assert "rtx_mesh_build_workspace_bytes" in call(ws_bytes=need - 1)[1]


def test_argument_checks_need_no_gpu():
    build_argument_errors(L.load())
