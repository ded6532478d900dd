"""The mesh table made on the GPU (rtx_mesh_build, HipRenderer.mesh_build = "device").

The contract is the host's table: the device-built table is downloaded and compared with
``meshes.mesh_table`` by ``np.array_equal``, every word (a zero's sign is free, as it is for
``array_equal``), and frames from the two tables by ``torch.equal``. tests/test_mesh_build_cpu.py checks
that the small cases hold the ties, the -0.0, the equal extents and the uncut neighbour they are here for."""

import copy
import ctypes

import numpy as np
import pytest
import torch

from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests.test_mesh_build_cpu import CASES, LEAVES, _meshes_of, _parts, _shader, build_argument_errors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _device_renderer(hip, cap=3):
    r = hip.HipRenderer(cap)
    assert r.mesh_build == "host"  # the default
    r.mesh_build = "device"
    return r


@pytest.fixture(scope="module")
def renderer(hip):
    return _device_renderer(hip)


def _build(renderer, shapes, leaf):
    """The device-built table of ``shapes``, downloaded (built anew: the renderer's cache is emptied)."""
    renderer._mesh_tables.clear()
    inputs, key = M.device_inputs_entry(shapes, leaf)
    return renderer._build_mesh_table(key, inputs).cpu().numpy()


def _same(got, want, what):
    if not np.array_equal(got, want):  # say where, part by part, before failing
        assert got.shape == want.shape, what
        assert np.array_equal(got[:M.HDR_WORDS], want[:M.HDR_WORDS]), (what, "header")
        (r, m, n), (r2, m2, n2) = _parts(got), _parts(want)
        assert np.array_equal(r[:, M.T_NUM], r2[:, M.T_NUM]), (what, "the leaf order", r[:, M.T_NUM], r2[:, M.T_NUM])
        bad = np.nonzero((r != r2).any(axis=0))[0]
        assert bad.size == 0, (what, "row words", bad)
        assert np.array_equal(m, m2), (what, "materials")
        bad = np.nonzero((n != n2).any(axis=0))[0]
        assert bad.size == 0, (what, "node words", bad, np.nonzero((n != n2).any(axis=1))[0][:8])
        assert False, (what, "the UV part or the texel blocks", np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", list(CASES))
def test_small_tables_equal_the_hosts(renderer, name, leaf):
    shapes = CASES[name]()
    _same(_build(renderer, shapes, leaf), M.mesh_table(shapes, leaf), f"{name} leaf {leaf}")


@pytest.mark.parametrize("leaf", LEAVES)
def test_level_4_equals_the_hosts(renderer, leaf):
    """6,146 triangles: several blocks per kernel, segments across blocks and waves, several radix passes."""
    shapes = _meshes_of(scenes.mesh_spec(48, 27, 4))
    assert sum(len(m.faces) for m in shapes) == 6146
    _same(_build(renderer, shapes, leaf), M.mesh_table(shapes, leaf), f"level 4 leaf {leaf}")


def test_level_6_equals_the_hosts(renderer):
    """The benchmark's largest table: 82,946 triangles, 65,535 nodes, at leaf 4."""
    shapes = _meshes_of(scenes.mesh_spec(48, 27, 6))
    want = M.mesh_table(shapes, 4)
    assert (int(want[M.MH_NTRI]), int(want[M.MH_NNODES])) == (82946, 65535)
    _same(_build(renderer, shapes, 4), want, "level 6 leaf 4")


# ---- the renderer ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ["mesh", "textured"])
def test_frames_are_the_host_tables_frames(hip, spec):
    spec = scenes.mesh_spec(64, 36, 1) if spec == "mesh" else scenes.textured_mesh_spec(64, 36)
    host, dev = hip.HipRenderer(3), _device_renderer(hip)
    scene = scenes.build_scene(spec)
    a, b = host.render(scene).data, dev.render(scene).data
    assert a.dtype == torch.float64 and torch.equal(a, b) and float(a.max()) > 0.5
    a8, b8 = host.render_tile(scene, out="u8"), dev.render_tile(scene, out="u8")
    assert a8.dtype == torch.uint8 and torch.equal(a8, b8)
    # the second render built nothing: the cache holds the first render's table
    (key, table), = dev._mesh_tables.items()
    dev.render(scene)
    assert len(dev._mesh_tables) == 1 and dev._mesh_tables[key] is table


def test_a_moved_vertex_gives_the_moved_scenes_host_frame(hip):
    spec = scenes.mesh_spec(64, 36, 1)
    host, dev = hip.HipRenderer(3), _device_renderer(hip)
    scene = scenes.build_scene(spec)
    first = dev.render(scene).data.clone()
    moved = scenes.build_scene(copy.deepcopy(spec))
    mesh = moved.shapes[-2]  # the icosphere
    mesh.vertices[0] = mesh.vertices[0] * 1.5 + 0.1
    want = host.render(moved).data
    got = dev.render(moved).data
    assert torch.equal(got, want) and not torch.equal(got, first) and len(dev._mesh_tables) == 2


def test_a_degenerate_face_raises_the_hosts_message_and_a_clean_build_follows(hip):
    from python_ray_tracer_amd.domain import TriangleMesh

    dev = _device_renderer(hip)
    spec = scenes.mesh_spec(48, 27, 1)
    for where in ("first", "last of the second mesh"):
        scene = scenes.build_scene(copy.deepcopy(spec))
        idx = [i for i, sh in enumerate(scene.shapes) if isinstance(sh, TriangleMesh)]
        mesh = scene.shapes[idx[0] if where == "first" else idx[1]]
        faces = np.array(mesh.faces)
        faces[0 if where == "first" else -1, 1] = faces[0 if where == "first" else -1, 0]  # two corners are one
        mesh.faces = faces
        with pytest.raises(ValueError) as host_err:
            M.mesh_table(scene.shapes)
        with pytest.raises(ValueError) as dev_err:
            dev.render(scene)
        assert str(dev_err.value) == str(host_err.value) and "is degenerate" in str(dev_err.value), where
        assert dev._mesh_tables == {}  # a failed build leaves nothing behind
    scene = scenes.build_scene(spec)
    assert torch.equal(dev.render(scene).data, hip.HipRenderer(3).render(scene).data) and len(dev._mesh_tables) == 1


# ---- the op and the entry -------------------------------------------------------------------------------------

def _op_args(inputs, device):
    up = lambda a: None if a is None else torch.tensor(a, device=device)  # noqa: E731
    return [up(a) for a in (inputs.vertices, inputs.faces, inputs.tri_mesh, inputs.normals, inputs.smooth, inputs.uvs)]


def test_the_op_builds_the_table_and_checks_on_the_host(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    lib = L.load()
    for name, leaf in (("ico1", 4), ("textured", 2), ("strip", None)):
        shapes = CASES[name]()
        d = M.device_inputs(shapes, leaf)
        T, N = d.faces.shape[0], int(d.skeleton[M.MH_NNODES])
        need = lib.rtx_mesh_build_workspace_bytes(T, N)
        args = _op_args(d, "cuda")
        table = torch.tensor(d.skeleton, device="cuda")
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        status = torch.ops.rt.mesh_build(*args, table, d.max_leaf, ws)
        assert status.dtype == torch.int32 and status.tolist() == [-1, 0]
        _same(table.cpu().numpy(), M.mesh_table(shapes, leaf), f"op {name}")
        # the Meta form: the same result shape, nothing run
        meta = [None if a is None else a.to("meta") for a in args]
        out = torch.ops.rt.mesh_build(*meta, table.to("meta"), d.max_leaf, ws.to("meta"))
        assert out.shape == (2,) and out.dtype == torch.int32 and out.device.type == "meta"
        # check=True refuses a short skeleton and a short workspace on the host, before the entry
        with pytest.raises(RuntimeError, match="fewer than its header says"):
            torch.ops.rt.mesh_build(*args, table[:-1].clone(), d.max_leaf, ws)
        with pytest.raises(RuntimeError, match="workspace too small.*rtx_mesh_build_workspace_bytes"):
            torch.ops.rt.mesh_build(*args, table, d.max_leaf, ws[:need - 1].clone())
        # ... and check=False leaves them to the entry's RTX_E_ARG
        with pytest.raises(RuntimeError, match=r"rtx_mesh_build failed \(-1\)"):
            torch.ops.rt.mesh_build(*args, table[:-1].clone(), d.max_leaf, ws, False)
        with pytest.raises(RuntimeError, match=r"rtx_mesh_build failed \(-1\)"):
            torch.ops.rt.mesh_build(*args, table, d.max_leaf, ws[:need - 1].clone(), False)
    with pytest.raises(RuntimeError, match="faces must be"):
        torch.ops.rt.mesh_build(args[0], args[1].to(torch.int64), *args[2:], table, d.max_leaf, ws)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        torch.ops.rt.mesh_build(args[0].cpu(), *args[1:], table, d.max_leaf, ws)
    # a degenerate triangle: the status word without check, an error with it
    from tests.test_mesh_cpu import _mesh

    d = M.device_inputs([_mesh(sh=_shader()), _mesh(faces=((0, 1, 1),), sh=_shader())], 4)
    args = _op_args(d, "cuda")
    ws = torch.empty(lib.rtx_mesh_build_workspace_bytes(2, 1), dtype=torch.uint8, device="cuda")
    status = torch.ops.rt.mesh_build(*args, torch.tensor(d.skeleton, device="cuda"), 4, ws, False)
    assert status.tolist() == [1, 0]
    with pytest.raises(RuntimeError, match="triangle 1 is degenerate"):
        torch.ops.rt.mesh_build(*args, torch.tensor(d.skeleton, device="cuda"), 4, ws)


def test_the_entry_returns_e_arg_for_each_argument_error(hip):
    build_argument_errors(L.load())
    assert ctypes.cast(L.load().rtx_mesh_build, ctypes.c_void_p).value
