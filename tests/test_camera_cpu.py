"""The perspective camera (domain.PerspectiveCamera, python_ray_tracer_amd/camera.py, rtx_camera_rays):
what needs no GPU.

The C ABI entry point and its host-side argument checks, the rt::camera_rays op (schema, Meta shapes,
TORCH_CHECKs), the camera basis and the lens table, every refusal, the scene specs, and the camera's
semantics on the oracle alone (tests/camera_ref.py's rays through oracle.numpy_oracle.intersect), so
that a restatement that is wrong yet agrees with the kernel cannot pass.
"""

import copy
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import camera as C
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.domain import Camera, PerspectiveCamera, Vector3D
from python_ray_tracer_amd.infrastructure.hip import HipRenderer
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import camera_ref as R

REPO = Path(__file__).resolve().parent.parent


def _cam(position=(0, 0.5, -2), target=(0, 0.5, 3), width=48, height=32, **kw):
    return PerspectiveCamera(Vector3D(*position), width, height, Vector3D(*target), **kw)


# ---------------------------------------------------------------- the C ABI
def test_header_sigs_and_exports_agree_and_the_abi_is_still_3():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"int rtx_camera_rays\(const double\* cam, const double\* lens, int k, int width, int height,\s*"
                     r"int row_block, int n_parts, int part, int part_run, int n_local_rows,\s*"
                     r"double\* origins_out, double\* dirs_out, void\* stream\);", text)
    assert "base.py:123-141" in text[text.index("A perspective camera's ray generator"):text.index("int rtx_camera_rays(")]
    for name, value in (("RTX_CAM_WORDS", 24), ("RTX_C_EYE", 0), ("RTX_C_FWD", 3), ("RTX_C_U", 6), ("RTX_C_V", 9),
                        ("RTX_C_LU", 12), ("RTX_C_LV", 15)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    assert (C.CAM_WORDS, C.C_EYE, C.C_FWD, C.C_U, C.C_V, C.C_LU, C.C_LV) == (24, 0, 3, 6, 9, 12, 15)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION == 3
    p, i32 = ctypes.c_void_p, ctypes.c_int
    assert L._SIGS["rtx_camera_rays"] == (i32, [p, p, i32, i32, i32, i32, i32, i32, i32, i32, p, p, p])
    lib = L.load()
    layout = (ctypes.c_int * 8)()
    assert lib.rtx_abi_version(layout, 8) == 3
    assert "rtx_camera_rays" in L.EXPORTS and hasattr(lib, "rtx_camera_rays")
    assert ctypes.cast(lib.rtx_camera_rays, ctypes.c_void_p).value


def test_argument_checks_need_no_gpu():
    """Every bad argument returns RTX_E_ARG (-1) with a message before any HIP call, and an empty tile
    returns RTX_OK without a launch: the device pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)
    err = lib.rtx_last_error
    pinhole = C.camera_record(_cam())
    lensed = C.camera_record(_cam(lens_radius=0.05))

    def rays(cam=pinhole, lens=None, k=2, width=8, height=4, row_block=1, n_parts=1, part=0, part_run=1, rows=None,
             origins=None, dirs=p):
        rows = height if rows is None else rows
        cam_p = None if cam is None else cam.ctypes.data
        return lib.rtx_camera_rays(cam_p, lens, k, width, height, row_block, n_parts, part, part_run, rows, origins,
                                   dirs, None)

    assert rays(cam=None) == -1 and b"null" in err()
    assert rays(dirs=None) == -1 and b"null" in err()
    for k in (0, -1, 9, 64):
        assert rays(k=k) == -1 and b"1..8" in err(), k
    for kw in ({"width": 0}, {"width": -3}, {"height": 0}, {"row_block": 0}, {"n_parts": 0}, {"part": -1},
               {"n_parts": 2, "part": 2, "rows": 0}, {"n_parts": 3, "part": 2, "part_run": 2, "rows": 0}, {"part_run": 0},
               {"rows": 5}, {"rows": -1}, {"n_parts": 2, "part": 1, "rows": 3}):
        assert rays(**kw) == -1 and b"geometry" in err(), kw
    # k*width or k*height at 2^31, and n = k*k*width*rows at 2^31 (exactly, and beyond)
    assert rays(k=2, width=1 << 30, height=1, rows=0) == -1 and b"2^31" in err()
    assert rays(k=8, width=1, height=1 << 28, rows=0) == -1 and b"2^31" in err()
    for k, w, h in ((2, 1 << 15, 1 << 14), (8, 1 << 13, 1 << 12), (1, 1 << 16, 1 << 15), (3, 238609295, 1)):
        assert k * k * w * h >= 2**31
        assert rays(k=k, width=w, height=h) == -1 and b"2^31" in err(), (k, w, h)
    # a record with a lens needs the lens table and somewhere to put the origins
    assert rays(cam=lensed) == -1 and b"lens" in err()
    assert rays(cam=lensed, lens=p) == -1 and b"lens" in err()
    assert rays(cam=lensed, origins=p) == -1 and b"lens" in err()
    for word in (0, 4, 8, 17):
        for bad in (math.nan, math.inf, -math.inf):
            rec = pinhole.copy()
            rec[word] = bad
            assert rays(cam=rec) == -1 and b"finite" in err(), (word, bad)
    # an empty tile: nothing to launch, with or without a lens
    assert rays(n_parts=8, part=5, rows=0) == 0
    assert rays(cam=lensed, lens=p, origins=p, n_parts=8, part=5, rows=0) == 0


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "camera_rays" in ops.OPS
    assert str(torch.ops.rt.camera_rays.default._schema) == \
        ("rt::camera_rays(Tensor cam, Tensor? lens, int k, int width, int height, int row_block=1, int n_parts=1, "
         "int part=0, int part_run=1) -> (Tensor?, Tensor)")
    W, H, k = 7, 5, 3
    cam = torch.empty(24, dtype=torch.float64, device="meta")
    lens = torch.empty(2, k * k, dtype=torch.float64, device="meta")
    o, d = torch.ops.rt.camera_rays(cam, None, k, W, H)
    assert o is None and tuple(d.shape) == (3, k * k * W * H) and d.dtype == torch.float64 and d.device.type == "meta"
    o, d = torch.ops.rt.camera_rays(cam, lens, k, W, H)
    assert tuple(o.shape) == tuple(d.shape) == (3, k * k * W * H) and o.dtype == torch.float64
    o, d = torch.ops.rt.camera_rays(cam, lens, k, W, H, 2, 3, 1, 1)  # rows 2, 3 of every 6: two of five rows
    assert tuple(o.shape) == tuple(d.shape) == (3, k * k * W * 2)
    assert tuple(torch.ops.rt.camera_rays(cam, None, 1, W, H, 2, 3, 1, 2)[1].shape) == (3, W * 3)
    for bad in (cam[:23], torch.empty(24, dtype=torch.float32, device="meta"),
                torch.empty(2, 12, dtype=torch.float64, device="meta")):
        with pytest.raises(RuntimeError, match="cam must be"):
            torch.ops.rt.camera_rays(bad, None, k, W, H)
    for bad in (lens[:, :-1], torch.empty(2, k * k, dtype=torch.float32, device="meta"),
                torch.empty(2, 16, dtype=torch.float64, device="meta")):
        with pytest.raises(RuntimeError, match="lens must be"):
            torch.ops.rt.camera_rays(cam, bad, k, W, H)
    with pytest.raises(RuntimeError, match="1..8"):
        torch.ops.rt.camera_rays(cam, None, 9, W, H)
    with pytest.raises(RuntimeError, match="geometry"):
        torch.ops.rt.camera_rays(cam, None, k, W, H, 1, 2, 2)
    with pytest.raises(RuntimeError, match="2\\^31"):
        torch.ops.rt.camera_rays(cam, None, 2, 1 << 15, 1 << 14)
    # on the host: the record must be a host tensor, the lens table a GPU tensor
    host = torch.from_numpy(C.camera_record(_cam(lens_radius=0.05)))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.camera_rays(host, torch.zeros(2, k * k, dtype=torch.float64), k, W, H)


# ---------------------------------------------------------------- the camera basis
def test_axis_aligned_basis_is_exact():
    cam = _cam(position=(0, 0.5, -2), target=(0, 0.5, 3), up=(0, 1, 0))
    b = C.camera_basis(cam)
    assert b["fwd"] == (0.0, 0.0, 1.0) and b["right"] == (1.0, 0.0, 0.0) and b["tup"] == (0.0, 1.0, 0.0)
    rec = C.camera_record(cam)
    assert rec.shape == (24,) and rec.dtype == np.float64
    assert rec[C.C_EYE:C.C_EYE + 3].tolist() == [0.0, 0.5, -2.0]
    assert rec[C.C_FWD:C.C_FWD + 3].tolist() == [0.0, 0.0, 5.0]
    hh = math.tan(math.radians(40.0) / 2.0)
    assert rec[C.C_U:C.C_U + 3].tolist() == [hh * (48.0 / 32) * 5.0, 0.0, 0.0]
    assert rec[C.C_V:C.C_V + 3].tolist() == [0.0, hh * 5.0, 0.0]
    assert not rec[C.C_LU:].any()
    lensed = C.camera_record(_cam(lens_radius=0.15, focus_distance=2.0))
    assert lensed[C.C_FWD:C.C_FWD + 3].tolist() == [0.0, 0.0, 2.0]
    assert lensed[C.C_LU:C.C_LU + 3].tolist() == [0.15, 0.0, 0.0] and lensed[C.C_LV:C.C_LV + 3].tolist() == [0.0, 0.15, 0.0]
    assert not lensed[18:].any()


TILTED = dict(position=(2.5, 1.75, 4.25), target=(-0.3, 0.2, 1.0), up=(0.2, 1.0, -0.1), fov=55.0)


def test_tilted_basis_is_orthonormal_and_equals_the_restatement():
    cam = _cam(**TILTED, width=37, height=23)
    b = C.camera_basis(cam)
    f, r, t = (np.array(b[name]) for name in ("fwd", "right", "tup"))
    assert abs(np.dot(np.array(TILTED["up"]), f)) > 0.1  # up is not perpendicular to the view
    for v in (f, r, t):
        assert abs(np.dot(v, v) - 1.0) <= 1e-15
    for v, w in ((f, r), (f, t), (r, t)):
        assert abs(np.dot(v, w)) <= 1e-15
    assert np.dot(t, np.array(TILTED["up"])) > 0  # the true up stays on up's side
    for kw in ({}, {"lens_radius": 0.05}, {"lens_radius": 0.05, "focus_distance": 7.5}):
        cam = _cam(**TILTED, width=37, height=23, **kw)
        assert np.array_equal(C.camera_record(cam), R.record_ref(cam))
    # up given as a Vector3D, as build_scene gives it
    cam = _cam(**{**TILTED, "up": Vector3D(*TILTED["up"])}, width=37, height=23)
    assert np.array_equal(C.camera_record(cam), R.record_ref(cam))


def test_middle_ray_is_the_view_direction_and_the_edges_span_the_field_of_view():
    cam = _cam(width=3, height=3)  # fwd = +z, tup = +y
    _, dirs = R.rays_ref(cam, 1, [0, 1, 2], lens=False)
    assert tuple(dirs[:, 4]) == C.camera_basis(cam)["fwd"] == (0.0, 0.0, 1.0)  # exactly: u = v = 0, d = C
    tilted = _cam(**TILTED, width=3, height=3)
    _, dirs = R.rays_ref(tilted, 1, [0, 1, 2], lens=False)
    assert np.abs(dirs[:, 4] - np.array(C.camera_basis(tilted)["fwd"])).max() <= 4e-16  # (renormalised: an ulp)
    for fov, H in ((40.0, 32), (75.0, 23), (20.0, 5)):
        cam = _cam(width=1, height=H, fov=fov)  # one column: u = 0
        _, d = R.rays_ref(cam, 1, [0, H - 1], lens=False)
        top, bottom = d[:, 0], d[:, 1]
        assert top[0] == 0.0 and bottom[0] == 0.0
        want = math.tan(math.radians(fov) / 2.0) * (H - 1) / H  # the edge pixels' centres, in tangent space
        assert abs(top[1] / top[2] - want) <= 1e-14 and abs(bottom[1] / bottom[2] + want) <= 1e-14


# ---------------------------------------------------------------- the lens table
@pytest.mark.parametrize("k", range(1, 9))
def test_lens_table(k):
    t = C.lens_table(k)
    assert t.shape == (2, k * k) and t.dtype == np.float64
    assert np.array_equal(t, R.lens_table_ref(k))
    assert len({(x, y) for x, y in t.T}) == k * k  # distinct points
    assert np.all(t[0] * t[0] + t[1] * t[1] < 1.0)  # inside the unit disk
    assert abs(t[0].mean()) < 1e-15 and abs(t[1].mean()) < 1e-15
    if k == 3:
        assert t[:, 4].tolist() == [0.0, 0.0]
    if k == 1:
        assert t.tolist() == [[0.0], [0.0]]


def test_lens_table_refuses_a_bad_k():
    for bad in (0, 9, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="1..8"):
            C.lens_table(bad)


# ---------------------------------------------------------------- refusals
def test_camera_refusals():
    nan, inf = math.nan, math.inf
    for kw in ({"position": (0, nan, -2)}, {"target": (inf, 0, 0)}, {"up": (0, 1, nan)}, {"fov": nan},
               {"lens_radius": inf}, {"focus_distance": nan}, {"focus_distance": inf}):
        with pytest.raises(ValueError, match="finite"):
            C.camera_record(_cam(**kw))
    with pytest.raises(ValueError, match="target"):  # dist == 0
        C.camera_record(_cam(position=(1, 2, 3), target=(1, 2, 3)))
    for up in ((0, 0, 1), (0, 0, -2.5), (0, 0, 0), (0, 1e-13, 1)):  # parallel to the view (or nearly, or zero)
        with pytest.raises(ValueError, match="up"):
            C.camera_record(_cam(up=up))
    C.camera_record(_cam(up=(0, 1e-11, 1)))  # r.r = 1e-22 > 1e-24 * up.up
    for fov in (0, 180, -40, 180.5, 360):
        with pytest.raises(ValueError, match="fov"):
            C.camera_record(_cam(fov=fov))
    with pytest.raises(ValueError, match="lens_radius"):
        C.camera_record(_cam(lens_radius=-0.01))
    for F in (0, -1.0):
        with pytest.raises(ValueError, match="focus_distance"):
            C.camera_record(_cam(focus_distance=F))
    for kw in ({"fov": "40"}, {"lens_radius": None}, {"focus_distance": "far"}, {"fov": True}):
        with pytest.raises(ValueError):
            C.camera_record(_cam(**kw))
    with pytest.raises(ValueError, match="3-vector|three"):
        C.camera_record(_cam(up=(0, 1)))
    with pytest.raises(ValueError, match="PerspectiveCamera"):
        C.camera_record(Camera(Vector3D(0, 0, -2), 8, 4))
    # depth of field needs samples
    with pytest.raises(ValueError, match="samples >= 2"):
        C.check_camera(_cam(lens_radius=0.05), 1)
    assert C.check_camera(_cam(lens_radius=0.05), 2).shape == (24,)
    assert C.check_camera(_cam(), 1).shape == (24,)


def _bare(**attrs):
    """A HipRenderer that never saw its constructor (no library, no device): a refusal that reaches
    for either would fail with something other than the ValueError asked for."""
    r = object.__new__(HipRenderer)
    for k, v in {"samples": 1, "adaptive": False, **attrs}.items():
        setattr(r, k, v)
    return r


def _scene(**cam_kw):
    spec = scenes.readme_spec(8, 4)
    spec["camera"].update({"position": [1.5, 1.0, -2.0], "target": [0, 0.3, 3], **cam_kw})
    return scenes.build_scene(spec)


def test_renderer_refusals_come_before_any_gpu_use():
    pin, lens = _scene(), _scene(lens_radius=0.05)
    r1, r2 = _bare(), _bare(samples=2)
    # a lens with samples == 1, wherever the camera enters
    for call in (lambda: r1.render_tile(lens), lambda: r1.render(lens), lambda: r1.render_tile(lens, 2, 3, 1, out="u8"),
                 lambda: r1.render_batch([pin, lens]), lambda: r1.get_ray_directions(lens.camera),
                 lambda: r1.camera_rays(lens.camera), lambda: r1.render_aovs(lens)):
        with pytest.raises(ValueError, match="samples >= 2"):
            call()
    # a bad camera, through the renderer
    for bad in (_scene(fov=0), _scene(up=[-1.5, -0.7, 5.0]), _scene(target=[1.5, 1.0, -2.0])):
        for r in (r1, r2):
            with pytest.raises(ValueError, match="fov|up|target"):
                r.render_tile(bad)
            with pytest.raises(ValueError, match="fov|up|target"):
                r.get_ray_directions(bad.camera)
    # a caller's blob holds the reference camera
    for r, sc in ((r1, pin), (r2, lens)):
        with pytest.raises(ValueError, match="blob"):
            r.render_tile(sc, blob=torch.zeros(200, dtype=torch.float64), n_spheres=3)
    # the native row-tiled plan, adaptive anti-aliasing and the edge mask
    for r, sc in ((r1, pin), (r2, pin), (r2, lens)):
        with pytest.raises(ValueError, match="PerspectiveCamera"):
            r.submit_tiles(None, 0, sc, 4, 1, 0, None)
        with pytest.raises(ValueError, match="PerspectiveCamera"):
            r.edge_mask(sc)
    ra = _bare(samples=2, adaptive=True)
    for call in (lambda: ra.render_tile(pin), lambda: ra.render(lens), lambda: ra.edge_mask(pin),
                 lambda: ra.submit_tiles(None, 0, pin, 4, 1, 0, None)):
        with pytest.raises(ValueError, match="PerspectiveCamera"):
            call()
    with pytest.raises(ValueError, match="adaptive"):
        ra.render_batch([pin, pin])
    # render passes: one sample per pixel, no lens
    with pytest.raises(ValueError, match="samples=2"):
        r2.render_aovs(pin)
    with pytest.raises(ValueError, match="samples=2"):
        r2.render_aovs(lens)
    # materialised directions: a pinhole at samples == 1 only
    rays = r2.get_ray_directions(lens.camera)
    with pytest.raises(ValueError, match="one direction per pixel"):
        rays.data
    with pytest.raises(ValueError, match="one direction per pixel"):
        r2.get_ray_directions(pin.camera).x
    with pytest.raises(ValueError, match="PerspectiveCamera"):
        r1.camera_rays(Camera(Vector3D(0, 0, -2), 8, 4))


def test_a_plain_camera_at_the_same_position_is_another_camera():
    from python_ray_tracer_amd.infrastructure.hip.base import _same_camera

    pin = _scene().camera
    plain = Camera(pin.position, pin.width, pin.height)
    assert _same_camera(pin, pin) and _same_camera(plain, plain)
    assert not _same_camera(pin, plain) and not _same_camera(plain, pin)
    assert _same_camera(pin, _scene().camera)  # equal by value
    for other in (_scene(fov=41.0), _scene(target=[0, 0.3, 3.5]), _scene(up=[0, 1, 0.1]), _scene(lens_radius=0.1),
                  _scene(focus_distance=4.0)):
        assert not _same_camera(pin, other.camera)


# ---------------------------------------------------------------- scene specs
def test_specs_round_trip_the_camera_keys():
    spec = scenes.readme_spec(16, 9)
    assert type(scenes.build_scene(spec).camera) is Camera  # no "target": the reference camera
    full = scenes.with_camera(spec, [1, 2, -3], target=[0, 0.5, 3], up=[0.1, 1, 0], fov=55.0, lens_radius=0.05,
                              focus_distance=4.5)
    assert "target" not in spec["camera"]  # a copy
    assert full["camera"] == {"position": [1, 2, -3], "width": 16, "height": 9, "target": [0, 0.5, 3], "up": [0.1, 1, 0],
                              "fov": 55.0, "lens_radius": 0.05, "focus_distance": 4.5}
    cam = scenes.build_scene(full).camera
    assert isinstance(cam, PerspectiveCamera) and isinstance(cam, Camera)
    assert (cam.position.x, cam.position.y, cam.position.z) == (1, 2, -3) and (cam.width, cam.height) == (16, 9)
    assert (cam.target.x, cam.target.y, cam.target.z) == (0, 0.5, 3) and (cam.up.x, cam.up.y, cam.up.z) == (0.1, 1, 0)
    assert (cam.fov, cam.lens_radius, cam.focus_distance) == (55.0, 0.05, 4.5)
    # the other four keys are optional
    cam = scenes.build_scene(scenes.with_camera(spec, target=[0, 0.5, 3])).camera
    assert (tuple(cam.up), cam.fov, cam.lens_radius, cam.focus_distance) == ((0.0, 1.0, 0.0), 40.0, 0.0, None)
    # with_camera passes the keys of a perspective spec through
    moved = scenes.with_camera(full, [4, 5, 6], width=32)
    assert moved["camera"] == {**full["camera"], "position": [4, 5, 6], "width": 32}
    assert scenes.build_scene(moved).camera.fov == 55.0
    # the packer and the scene key read position, width and height as ever
    from python_ray_tracer_amd.infrastructure.hip.scene_pack import scene_key

    plain = scenes.build_scene(scenes.with_camera(spec, [1, 2, -3]))
    assert scene_key(scenes.build_scene(full)) == scene_key(plain)


# ---------------------------------------------------------------- semantics, on the oracle alone
def _dof_spec():
    spec = scenes.readme_spec(48, 32)
    near = copy.deepcopy(spec["spheres"][0])
    near["center"], near["radius"] = [0, 0.5, 3], 0.5  # in focus
    far = copy.deepcopy(near)
    far["center"] = [1.6, 0.5, 9]  # out of focus
    spec["spheres"] = [near, far, spec["spheres"][2]]
    return spec


def _coverage(spec, k=4, **cam_kw):
    """Per sphere (fully covered pixels, partly covered pixels, samples), and the sample-frame map of
    the shape each sample sees: the argmin of intersect over the scene's spheres, -1 on a miss."""
    W, H = 48, 32
    cam = _cam(position=(0, 0.5, -2), target=(0, 0.5, 3), width=W, height=H, **cam_kw)
    o, d = R.rays_ref(cam, k, range(H), lens=cam.lens_radius > 0)
    dist = np.stack([O.intersect(sp, *o, *d) for sp in O.scene_from_spec(spec).spheres])
    shape = np.where(dist.min(axis=0) < O.FARAWAY, np.argmin(dist, axis=0), -1)
    out = []
    for s in (0, 1):
        cov = (shape.reshape(H, k, W, k) == s).sum(axis=(1, 3))
        out.append((int((cov == k * k).sum()), int(((cov > 0) & (cov < k * k)).sum()), int(cov.sum())))
    return out, shape.reshape(H * k, W * k)


def test_depth_of_field_and_field_of_view_on_the_oracle():
    spec = _dof_spec()
    (pin0, pin1), shape = _coverage(spec)
    (dof0, dof1), _ = _coverage(spec, lens_radius=0.15)
    (tele0, _), _ = _coverage(spec, fov=20.0)
    print("pinhole", pin0, pin1, "lens 0.15", dof0, dof1, "fov 20", tele0)
    assert shape[64, 96] == 0  # the centre sample looks at the target
    # the sphere in the plane of focus keeps its outline ...
    assert abs(dof0[2] - pin0[2]) < 0.02 * pin0[2]
    assert abs(dof0[0] - pin0[0]) <= 1
    # ... the one behind it is smeared over more pixels
    assert dof1[1] >= 1.5 * pin1[1]
    # half the field of view: four times the area
    assert tele0[2] > 4 * pin0[2]
