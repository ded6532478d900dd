"""Several point lights on the GPU: multi-light scenes through HipRenderer and rt::trace_lights.

Every render is compared with the NumPy restatement (tests/lights_ref.py) at the project's bar for float64
colour, |GPU - restatement| <= 1e-12 * max(1, |colour|) (the kernel sums the same terms in another
association), and its uint8 frame must be identical, no pixel excluded: tests/test_lights_cpu.py checks
that no pixel of a case sits within 1e-9 of a quantisation step. Which rays exist, what they hit and which
light reaches a hit are decisions the kernel must take bit for bit like the restatement; a wrong one moves a
pixel by far more than the bar. The counts asserted with each case keep it from passing on a frame that
proves nothing. Nothing here provokes an overflow of a lane's stack: the stack filled to its last entry and one
over, and a worker's second item at a cap above 0, are in tests/test_gpu_lights_limits.py.
"""

import copy

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import lights, scenes, tiling
from tests import lights_ref as R
from tests import ssaa_ref
from tests.test_lights_cpu import H, W, colored, frame, pool, step_distance, with_lights

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


def _render(hip, spec, cap, **kw):
    r = hip.HipRenderer(cap, **kw)
    r._lib = calls = _Calls(r._lib)
    return r.render(scenes.build_scene(spec)).data.cpu().numpy(), calls.names


ONE_LIGHT = {
    "readme": lambda: scenes.readme_spec(W, H),
    "main": lambda: scenes.main_spec(W, H),
    "rand17": lambda: scenes.random_spec(16, 1, W, H),
    "rand65": lambda: scenes.random_spec(64, 2, 48, 27),  # a culling tree in the nearest-hit search too
}


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("key", sorted(ONE_LIGHT))
def test_one_unit_light_against_the_existing_path(hip, key, cap):
    """ColoredPointLight(p) of intensity 1 and white through k_trace_lights against PointLight(p) through
    today's kernels: both within the bar of the oracle and of each other, the same uint8 frame."""
    spec = ONE_LIGHT[key]()
    w, h = spec["camera"]["width"], spec["camera"]["height"]
    got, names = _render(hip, colored(spec), cap)
    plain, plain_names = _render(hip, spec, cap)
    assert names.count("rtx_trace_lights") == 1 and not any(n.startswith("rtx_render_camera") for n in names)
    assert "rtx_trace_lights" not in plain_names and any(n.startswith("rtx_render_camera") for n in plain_names)
    want = O.render(O.scene_from_spec(spec), cap)
    assert step_distance(want) > 1e-9
    _check(got, want, w, h, f"{key} B={cap} against the oracle")
    _check(got, plain, w, h, f"{key} B={cap} against the one-light path")


@pytest.mark.parametrize("key", ["two", "three", "eight"])
def test_frames_against_the_restatement(hip, key):
    spec, cap, want, c = frame(key)
    assert min(c.first_only, c.other_only, c.several, c.none) > 0 and c.reflected_by_others > 0
    got, names = _render(hip, spec, cap)
    assert names.count("rtx_trace_lights") == 1
    _check(got, want, W, H, key)
    plain = O.render(O.scene_from_spec(spec), cap)  # lights[0] alone: what a renderer that ignores the others gives
    assert int((O.to_uint8(got, W, H) != O.to_uint8(plain, W, H)).any(axis=-1).sum()) > 100


def test_ties_under_two_coincident_spheres(hip):
    spec, cap, want, c = frame("ties")
    assert c.ties > 50 and cap == 3
    got, _ = _render(hip, spec, cap)  # (an overflowed stack would raise RecursionError here)
    _check(got, want, W, H, "ties")


def test_textures_and_the_culling_tree(hip):
    spec, cap, want, c = frame("tree")
    assert len(spec["spheres"]) == 17 and c.several > 0
    got, _ = _render(hip, spec, cap)
    _check(got, want, W, H, "tree")


@pytest.mark.parametrize("key", ["1x1", "7x5", "67x5"])
def test_frames_that_end_inside_a_wave(hip, key):
    spec, cap, want, _ = frame(key)
    got, _ = _render(hip, spec, cap)
    _check(got, want, spec["camera"]["width"], spec["camera"]["height"], key)


def test_a_frame_larger_than_the_pool_of_workers(hip):
    """640 x 360 at cap 0: 230,400 rays for a pool of 196,608 workers, so 33,792 workers take a second
    item (the frame's last 53 rows). Equal to the same frame in row tiles, none of which reaches a second
    lap, bit for bit; every 24th row and the last against the restatement."""
    spec = scenes.lights_spec(640, 360)
    w, h = 640, 360
    p = pool(0)
    assert p < w * h < 2 * p, "the pool was retuned: pick another frame"
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(0)
    full = r.render(scene).data.cpu().numpy().reshape(3, h, w)
    for part in range(4):
        rows = tiling.tile_rows(h, 8, 4, part)
        assert w * len(rows) < p
        tile = r.render_tile(scene, 8, 4, part).cpu().numpy()
        assert np.array_equal(tile, full[:, rows].reshape(3, -1)), part
    rows = sorted(set(range(0, h, 24)) | {h - 1})
    assert sum(row * w >= p for row in rows) >= 2  # rows of the second lap are among them
    want = R.render(spec, 0, rows=rows)
    assert step_distance(want) > 1e-9
    _check(full[:, rows].reshape(3, -1), want, w, len(rows), "rows of the 640x360 frame")


def test_row_tiles_runs_and_outputs(hip):
    spec, cap, want, _ = frame("three")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data.cpu().numpy()
    _check(full, want, W, H, "three")
    full_u8 = r.render_tile(scene, out="u8")
    assert full_u8.dtype == torch.uint8 and tuple(full_u8.shape) == (H, W, 3)
    full_u8 = full_u8.cpu().numpy()
    assert np.array_equal(full_u8, O.to_uint8(want, W, H))
    full = full.reshape(3, H, W)
    rb, P = 4, 3  # 22 rows: one whole cycle of 12 and a partial one
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
    r32 = hip.HipRenderer(cap, color_dtype=torch.float32)
    got32 = r32.render(scene).data
    assert got32.dtype == torch.float32
    assert np.array_equal(got32.cpu().numpy(), full.reshape(3, -1).astype(np.float32))  # the float64 value rounded once


def test_supersampled_frame(hip):
    """samples=2: the sample frame traced by the lights kernel, resolved as for every other scene."""
    spec = scenes.lights_spec(24, 13)
    sample = R.render(ssaa_ref.spec_at(spec, 2), 3)
    want = ssaa_ref.resolve_ref(sample, 2, 24, 13)
    assert step_distance(want) > 1e-9
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3, samples=2)
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, 24, 13, "samples=2")
    rows = tiling.tile_rows(13, 2, 2, 1)
    tile = r.render_tile(scene, 2, 2, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 13, 24)[:, rows].reshape(3, -1))
    assert np.array_equal(r.render_tile(scene, out="u8").cpu().numpy(), ssaa_ref.to_u8(got, 24, 13))


def test_pinhole_perspective_camera(hip):
    spec = scenes.with_camera(scenes.lights_spec(37, 23), position=[2.5, 1.5, -1.5], target=[0, 0.3, 3], fov=50.0)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    origins, dirs = r.camera_rays(scene.camera)  # (tests/test_gpu_camera.py pins them to the restatement)
    assert origins is None
    eye = tuple(float(c) for c in spec["camera"]["position"])
    d = tuple(dirs.cpu().numpy())
    osc = O.scene_from_spec(spec)
    want = np.stack(R.trace(osc, R.table_of(spec), eye, d, 3))
    assert step_distance(want) > 1e-9
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, 37, 23, "pinhole")
    plain = np.stack(O.trace(osc, eye, d, 3))
    assert int((O.to_uint8(want, 37, 23) != O.to_uint8(plain, 37, 23)).any(axis=-1).sum()) > 100
    rows = tiling.tile_rows(23, 2, 3, 1)
    tile = r.render_tile(scene, 2, 3, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 23, 37)[:, rows].reshape(3, -1))


def test_explicit_rays_with_per_ray_origins(hip):
    """raytrace_scene on caller-supplied rays: a shared origin, and one origin per ray (the frame's own
    rays pulled back along their directions by varying amounts: the same hits from other origins)."""
    spec, cap, want, _ = frame("three")
    scene = scenes.build_scene(spec)
    osc = O.scene_from_spec(spec)
    cam = tuple(float(c) for c in osc.cam)
    d = np.stack(O.ray_directions(osc.cam, W, H))
    r = hip.HipRenderer(cap)
    dev = torch.from_numpy(d).cuda()
    got = r.raytrace_scene(scene.camera.position, hip.HipVector3D(dev[0], dev[1], dev[2]), scene)
    _check(got.data.cpu().numpy(), want, W, H, "explicit rays, shared origin")
    back = np.linspace(0.0, 0.5, d.shape[1])
    o = np.stack([cam[c] - d[c] * back for c in range(3)])
    want_o = np.stack(R.trace(osc, R.table_of(spec), tuple(o), tuple(d), cap))
    assert step_distance(want_o) > 1e-9
    odev = torch.from_numpy(o).cuda()
    got = r.raytrace_scene(hip.HipVector3D(odev[0], odev[1], odev[2]), hip.HipVector3D(dev[0], dev[1], dev[2]), scene)
    _check(got.data.cpu().numpy(), want_o, W, H, "explicit rays, per-ray origins")


def test_render_image_pipeline_writes_the_png_of_the_restatement(hip, tmp_path):
    from PIL import Image

    from python_ray_tracer_amd.application import render_image_pipeline

    spec, cap, want, _ = frame("three")
    out = tmp_path / "lights.png"
    render_image_pipeline(scenes.build_scene(spec), out, hip.HipRenderer(cap))
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), O.to_uint8(want, W, H))


def test_op_against_the_renderer(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    spec, cap, want, _ = frame("three")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S = r.scene_blob(scene)
    table = torch.from_numpy(lights.lights_table(scene.lights)).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    out = torch.ops.rt.trace_lights(blob, S, table, eye, dirs, cap, 1)
    assert torch.equal(out, full)
    out32 = torch.ops.rt.trace_lights(blob, S, table, eye.unsqueeze(1).expand(3, W * H).contiguous(), dirs, cap, 0)
    assert torch.equal(out32, full.to(torch.float32))
    u8 = torch.ops.rt.trace_lights(blob, S, table, eye, dirs, cap, 2, check=False)
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), O.to_uint8(want, W, H))
    empty = torch.ops.rt.trace_lights(blob, S, table, eye, dirs[:, :0].contiguous(), cap, 1)
    assert tuple(empty.shape) == (3, 0)
    with pytest.raises(RuntimeError, match="max_bounces"):
        torch.ops.rt.trace_lights(blob, S, table, eye, dirs, 17, 1)
    with pytest.raises(RuntimeError, match="lights"):
        torch.ops.rt.trace_lights(blob, S, table[:, :5].contiguous(), eye, dirs, cap, 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.rt.trace_lights(blob, S, table, eye, dirs.t().contiguous().t(), cap, 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_lights(blob, S, table.cpu(), eye, dirs, cap, 1)
    # a blob of another sphere count: every ray a miss, as in the other kernels
    miss = torch.ops.rt.trace_lights(blob, S - 1, table, eye, dirs, cap, 1, check=False)
    assert tuple(miss.shape) == (3, W * H) and not miss.any()
    with pytest.raises(RuntimeError):
        torch.ops.rt.trace_lights(blob, S - 1, table, eye, dirs, cap, 1)  # check=True reads the header


def test_a_last_light_of_intensity_zero_changes_nothing(hip):
    spec, cap, want, _ = frame("three")
    more = copy.deepcopy(spec)
    more["lights"].append({"kind": "point", "position": [-3.0, 4.0, -2.0], "intensity": 0.0, "color": [1.0, 0.5, 0.2]})
    r = hip.HipRenderer(cap)
    a = r.render(scenes.build_scene(spec)).data
    b = r.render(scenes.build_scene(more)).data
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert lights.lights_table(scenes.build_scene(more).lights).shape == (4, 6)


def test_a_plain_scene_keeps_its_path_and_the_table_is_part_of_a_render(hip):
    """Two plain PointLights: the second stays ignored, through today's kernels. And two multi-light scenes
    that differ only in a light the scene key does not hold give two frames from one renderer."""
    spec = scenes.readme_spec(W, H)
    two = copy.deepcopy(spec)
    two["lights"].append({"kind": "point", "position": [-1.33, 8.16, 7.23]})
    a, names = _render(hip, two, 3)
    b, _ = _render(hip, spec, 3)
    assert "rtx_trace_lights" not in names and np.array_equal(a, b)
    r = hip.HipRenderer(3)
    for k in (2, 3, 2):
        s = with_lights(spec, k)
        got = r.render(scenes.build_scene(s)).data.cpu().numpy()
        _check(got, frame("two" if k == 2 else "three")[2], W, H, f"{k} lights from one renderer")
