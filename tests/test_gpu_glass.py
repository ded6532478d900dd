"""Transmission on the GPU: scenes with glass spheres through HipRenderer and rt::trace_glass.

Every render is compared with the NumPy restatement (tests/glass_ref.py) at ATOL = 1e-12, the
project's bar for float64 colour (tests/test_gpu_parity.py: the kernels sum the same terms in another
association), and its uint8 frame must be identical. Which rays exist and what they hit are decisions
the kernel must take bit for bit like the restatement; a wrong one moves a pixel by far more than
1e-12. The floors (half the measured count of changed uint8 pixels, tests/test_glass_cpu.py) keep
equality with the plain render from passing: a renderer that ignores the gain fails every case.
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes, tiling
from tests import glass_ref as G
from tests import ssaa_ref
from tests.test_glass_cpu import CASES, frame

pytestmark = pytest.mark.gpu

ATOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _check(got, want, W, H, what=""):
    """float64 colour within ATOL of the restatement's, and the same uint8 frame."""
    err = float(np.abs(got - want).max())
    print(f"{what}: max |gpu - ref| = {err:.3e} (colours up to {want.max():.3f})")
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert err <= ATOL, (what, err)
    assert np.array_equal(O.to_uint8(got, W, H), O.to_uint8(want, W, H)), what


def _changed(a, b, W, H) -> int:
    return int((O.to_uint8(a, W, H) != O.to_uint8(b, W, H)).any(axis=-1).sum())


@pytest.mark.parametrize("key", sorted(CASES))
def test_frames_against_the_restatement(hip, key):
    spec, gains, cap, want, counts, changed = frame(key)
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    r = hip.HipRenderer(cap)
    got = r.render(scenes.build_scene(G.with_gains(spec, gains))).data.cpu().numpy()
    _check(got, want, W, H, key)
    plain = r.render(scenes.build_scene(spec)).data.cpu().numpy()
    moved = _changed(got, plain, W, H)
    print(f"{key}: {moved} uint8 pixels differ from the opaque render ({changed} in the restatement)")
    assert moved >= (changed + 1) // 2


def test_two_indices_of_refraction_and_gains(hip):
    spec = scenes.readme_spec(64, 36)
    gains, iors = [0.7, 0.4, 0.0], [1.33, 1.5, 1.5]
    want = G.render(spec, gains, iors, 3)
    r = hip.HipRenderer(3)
    got = r.render(scenes.build_scene(G.with_gains(spec, gains, iors))).data.cpu().numpy()
    _check(got, want, 64, 36, "ior 1.33 and 1.5")
    same_ior = G.render(spec, gains, [1.5] * 3, 3)
    assert _changed(want, same_ior, 64, 36) >= 140  # the index bends the rays: 1.33 is not 1.5 (280 measured)
    assert _changed(want, O.render(O.scene_from_spec(spec), 3), 64, 36) >= 218  # (436 measured)


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (67, 5)])
def test_frames_that_end_inside_a_wave(hip, size):
    W, H = size
    spec = scenes.main_spec(W, H)
    gains = [0.9, 0.9, 0.5]
    want = G.render(spec, gains, None, 3)
    got = hip.HipRenderer(3).render(scenes.build_scene(G.with_gains(spec, gains))).data.cpu().numpy()
    _check(got, want, W, H, f"main {size}")
    if size == (67, 5):
        assert _changed(want, O.render(O.scene_from_spec(spec), 3), W, H) >= 40  # (79 measured)


def test_a_scene_beyond_the_lds_table(hip):
    """200 spheres (above the 128 of the LDS table and the culling-tree threshold), every third glass."""
    spec = scenes.random_spec(200, 3, 48, 27)
    gains = [0.8 if i % 3 == 0 else 0.0 for i in range(201)]
    counts = G.Counts()
    want = G.render(spec, gains, None, 2, counts=counts)
    got = hip.HipRenderer(2).render(scenes.build_scene(G.with_gains(spec, gains))).data.cpu().numpy()
    _check(got, want, 48, 27, "rand200")
    # (123 transmitted rays and 91 changed pixels measured)
    assert counts.transmitted >= 60 and _changed(want, O.render(O.scene_from_spec(spec), 2), 48, 27) >= 45


def test_float32_and_uint8_outputs(hip):
    spec, gains, cap, want, _, changed = frame("readme")
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(G.with_gains(spec, gains))
    got = hip.HipRenderer(cap).render(scene).data.cpu().numpy()
    r32 = hip.HipRenderer(cap, color_dtype=torch.float32)
    got32 = r32.render(scene).data
    assert got32.dtype == torch.float32
    assert np.array_equal(got32.cpu().numpy(), got.astype(np.float32))  # the float64 value rounded once
    for r in (r32, hip.HipRenderer(cap)):
        u8 = r.render_tile(scene, out="u8")
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
        assert np.array_equal(u8.cpu().numpy(), O.to_uint8(want, W, H))
    into = torch.zeros((3, W * H), dtype=torch.float64, device=got32.device)
    assert hip.HipRenderer(cap).render_tile(scene, into=into) is into
    assert np.array_equal(into.cpu().numpy(), got)


def test_row_tiles_equal_the_rows_of_the_whole_frame(hip):
    spec, gains, cap, want, _, _ = frame("readme")
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(G.with_gains(spec, gains))
    r = hip.HipRenderer(cap)
    full = r.render(scene).data.cpu().numpy().reshape(3, H, W)
    full_u8 = r.render_tile(scene, out="u8").cpu().numpy()
    rb, P = 4, 3  # 54 rows: 4 whole cycles of 12 and a partial one
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
    # a tile is the restatement's rows, too
    rows = tiling.tile_rows(H, rb, P, 1, 2)
    _check(r.render_tile(scene, rb, P, 1, part_run=2).cpu().numpy(), G.render(spec, gains, None, cap, rows=rows), W,
           len(rows), "rows of parts 1-2")


def test_explicit_rays_with_per_ray_origins(hip):
    """raytrace_scene on caller-supplied rays: a shared origin, and one origin per ray (the frame's own
    rays pulled back along their directions by varying amounts: the same hits from other origins)."""
    spec, gains, cap, want, _, _ = frame("main")
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(G.with_gains(spec, gains))
    osc, g, iors = G.scene_of(spec, gains)
    cam = tuple(float(c) for c in osc.cam)
    d = np.stack(O.ray_directions(osc.cam, W, H))
    r = hip.HipRenderer(cap)
    dev = torch.from_numpy(d).cuda()
    got = r.raytrace_scene(scene.camera.position, hip.HipVector3D(dev[0], dev[1], dev[2]), scene)
    _check(got.data.cpu().numpy(), want, W, H, "explicit rays, shared origin")
    back = np.linspace(0.0, 0.5, d.shape[1])
    o = np.stack([cam[c] - d[c] * back for c in range(3)])
    want_o = np.stack(G.trace(osc, g, iors, tuple(o), tuple(d), cap))
    odev = torch.from_numpy(o).cuda()
    got = r.raytrace_scene(hip.HipVector3D(odev[0], odev[1], odev[2]), hip.HipVector3D(dev[0], dev[1], dev[2]), scene)
    _check(got.data.cpu().numpy(), want_o, W, H, "explicit rays, per-ray origins")
    assert _changed(want_o, np.stack(O.trace(O.scene_from_spec(spec), tuple(o), tuple(d), cap)), W, H) >= 420  # (840 measured)


def test_pinhole_perspective_camera(hip):
    spec = scenes.with_camera(scenes.main_spec(37, 23), position=[2.5, 1.5, -1.5], target=[0, 0.3, 3], fov=50.0)
    gains = [0.9, 0.9, 0.0]
    scene = scenes.build_scene(G.with_gains(spec, gains))
    r = hip.HipRenderer(3)
    origins, dirs = r.camera_rays(scene.camera)  # (tests/test_gpu_camera.py pins them to the restatement)
    assert origins is None
    osc, g, iors = G.scene_of(spec, gains)
    eye = tuple(float(c) for c in spec["camera"]["position"])
    d = tuple(dirs.cpu().numpy())
    want = np.stack(G.trace(osc, g, iors, eye, d, 3))
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, 37, 23, "pinhole")
    assert _changed(want, np.stack(O.trace(O.scene_from_spec(spec), eye, d, 3)), 37, 23) >= 50
    rows = tiling.tile_rows(23, 2, 3, 1)
    tile = r.render_tile(scene, 2, 3, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 23, 37)[:, rows].reshape(3, -1))


def test_supersampled_frame(hip):
    """samples=2: the sample frame traced by the glass kernel, resolved as for every other scene."""
    spec = scenes.readme_spec(48, 27)
    gains = [0.9, 0.9, 0.0]
    sample = G.render(ssaa_ref.spec_at(spec, 2), gains, None, 3)
    want = ssaa_ref.resolve_ref(sample, 2, 48, 27)
    scene = scenes.build_scene(G.with_gains(spec, gains))
    r = hip.HipRenderer(3, samples=2)
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, 48, 27, "samples=2")
    plain = ssaa_ref.resolve_ref(O.render(O.scene_from_spec(ssaa_ref.spec_at(spec, 2)), 3), 2, 48, 27)
    assert _changed(want, plain, 48, 27) >= 120  # (243 measured)
    rows = tiling.tile_rows(27, 2, 2, 1)
    tile = r.render_tile(scene, 2, 2, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 27, 48)[:, rows].reshape(3, -1))
    u8 = r.render_tile(scene, out="u8").cpu().numpy()
    assert np.array_equal(u8, ssaa_ref.to_u8(got, 48, 27))


def test_shaders_without_the_attribute(hip):
    """Shaders that lack transmission_gain (the reference's own NumpyShader objects) render bit for bit
    like the same scene with the attribute at 0.0, through the opaque path."""
    spec = scenes.readme_spec(50, 22)
    with_attr = scenes.build_scene(spec)
    without = scenes.build_scene(spec)
    for s in without.shapes:
        del s.shader.transmission_gain
        assert not hasattr(s.shader, "transmission_gain")
    assert all(s.shader.transmission_gain == 0.0 for s in with_attr.shapes)
    r = hip.HipRenderer(3)
    a, b = r.render(with_attr).data, r.render(without).data
    assert torch.equal(a, b)
    assert np.abs(a.cpu().numpy() - O.render(O.scene_from_spec(spec), 3)).max() <= ATOL
    # one shader with the attribute, the others without
    without.shapes[1].shader.transmission_gain = 0.9
    want = G.render(spec, [0.0, 0.9, 0.0], None, 3)
    _check(r.render(without).data.cpu().numpy(), want, 50, 22, "one attribute")


def test_op_against_the_renderer(hip):
    import python_ray_tracer_amd.ops  # noqa: F401
    from python_ray_tracer_amd import glass

    spec, gains, cap, want, _, _ = frame("readme")
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(G.with_gains(spec, gains))
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S = r.scene_blob(scene)
    table = torch.from_numpy(glass.glass_table(scene.shapes)).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    out = torch.ops.rt.trace_glass(blob, S, table, eye, dirs, cap, 1)
    assert torch.equal(out, full)
    out32 = torch.ops.rt.trace_glass(blob, S, table, eye.unsqueeze(1).expand(3, W * H).contiguous(), dirs, cap, 0)
    assert torch.equal(out32, full.to(torch.float32))
    u8 = torch.ops.rt.trace_glass(blob, S, table, eye, dirs, cap, 2, check=False)
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), O.to_uint8(want, W, H))
    # a table of zero gains through the glass kernel: the opaque frame within the bar
    zero = torch.zeros_like(table)
    zero[1] = 1.5
    plain = torch.ops.rt.trace_glass(blob, S, zero, eye, dirs, cap, 1).cpu().numpy()
    assert np.abs(plain - O.render(O.scene_from_spec(spec), cap)).max() <= ATOL
    empty = torch.ops.rt.trace_glass(blob, S, table, eye, dirs[:, :0].contiguous(), cap, 1)
    assert tuple(empty.shape) == (3, 0)
    with pytest.raises(RuntimeError, match="max_bounces"):
        torch.ops.rt.trace_glass(blob, S, table, eye, dirs, 9, 1)
    with pytest.raises(RuntimeError, match="glass"):
        torch.ops.rt.trace_glass(blob, S, table[:, :2].contiguous(), eye, dirs, cap, 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.rt.trace_glass(blob, S, table, eye, dirs.t().contiguous().t(), cap, 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_glass(blob, S, table.cpu(), eye, dirs, cap, 1)


def test_refusals(hip):
    spec, gains, cap, _, _, _ = frame("readme")
    scene = scenes.build_scene(G.with_gains(spec, gains))
    plain = scenes.build_scene(spec)
    with pytest.raises(ValueError, match="finite bounce cap"):
        hip.HipRenderer().render(scene)
    with pytest.raises(ValueError, match="max_bounces in 0..8"):
        hip.HipRenderer(9).render(scene)
    hip.HipRenderer(9).render(plain)  # (an opaque scene: any cap)
    r = hip.HipRenderer(3)
    with pytest.raises(ValueError, match="render_batch.*transmissive"):
        r.render_batch([plain, scene])
    with pytest.raises(ValueError, match="submit_tiles.*transmissive"):
        r.submit_tiles(None, 0, scene, 1, 1, 0, None)
    blob, S = r.scene_blob(scene)
    with pytest.raises(ValueError, match="blob.*transmissive"):
        r.render_tile(scene, blob=blob, n_spheres=S)
    o = scene.camera.position
    d = hip.HipVector3D(np.array([0.0]), np.array([0.0]), np.array([1.0]))
    with pytest.raises(ValueError, match="shade_hits.*transmissive"):
        r.shade_hits(scene.shapes[0], scene, o, d, np.array([1.0]))
    with pytest.raises(ValueError, match="shade_hits.*transmissive"):
        scene.shapes[0].shader.create(scene.shapes[0], scene, o, d, np.array([1.0]), ray_tracer=r)
    with pytest.raises(ValueError, match="shade_hits.*transmissive"):  # an opaque scene, a transmissive shader
        r.shade_hits(plain.shapes[0], plain, o, d, np.array([1.0]), shader=scene.shapes[1].shader)
    with pytest.raises(ValueError, match="adaptive"):
        hip.HipRenderer(3, samples=2, adaptive=True).render(scene)
    for bad, what in ((-0.5, "transmission_gain"), (float("nan"), "transmission_gain"), ("0.5", "transmission_gain")):
        broken = scenes.build_scene(G.with_gains(spec, [0.0, bad, 0.0]))
        with pytest.raises(ValueError, match=what):
            r.render(broken)
    for bad in (0.9, float("inf")):
        broken = scenes.build_scene(G.with_gains(spec, gains, [1.5, bad, 1.5]))
        with pytest.raises(ValueError, match="specular_ior"):
            r.render(broken)
    # the passes look at the primary hit only and stay as they are
    a = r.render_aovs(scene, ("id",))["id"]
    assert torch.equal(a, r.render_aovs(plain, ("id",))["id"])
    assert set(r.render_occlusion(scene, side=1)) == {"ao", "soft_lit"}
