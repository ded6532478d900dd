"""The environment map on the GPU: environment scenes through HipRenderer and the three ops.

Every render is compared with the NumPy restatement (tests/env_ref.py) at the project's bar for float64
colour, |GPU - restatement| <= 1e-12 * max(1, |colour|), and its uint8 frame must be identical, no pixel
excluded: tests/test_env_cpu.py checks that no pixel of a case sits within 1e-9 of a quantisation step.
The lookup is bilinear, so the few ulp between the device's atan2 / asin and NumPy's move a colour by
about as much (images of 64 x 32 or smaller; the drift grows with the image's width). Each frame case
also has to differ from the same render without the EnvironmentLight on at least half the pinned
count of changed pixels: a renderer that ignores the light fails every case. Nothing here provokes an
overflow of a lane's stack: the walk is the lights kernel's (one text, rtx_lights_walk.inc), whose stack
tests/test_gpu_lights_limits.py fills to its last entry and one over.
"""

import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import environment, glass, scenes, tiling
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import env_ref as E
from tests import ssaa_ref
from tests.test_env_cpu import (EDGE_DIRS, ENV, PINHOLE_MISSES, PINNED, H, W, changed, edge_dirs, frame,
                                pinhole_dirs, pinhole_spec)
from tests.test_gpu_lights import _Calls
from tests.test_lights_cpu import pool, step_distance

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


def _render(hip, spec, cap, **kw):
    r = hip.HipRenderer(cap, **kw)
    r._lib = calls = _Calls(r._lib)
    return r.render(scenes.build_scene(spec)).data.cpu().numpy(), calls.names


def _unit_dirs(n, seed=7):
    d = np.random.default_rng(seed).normal(size=(3, n))
    return d / np.sqrt((d * d).sum(axis=0))


# ---- the sampler ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (5, 3), (16, 8), (64, 32)])
def test_env_sample_against_the_restatement(hip, size):
    import python_ray_tracer_amd.ops  # noqa: F401

    w, h = size
    t = ENV.texels if size == (16, 8) else np.random.default_rng(w * 100 + h).uniform(0, 2, (h, w, 3)).astype(np.float32)
    env = E.Env(t, ENV.gain, ENV.rotation)
    light = scenes.build_scene(E.with_env(scenes.readme_spec(W, H), env)).lights[2]
    texels = torch.tensor(light.texels).cuda()
    gain, turn = environment.env_params(light)
    d = np.concatenate([_unit_dirs(4096), edge_dirs()], axis=1)
    want = np.stack(E.sample(env, tuple(d)))
    dev = torch.from_numpy(d).cuda()
    got = torch.ops.rt.env_sample(texels, list(gain), turn, dev).cpu().numpy()
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"env_sample {w} x {h}: max error {err:.3e}")
    assert np.isfinite(got).all() and err <= RTOL
    assert not got[:, 4096 + len(EDGE_DIRS):].any()  # the NaN directions give zeros
    assert got[:, :4096].max() > 0.5
    for n in (1, 63, 65):
        part = torch.ops.rt.env_sample(texels, list(gain), turn, dev[:, :n].contiguous()).cpu().numpy()
        assert np.array_equal(part, got[:, :n]), n
    assert tuple(torch.ops.rt.env_sample(texels, list(gain), turn, dev[:, :0].contiguous()).shape) == (3, 0)


def test_sample_environment_is_the_op(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    scene = scenes.build_scene(frame("readme")[0])
    r = hip.HipRenderer(3)
    d = _unit_dirs(300, seed=11)
    dev = torch.from_numpy(d).cuda()
    got = r.sample_environment(scene, hip.HipVector3D(dev[0], dev[1], dev[2]))
    light = scene.lights[2]
    gain, turn = environment.env_params(light)
    assert torch.equal(got, torch.ops.rt.env_sample(torch.tensor(light.texels).cuda(), list(gain), turn, dev))
    assert torch.equal(got, r.sample_environment(scene, tuple(d)))  # host arrays too
    assert list(r._env_images) == [light.digest]  # uploaded once
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.rt.env_sample(torch.tensor(light.texels).cuda(), list(gain), turn, dev.t().contiguous().t())


# ---- frames -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["readme", "main", "rand17", "rand65", "lights3", "1x1", "7x5", "67x5"])
def test_frames_against_the_restatement(hip, key):
    spec, cap, want, c, base = frame(key)
    w, h = spec["camera"]["width"], spec["camera"]["height"]
    got, names = _render(hip, spec, cap)
    assert names.count("rtx_trace_lights_env") == 1 and "rtx_trace_lights" not in names
    assert not any(n.startswith("rtx_render_camera") for n in names)
    _check(got, want, w, h, key)
    without, plain_names = _render(hip, E.plain(spec), cap)
    assert not any(n.endswith("_env") for n in plain_names)
    assert 2 * changed(got, without, w, h) >= PINNED[key][1] > 0


def test_the_readme_frame_at_cap_zero_is_the_sampler_where_it_misses(hip):
    """The 355 pixels whose ray meets nothing are env_sample of their directions; the rest are the
    environment-less frame: equal (==) to it as rtx_trace_lights renders it (the same walk, under a
    ColoredPointLight of intensity 1 and white), and within the bar of it as the camera launch renders it
    (another kernel, which sums a hit's terms in another association)."""
    spec, cap, want, c, base = frame("readme0")
    assert cap == 0
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(0)
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, W, H, "readme, cap 0")
    without = hip.HipRenderer(0).render(scenes.build_scene(E.plain(spec))).data.cpu().numpy()
    osc = O.scene_from_spec(E.plain(spec))
    d = np.stack(O.ray_directions(osc.cam, W, H))
    miss = ~without.any(axis=0)  # (a hit's colour holds the ambient 0.004)
    assert int(miss.sum()) == PINNED["readme0"][0][0] == 355
    sampled = r.sample_environment(scene, tuple(d[:, miss])).cpu().numpy()
    err = float((np.abs(got[:, miss] - sampled) / np.maximum(1.0, np.abs(sampled))).max())
    assert err <= RTOL
    hit_err = float((np.abs(got[:, ~miss] - without[:, ~miss]) / np.maximum(1.0, np.abs(without[:, ~miss]))).max())
    assert hit_err <= RTOL
    unit = E.plain(spec)
    unit["lights"][0]["intensity"] = 1.0
    same_walk, names = _render(hip, unit, 0)
    assert names.count("rtx_trace_lights") == 1
    assert np.array_equal(got[:, ~miss], same_walk[:, ~miss]) and not same_walk[:, miss].any()
    assert 2 * changed(got, without, W, H) >= PINNED["readme0"][1]


def test_glass_under_the_environment(hip):
    spec, cap, want, c, base = frame("glass")
    assert c.transmitted_misses == 296
    got, names = _render(hip, spec, cap)
    assert names.count("rtx_trace_glass_env") == 1 and "rtx_trace_glass" not in names and "rtx_trace_lights_env" not in names
    _check(got, want, W, H, "glass")
    without, plain_names = _render(hip, E.plain(spec), cap)
    assert plain_names.count("rtx_trace_glass") == 1 and not any(n.endswith("_env") for n in plain_names)
    _check(without, base, W, H, "glass without the environment")
    assert 2 * changed(got, without, W, H) >= PINNED["glass"][1]


def test_pinhole_perspective_camera_pitched_up(hip):
    spec = pinhole_spec()
    full = E.with_env(spec, ENV)
    scene = scenes.build_scene(full)
    r = hip.HipRenderer(3)
    origins, dirs = r.camera_rays(scene.camera)  # (tests/test_gpu_camera.py pins them to the restatement)
    assert origins is None
    d = dirs.cpu().numpy()
    assert np.abs(d - pinhole_dirs(spec)).max() <= 1e-15
    eye = tuple(float(c) for c in spec["camera"]["position"])
    counts = E.Counts()
    want = np.stack(E.trace(O.scene_from_spec(spec), E.unit_table(spec), eye, tuple(d), 3, ENV, counts))
    assert counts.misses == PINHOLE_MISSES and 2 * counts.misses[0] > 37 * 23 and step_distance(want) > 1e-9
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, 37, 23, "pinhole")
    without = r.render(scenes.build_scene(spec)).data.cpu().numpy()
    assert 2 * changed(got, without, 37, 23) >= changed(want, without, 37, 23) > 600
    rows = tiling.tile_rows(23, 2, 3, 1)
    tile = r.render_tile(scene, 2, 3, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 23, 37)[:, rows].reshape(3, -1))


def test_a_frame_larger_than_the_pool_of_workers(hip):
    """640 x 360 at cap 0: 230,400 rays for a pool of 196,608 workers (read from
    rtx_lights_workspace_bytes), so some workers take a second item. Equal to the same frame in row tiles,
    none of which reaches a second lap, bit for bit; 16 rows against the restatement."""
    w, h = 640, 360
    spec = E.with_env(scenes.readme_spec(w, h), ENV)
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
    assert len(rows) == 16 and sum(row * w >= p for row in rows) >= 2  # rows of the second lap are among them
    want = E.render(spec, ENV, 0, rows=rows)
    assert step_distance(want) > 1e-9
    _check(full[:, rows].reshape(3, -1), want, w, len(rows), "rows of the 640x360 frame")
    assert int((want[:, :w] != 0).all(axis=0).sum()) == w  # the top row is sky: the environment's


def test_row_tiles_runs_and_outputs(hip):
    spec, cap, want, _, _ = frame("readme")
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data.cpu().numpy()
    _check(full, want, W, H, "readme")
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
    """samples=2: the sample frame traced by the environment kernel, resolved as for every other scene."""
    spec = scenes.readme_spec(24, 13)
    sample = E.render(ssaa_ref.spec_at(spec, 2), ENV, 3)
    want = ssaa_ref.resolve_ref(sample, 2, 24, 13)
    assert step_distance(want) > 1e-9
    scene = scenes.build_scene(E.with_env(spec, ENV))
    r = hip.HipRenderer(3, samples=2)
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, 24, 13, "samples=2")
    without = r.render(scenes.build_scene(spec)).data.cpu().numpy()
    assert changed(got, without, 24, 13) > 150
    rows = tiling.tile_rows(13, 2, 2, 1)
    tile = r.render_tile(scene, 2, 2, 1).cpu().numpy()
    assert np.array_equal(tile, got.reshape(3, 13, 24)[:, rows].reshape(3, -1))
    assert np.array_equal(r.render_tile(scene, out="u8").cpu().numpy(), ssaa_ref.to_u8(got, 24, 13))


def test_explicit_rays_with_per_ray_origins(hip):
    spec, cap, want, _, _ = frame("readme")
    scene = scenes.build_scene(spec)
    osc = O.scene_from_spec(E.plain(spec))
    cam = tuple(float(c) for c in osc.cam)
    d = np.stack(O.ray_directions(osc.cam, W, H))
    r = hip.HipRenderer(cap)
    dev = torch.from_numpy(d).cuda()
    got = r.raytrace_scene(scene.camera.position, hip.HipVector3D(dev[0], dev[1], dev[2]), scene)
    _check(got.data.cpu().numpy(), want, W, H, "explicit rays, shared origin")
    back = np.linspace(0.0, 0.5, d.shape[1])
    o = np.stack([cam[c] - d[c] * back for c in range(3)])
    want_o = np.stack(E.trace(osc, E.unit_table(E.plain(spec)), tuple(o), tuple(d), cap, ENV))
    assert step_distance(want_o) > 1e-9
    odev = torch.from_numpy(o).cuda()
    got = r.raytrace_scene(hip.HipVector3D(odev[0], odev[1], odev[2]), hip.HipVector3D(dev[0], dev[1], dev[2]), scene)
    _check(got.data.cpu().numpy(), want_o, W, H, "explicit rays, per-ray origins")


def test_render_image_pipeline_writes_the_png_of_the_restatement(hip, tmp_path):
    from PIL import Image

    from python_ray_tracer_amd.application import render_image_pipeline

    spec, cap, want, _, _ = frame("readme")
    out = tmp_path / "env.png"
    render_image_pipeline(scenes.build_scene(spec), out, hip.HipRenderer(cap))
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), O.to_uint8(want, W, H))


# ---- the ops ----------------------------------------------------------------------------------------------------

def _op_inputs(hip, key):
    spec, cap, want, _, _ = frame(key)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S = r.scene_blob(scene)
    light = environment.environment_of(scene.lights)
    gain, turn = environment.env_params(light)
    texels = torch.tensor(light.texels).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    return scene, cap, want, r, full, blob, S, texels, list(gain), turn, dirs, eye


def test_lights_op_against_the_renderer(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    scene, cap, want, r, full, blob, S, texels, gain, turn, dirs, eye = _op_inputs(hip, "readme")
    table = torch.from_numpy(environment.unit_light_table(scene.lights[0])).cuda()
    op = torch.ops.rt.trace_lights_env
    assert torch.equal(op(blob, S, table, eye, dirs, cap, 1, texels, gain, turn), full)
    out32 = op(blob, S, table, eye.unsqueeze(1).expand(3, W * H).contiguous(), dirs, cap, 0, texels, gain, turn)
    assert torch.equal(out32, full.to(torch.float32))
    u8 = op(blob, S, table, eye, dirs, cap, 2, texels, gain, turn, check=False)
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), O.to_uint8(want, W, H))
    assert tuple(op(blob, S, table, eye, dirs[:, :0].contiguous(), cap, 1, texels, gain, turn).shape) == (3, 0)
    with pytest.raises(RuntimeError, match="max_bounces"):
        op(blob, S, table, eye, dirs, 17, 1, texels, gain, turn)
    with pytest.raises(RuntimeError, match="texels"):
        op(blob, S, table, eye, dirs, cap, 1, texels[:, :, :3].contiguous(), gain, turn)
    with pytest.raises(RuntimeError, match="contiguous"):
        op(blob, S, table, eye, dirs, cap, 1, texels.transpose(0, 1), gain, turn)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        op(blob, S, table, eye, dirs, cap, 1, texels.cpu(), gain, turn)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        op(blob, S, table, eye, dirs, cap, 1, torch.zeros(8 * 16 * 4 + 1, device="cuda")[1:].view(8, 16, 4), gain, turn)
    # a blob of another sphere count: every ray a miss, so the frame is the sampler's
    miss = op(blob, S - 1, table, eye, dirs, cap, 1, texels, gain, turn, check=False)
    sampled = torch.ops.rt.env_sample(texels, gain, turn, dirs)
    assert torch.equal(miss, sampled) and bool(sampled.any())
    with pytest.raises(RuntimeError):
        op(blob, S - 1, table, eye, dirs, cap, 1, texels, gain, turn)  # check=True reads the header
    # under the three lights' table the op is the renderer's frame of that scene
    scene3, cap3, _, _, full3, blob3, S3, texels3, gain3, turn3, dirs3, eye3 = _op_inputs(hip, "lights3")
    from python_ray_tracer_amd import lights

    table3 = torch.from_numpy(lights.lights_table(scene3.lights)).cuda()
    assert table3.shape == (3, 6)
    assert torch.equal(op(blob3, S3, table3, eye3, dirs3, cap3, 1, texels3, gain3, turn3), full3)


def test_glass_op_against_the_renderer(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    scene, cap, want, r, full, blob, S, texels, gain, turn, dirs, eye = _op_inputs(hip, "glass")
    table = torch.from_numpy(glass.glass_table(scene.shapes)).cuda()
    op = torch.ops.rt.trace_glass_env
    assert torch.equal(op(blob, S, table, eye, dirs, cap, 1, texels, gain, turn), full)
    u8 = op(blob, S, table, eye, dirs, cap, 2, texels, gain, turn, check=False)
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), O.to_uint8(want, W, H))
    assert tuple(op(blob, S, table, eye, dirs[:, :0].contiguous(), cap, 0, texels, gain, turn).shape) == (3, 0)
    with pytest.raises(RuntimeError, match="max_bounces"):
        op(blob, S, table, eye, dirs, 9, 1, texels, gain, turn)
    with pytest.raises(RuntimeError, match="gain"):
        op(blob, S, table, eye, dirs, cap, 1, texels, gain[:2], turn)
    miss = op(blob, S - 1, table[:, :S - 1].contiguous(), eye, dirs, cap, 1, texels, gain, turn, check=False)
    assert torch.equal(miss, torch.ops.rt.env_sample(texels, gain, turn, dirs))


# ---- routing ----------------------------------------------------------------------------------------------------

def test_an_environment_of_intensity_zero_equals_the_scene_without_it(hip):
    """... rendered through rtx_trace_lights: under a ColoredPointLight of intensity 1 and white, the
    parent's kernel with the one-row table."""
    spec, cap, _, _, _ = frame("readme")
    dark = copy.deepcopy(spec)
    dark["lights"][2]["intensity"] = 0.0
    got, names = _render(hip, dark, cap)
    assert names.count("rtx_trace_lights_env") == 1
    unit = E.plain(spec)
    unit["lights"][0]["intensity"] = 1.0
    want, unit_names = _render(hip, unit, cap)
    assert unit_names.count("rtx_trace_lights") == 1 and "rtx_trace_lights_env" not in unit_names
    assert (got == want).all()


def test_which_entry_a_render_goes_through(hip):
    """A scene without an EnvironmentLight makes the camera launch and no _env call, and the reverse; two
    environment scenes that differ only in what the scene key does not hold give two frames from one
    renderer, and the image is uploaded once."""
    spec, cap, want, _, _ = frame("readme")
    _, names = _render(hip, E.plain(spec), cap)
    assert any(n.startswith("rtx_render_camera") for n in names) and not any(n.endswith("_env") for n in names)
    _, names = _render(hip, spec, cap)
    assert [n for n in names if n.endswith("_env")] == ["rtx_trace_lights_env"]
    assert not any(n.startswith("rtx_render_camera") for n in names)
    r = hip.HipRenderer(cap)
    turned = copy.deepcopy(spec)
    turned["lights"][2]["rotation"] = 0.0
    want_turned = E.render(E.plain(spec), E.Env(ENV.texels, ENV.gain, 0.0), cap)
    for s, w in ((spec, want), (turned, want_turned), (spec, want)):
        _check(r.render(scenes.build_scene(s)).data.cpu().numpy(), w, W, H, "one renderer, two rotations")
    assert len(r._env_images) == 1
    # a second plain PointLight stays ignored under the environment too
    two = copy.deepcopy(spec)
    two["lights"].insert(1, {"kind": "point", "position": [-1.33, 8.16, 7.23]})
    assert np.array_equal(r.render(scenes.build_scene(two)).data.cpu().numpy(),
                          r.render(scenes.build_scene(spec)).data.cpu().numpy())


def test_c_abi_struct_layout_on_the_device(hip):
    """rtx_env_sample through ctypes with the struct _lib declares: the layout the library reads."""
    light = scenes.build_scene(frame("readme")[0]).lights[2]
    gain, turn = environment.env_params(light)
    texels = torch.tensor(light.texels).cuda()
    d = _unit_dirs(130, seed=3)
    dev = torch.from_numpy(d).cuda()
    out = torch.empty_like(dev)
    env = L.Env(texels.data_ptr(), 16, 8, (ctypes.c_double * 3)(*gain), turn)
    lib = L.load()
    L.check(lib.rtx_env_sample(ctypes.byref(env), dev.data_ptr(), 130, out.data_ptr(), L.stream_handle()), "rtx_env_sample")
    torch.cuda.synchronize()
    want = np.stack(E.sample(ENV, tuple(d)))
    assert float((np.abs(out.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))).max()) <= RTOL
