"""The calls HipRenderer makes into the library, pinned entry for entry.

Parity tests compare pixels; they cannot see a dropped RTX_F_NO_GENERAL, a probe or dispatch order
that is no longer passed, an extra launch or another workspace size: the frame is the same and only
the time per step moves. Here the renderer's ``_lib`` is replaced by a proxy that forwards every call
and logs its name and arguments, a fixed script runs on the README scene at 16 x 8 (two 16 x 4 wave
tiles: the smallest frame with more than one dispatch unit) and, at its end, on the scenes that are traced
with a side table (glass, several lights, an environment, meshes), and the log must equal
tests/golden/host_calls.json. Integers and floats are logged as they are; whatever the entry point
declares as a pointer (a ``data_ptr()``, an address, a stream, a ctypes object) as 0 or 1 for null or
not. The device is synchronised after every step, so every probe event has landed before the next
call and the learnt state (deferred counts, dispatch orders, clean keys) is deterministic.

``RTX_RECORD_HOST_CALLS=1`` rewrites the fixture instead of comparing.
"""

import ctypes
import json
import numbers
import os

import numpy as np
import pytest
import torch

from python_ray_tracer_amd import scenes
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = GOLDEN / "host_calls.json"
W, H = 16, 8


def _is_pointer(ctype) -> bool:
    return ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer)


class _Recorder:
    """Stands in for the loaded library: every attribute is the library's function behind a logger."""

    def __init__(self, lib, log) -> None:
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            assert len(args) == len(fn.argtypes), (name, len(args))
            entry = [name]
            for a, t in zip(args, fn.argtypes):
                if _is_pointer(t):
                    entry.append(int(bool(a)))
                elif isinstance(a, numbers.Integral):
                    entry.append(int(a))
                else:
                    entry.append(float(a))
            self._log.append(entry)
            return fn(*args)

        return call


def _run_script(hip) -> list:
    log = []

    def renderer(*args, **kwargs):
        r = hip.HipRenderer(*args, **kwargs)
        r._lib = _Recorder(r._lib, log)
        return r

    def step(label, call):
        log.append("# " + label)
        out = call()
        torch.cuda.synchronize()
        return out

    spec = scenes.readme_spec(W, H)
    scene = scenes.build_scene(spec)
    moved = scenes.build_scene(scenes.with_camera(spec, [0.25, 0.2, -2]))
    pose = dict(position=[1.5, 1.0, -2.0], target=[0, 0.3, 3])
    pin = scenes.build_scene(scenes.with_camera(spec, **pose))
    lens = scenes.build_scene(scenes.with_camera(spec, **pose, lens_radius=0.05))
    eye = scene.camera.position

    # samples=1, capped: the probe, then the learnt order and RTX_F_NO_GENERAL
    r = renderer(3)
    for i in range(3):
        step(f"render_tile {i}", lambda: r.render_tile(scene))
    step("render_tile row tile", lambda: r.render_tile(scene, 4, 2, 1))
    into = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
    step("render_tile u8 into", lambda: r.render_tile(scene, out="u8", into=into))
    step("raytrace_scene lazy", lambda: r.raytrace_scene(eye, r.get_ray_directions(scene.camera), scene))
    step("render_batch", lambda: r.render_batch([scene, moved]))
    aovs = step("render_aovs", lambda: r.render_aovs(scene))
    rays = r.get_ray_directions(scene.camera)
    D = step("materialise", lambda: rays.data)
    step("raytrace_scene materialised", lambda: r.raytrace_scene(eye, rays, scene))
    step("trace_aovs", lambda: r.trace_aovs(eye, D, scene, passes=("depth", "lit")))
    m = aovs["id"] == 0
    Dm, tm = D[:, m].contiguous(), aovs["depth"][m]
    step("shade_hits own shader", lambda: r.shade_hits(scene.shapes[0], scene, eye, Dm, tm))
    step("shade_hits other shader",
         lambda: r.shade_hits(scene.shapes[0], scene, eye, Dm, tm, shader=scene.shapes[1].shader))
    step("perspective render_tile", lambda: r.render_tile(pin))
    step("perspective camera_rays", lambda: r.camera_rays(pin.camera))
    step("perspective render_aovs", lambda: r.render_aovs(pin))
    textured = scenes.readme_spec(W, H)
    texels = np.linspace(0.0, 1.0, 4 * 4 * 3).reshape(4, 4, 3)
    textured["spheres"][0]["shader"]["texture"] = {"kind": "image", "texels": texels}
    step("image texture", lambda: r.render_tile(scenes.build_scene(textured)))

    # uncapped: the status read-back, then the clean-key skip
    ru = renderer(None)
    for i in range(2):
        step(f"uncapped render_tile {i}", lambda: ru.render_tile(scene))

    r2 = renderer(3, samples=2)
    step("samples=2 render_tile", lambda: r2.render_tile(scene))
    step("samples=2 row tile", lambda: r2.render_tile(scene, 4, 2, 1))
    step("samples=2 render_batch", lambda: r2.render_batch([scene, moved]))
    step("samples=2 pinhole render_tile", lambda: r2.render_tile(pin))
    step("samples=2 lens render_tile", lambda: r2.render_tile(lens))
    step("samples=2 pinhole camera_rays", lambda: r2.camera_rays(pin.camera))
    step("samples=2 lens camera_rays", lambda: r2.camera_rays(lens.camera))

    ra = renderer(3, samples=2, adaptive=True)
    step("adaptive render", lambda: ra.render(scene))
    step("adaptive edge_mask", lambda: ra.edge_mask(scene))

    rs = renderer(3, collect_stats=True)
    step("collect_stats render_tile", lambda: rs.render_tile(scene))

    # the side-table scenes (glass, lights, environment, mesh): each twice, the second skips the status read-back
    glassy_env = scenes.env_spec(W, H, 8, 4)
    glassy_env["spheres"][1]["shader"].update(transmission_gain=0.9, diffuse_gain=0.1)
    tabled = {
        "glass": scenes.glass_spec(W, H),
        "lights": scenes.lights_spec(W, H),
        "env": scenes.env_spec(W, H, 8, 4),
        "glass env": glassy_env,
        "mesh": scenes.mesh_spec(W, H, 1),
        "mesh uv": scenes.textured_mesh_spec(W, H, 1, scenes.uv_grid_texels(4, 4)),
    }
    tabled = {name: scenes.build_scene(s) for name, s in tabled.items()}
    rt = renderer(3)
    for name, sc in tabled.items():
        for i in range(2):
            step(f"{name} render_tile {i}", lambda: rt.render_tile(sc))
    step("lights row tile", lambda: rt.render_tile(tabled["lights"], 4, 2, 1))
    mesh = tabled["mesh"]
    mesh_rays = rt.get_ray_directions(mesh.camera)
    step("mesh materialise", lambda: mesh_rays.data)
    step("mesh raytrace_scene materialised", lambda: rt.raytrace_scene(mesh.camera.position, mesh_rays, mesh))
    rt2 = renderer(3, samples=2)
    step("samples=2 glass render_tile", lambda: rt2.render_tile(tabled["glass"]))
    step("samples=2 mesh render_tile", lambda: rt2.render_tile(mesh))
    return log


def test_the_library_calls_of_a_fixed_script(hip_module):
    log = json.loads(json.dumps(_run_script(hip_module)))  # (tuples and lists alike, as the fixture holds them)
    if os.environ.get("RTX_RECORD_HOST_CALLS") == "1":
        FIXTURE.write_text("[\n" + ",\n".join(json.dumps(e) for e in log) + "\n]\n")
    want = json.loads(FIXTURE.read_text())
    for i, (got_e, want_e) in enumerate(zip(log, want)):
        assert got_e == want_e, (i, [e for e in log[:i] if isinstance(e, str)][-1:], got_e, want_e)
    assert len(log) == len(want), (len(log), len(want))


@pytest.fixture(scope="module")
def hip_module():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip

    return hip
