"""Triangle meshes against an analytic sphere in the same place, on the GPU.

    python tools/mesh_bench.py --out profiles/mesh_C2.json [--steps 20] [--cap 3]

The frame is ``scenes.mesh_spec(1920, 1080, level)``: the README scene (config C2) on a checkered quad, with
a torus and a smooth icosphere of ``level`` subdivisions, at levels 2, 4 and 6 (320 / 5,120 / 81,920
triangles in the icosphere; the quad and the torus add 1,026). Per reading, HIP events around every step, a
warm-up, the median and the interquartile range of ``--steps`` timed steps; the readings alternate by
rounds in one process:

* (m) ``render_tile`` of the mesh frame at each level: its rays generated (rtx_ray_directions) and traced by
  rtx_trace_mesh;
* (t) rtx_trace_mesh alone on the frame's rays generated once before, with the tables on the device: the
  kernel without the host's share of a render (the content digest of the meshes, about a millisecond per
  megabyte of vertices and faces, is taken per render and falls between (m)'s events);
* (s) ``render_tile`` of the README scene with an analytic sphere in the icosphere's place, the first light
  a ``ColoredPointLight`` of intensity 1, white: rtx_trace_lights, the path the renderer had before meshes;
* (p) the same frame with a plain ``PointLight`` through the camera launch.

Beside them: the host's table build per level (``meshes.mesh_table`` from the scene's shapes, its cache
emptied; one reading per level, the tree included), the table's size, and rays per pixel, counted by the
NumPy restatement (tests/mesh_ref.py: camera rays and traced reflections, not shadow rays) on the level-2
frame at 96 x 54; ns per ray divides a frame's time by pixels times that figure. No threshold is a pass
condition: the file records what the triangles cost.
"""

import argparse
import copy
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import environment, meshes, scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import _lib as L  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _eye_ptr  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402

LEVELS = (2, 4, 6)


def sphere_spec(W, H, colored):
    """The README scene with an analytic sphere where mesh_spec puts its icosphere."""
    spec = scenes.readme_spec(W, H)
    ico = scenes.mesh_spec(W, H)["meshes"][1]
    spec["spheres"].append({"center": ico["translation"], "radius": ico["scale"], "shader": copy.deepcopy(ico["shader"])})
    if colored:
        spec["lights"][0] = dict(spec["lights"][0], intensity=1.0)
    return spec


def rays_per_pixel(cap):
    from tests import mesh_ref as R

    c = R.Counts()
    R.render(scenes.mesh_spec(96, 54, 2), cap, counts=c)
    return c.rays / (96 * 54)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="the readings alternate in this many rounds")
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--label", default=None, help="a name for this build in the output (an A/B of two libraries)")
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.cap
    n = W * H
    r = HipRenderer(B)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
    sphere, plain = scenes.build_scene(sphere_spec(W, H, True)), scenes.build_scene(sphere_spec(W, H, False))
    steps = {"p_render_plain_sphere": lambda: r.render_tile(plain, out="u8", into=out),
             "s_render_lights_sphere": lambda: r.render_tile(sphere, out="u8", into=out)}
    host = {}
    first = scenes.build_scene(scenes.mesh_spec(W, H, LEVELS[0]))
    blob, S = r.scene_blob(first)  # (the spheres, the light and the camera: the same at every level)
    dirs = r.get_ray_directions(first.camera).data
    light = torch.tensor(environment.unit_light_table(first.lights[0]), device=r.device)
    ws = torch.zeros(int(r._lib.rtx_mesh_workspace_bytes(n, B)), dtype=torch.uint8, device=r.device)
    keep = [blob, dirs, light, ws, out]
    for level in LEVELS:
        scene = scenes.build_scene(scenes.mesh_spec(W, H, level))
        meshes._TABLES.clear()
        t0 = time.perf_counter()
        table = meshes.mesh_table(scene.shapes)
        host[f"level{level}"] = {"table_build_ms": round((time.perf_counter() - t0) * 1e3, 2),
                                 "triangles": int(table[meshes.MH_NTRI]), "nodes": int(table[meshes.MH_NNODES]),
                                 "table_bytes": int(table.nbytes)}
        t0 = time.perf_counter()
        meshes.mesh_table(scene.shapes)
        host[f"level{level}"]["table_cached_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        steps[f"m_render_level{level}"] = lambda scene=scene: r.render_tile(scene, out="u8", into=out)
        dev = torch.tensor(table, device=r.device)
        keep.append(dev)

        def trace(dev=dev):
            L.check(r._lib.rtx_trace_mesh(blob.data_ptr(), S, dev.data_ptr(), dev.numel(), light.data_ptr(), 1,
                                          _eye_ptr(blob), 0, dirs.data_ptr(), n, B, out.data_ptr(), L.OUT_U8_HWC,
                                          ws.data_ptr(), ws.numel(), r._stream()), "rtx_trace_mesh")

        steps[f"t_mesh_level{level}"] = trace
    for level in LEVELS:  # (the timed renders find every table cached)
        meshes.mesh_table(scenes.build_scene(scenes.mesh_spec(W, H, level)).shapes)
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    rpp = rays_per_pixel(B)
    res = {"scene": "mesh_spec", "width": W, "height": H, "pixels": n, "max_bounces": B, "label": a.label,
           "library": str(L.LIB_PATH.name), "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step (render_tile: the host's table lookup, the ray generation and the trace); "
                     "median and interquartile range of the timed steps; the readings alternate by rounds in one "
                     "process",
           "rays_per_pixel": round(rpp, 4),
           "rays_per_pixel_from": "tests/mesh_ref.py on mesh_spec(96, 54, 2): camera rays and traced reflections",
           "host": host, "readings": {name: summary(us) for name, us in times.items()}}
    med = {name: s["median_us"] for name, s in res["readings"].items()}
    res["derived"] = {
        "ns_per_ray": {name: round(us * 1e3 / (n * rpp), 4) for name, us in med.items() if name[:2] in ("m_", "t_")},
        "mesh_over_lights_sphere": {name: round(us / med["s_render_lights_sphere"], 3) for name, us in med.items()
                                    if name.startswith("m_")},
        "lights_sphere_over_plain_sphere": round(med["s_render_lights_sphere"] / med["p_render_plain_sphere"], 3),
    }
    for name, s in res["readings"].items():
        print(json.dumps({name: s}), flush=True)
    print(json.dumps({"host": host, "rays_per_pixel": res["rays_per_pixel"], "derived": res["derived"]}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "readings": len(res["readings"])}))


if __name__ == "__main__":
    main()
