"""What image textures on meshes cost, on the GPU.

    python tools/meshuv_bench.py --out profiles/meshuv_C2.json [--steps 20] [--cap 3]

The frame is ``scenes.textured_mesh_spec(1920, 1080)``: the mesh frame of tools/mesh_bench.py (level 2) with
the procedural 64 x 64 image on its ground quad and on its torus. The baseline is the same spec with the
image replaced by a constant colour (the image's mean), which the renderer traces through the unchanged
rtx_trace_mesh in the same process. Per reading, HIP events around every step, a warm-up, the median and the
interquartile range of ``--steps`` timed steps; the readings alternate by rounds:

* (m) ``render_tile`` of the textured frame (rtx_trace_mesh_uv) and of the constant-colour frame
  (rtx_trace_mesh);
* (t) the two entries alone on the frame's rays generated once before, with the tables on the device; and
  rtx_trace_mesh_uv on the constant-colour scene's table, which has no UV part: the second compilation of the
  walk without one lookup (the header words are 0, every mesh material is a constant).

Beside them: the host's table build with and without the two new parts (``meshes.mesh_table``, its cache
emptied), the tables' sizes, and how many hits looked the image up, counted by the NumPy restatement
(tests/meshuv_ref.py) on the frame at 96 x 54. No threshold is a pass condition: the file records what the
lookup costs.
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


def constant_spec(spec):
    """``spec`` with every mesh's image replaced by the image's mean colour."""
    out = copy.deepcopy(spec)
    for m in out["meshes"]:
        tex = m["shader"]["texture"]
        if tex["kind"] == "image":
            m["shader"]["texture"] = scenes._const(*(float(c) for c in tex["texels"].reshape(-1, 3).mean(axis=0)))
    return out


def lookups(cap):
    from tests import meshuv_ref as U

    c = U.Counts()
    U.render(scenes.textured_mesh_spec(96, 54), cap, counts=c)
    return {"rays_per_pixel": round(c.rays / (96 * 54), 4),
            "textured_hits_per_pixel": round((c.tex_primary + c.tex_reflected) / (96 * 54), 4),
            "from": "tests/meshuv_ref.py on textured_mesh_spec(96, 54): camera rays and traced reflections; hits that "
                    "looked an image up, every level"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="the readings alternate in this many rounds")
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/meshuv_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.cap
    n = W * H
    r = HipRenderer(B)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
    spec = scenes.textured_mesh_spec(W, H)
    scene_of = {"textured": scenes.build_scene(spec), "constant": scenes.build_scene(constant_spec(spec))}
    blob, S = r.scene_blob(scene_of["textured"])  # (the spheres, the light and the camera: the same in both)
    dirs = r.get_ray_directions(scene_of["textured"].camera).data
    light = torch.tensor(environment.unit_light_table(scene_of["textured"].lights[0]), device=r.device)
    ws = torch.zeros(int(r._lib.rtx_mesh_workspace_bytes(n, B)), dtype=torch.uint8, device=r.device)
    host, dev, steps = {}, {}, {}
    for name, scene in scene_of.items():
        build = []
        for _ in range(5):
            meshes._TABLES.clear()
            t0 = time.perf_counter()
            table = meshes.mesh_table(scene.shapes)
            build.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        meshes.mesh_table(scene.shapes)
        host[name] = {"table_build_ms_median_of_5": round(sorted(build)[2], 2),
                      "table_cached_ms": round((time.perf_counter() - t0) * 1e3, 2),
                      "triangles": int(table[meshes.MH_NTRI]), "table_bytes": int(table.nbytes),
                      "uv_part_bytes": 8 * meshes.UV_WORDS * int(table[meshes.MH_NTRI]) if table[meshes.MH_UVS] else 0,
                      "texel_bytes": int(8 * (table.size - table[meshes.MH_TEXELS])) if table[meshes.MH_TEXELS] else 0}
        dev[name] = torch.tensor(table, device=r.device)
        steps[f"m_render_{name}"] = lambda scene=scene: r.render_tile(scene, out="u8", into=out)

    def trace(entry, table):
        fn = getattr(r._lib, entry)

        def step():
            L.check(fn(blob.data_ptr(), S, table.data_ptr(), table.numel(), light.data_ptr(), 1, _eye_ptr(blob), 0,
                       dirs.data_ptr(), n, B, out.data_ptr(), L.OUT_U8_HWC, ws.data_ptr(), ws.numel(), r._stream()), entry)
        return step

    steps["t_mesh_uv_textured"] = trace("rtx_trace_mesh_uv", dev["textured"])
    steps["t_mesh_constant"] = trace("rtx_trace_mesh", dev["constant"])
    steps["t_mesh_uv_constant"] = trace("rtx_trace_mesh_uv", dev["constant"])
    frames = {}
    for name, fn in steps.items():
        for _ in range(a.warmup):
            fn()
        frames[name] = out.clone()
    torch.cuda.synchronize()
    # the second compilation of the walk computes what the first computes where no image is looked up
    same = bool(torch.equal(frames["t_mesh_uv_constant"], frames["t_mesh_constant"]))
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    res = {"scene": "textured_mesh_spec", "width": W, "height": H, "pixels": n, "max_bounces": B,
           "library": str(L.LIB_PATH.name), "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step (render_tile: the host's table lookup, the ray generation and the trace); "
                     "median and interquartile range of the timed steps; the readings alternate by rounds in one "
                     "process",
           "counts": lookups(B), "host": host, "uv_entry_on_constant_table_gives_the_same_frame": same,
           "readings": {name: summary(us) for name, us in times.items()}}
    med = {name: s["median_us"] for name, s in res["readings"].items()}
    res["derived"] = {
        "render_textured_over_constant": round(med["m_render_textured"] / med["m_render_constant"], 4),
        "trace_textured_over_constant": round(med["t_mesh_uv_textured"] / med["t_mesh_constant"], 4),
        "trace_uv_build_over_plain_build_on_the_constant_table": round(med["t_mesh_uv_constant"] / med["t_mesh_constant"], 4),
    }
    for name, s in res["readings"].items():
        print(json.dumps({name: s}), flush=True)
    print(json.dumps({"host": host, "counts": res["counts"], "derived": res["derived"], "same_frame": same}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "readings": len(res["readings"])}))


if __name__ == "__main__":
    main()
