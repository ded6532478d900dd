"""The primary-hit render passes of a mesh scene against the colour path, on the GPU.

    python tools/mesh_aov_bench.py --out profiles/mesh_aov_C2.json [--steps 20]

The frame is ``scenes.mesh_spec(1920, 1080, level)`` at levels 2, 4 and 6 (tools/mesh_bench.py's frames), its
rays generated once before and its tables on the device, so every reading is one kernel launch. Per reading,
HIP events around every step, a warm-up, the median and the interquartile range of ``--steps`` timed steps;
the readings alternate by rounds in one process:

* (a) rtx_mesh_aovs with all ten passes;
* (b) ``depth`` and ``id`` alone: the two walks, no hit point, no shadow walk;
* (c) (b) and ``lit``: the shadow walks on top;
* (d) what a caller had before: rtx_trace_mesh of the same rays at ``max_bounces=0`` into a float64 frame.

Derived: the bytes (a) writes per pixel and its TB/s, and (b) against (d): (b) does strictly less, so it should
sit below (d) by more than both interquartile ranges. No threshold is a pass condition: the file records what
the passes cost.
"""

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import environment, meshes, scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import MESH_AOV_NAMES, HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import _lib as L  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _eye_ptr  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402

LEVELS = (2, 4, 6)
# bytes per ray of each pass, in MESH_AOV_NAMES' order
BYTES = dict(zip(MESH_AOV_NAMES, (8, 4, 4, 24, 24, 24, 24, 1, 4, 16)))
CASES = {"a_all_ten": MESH_AOV_NAMES, "b_depth_id": ("depth", "id"), "c_depth_id_lit": ("depth", "id", "lit")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="the readings alternate in this many rounds")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--label", default=None, help="a name for this build in the output (an A/B of two libraries)")
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_aov_bench.py measures on the GPU; none found")
    W, H = a.width, a.height
    n = W * H
    r = HipRenderer(0)
    first = scenes.build_scene(scenes.mesh_spec(W, H, LEVELS[0]))
    blob, S = r.scene_blob(first)  # (the spheres, the light and the camera: the same at every level)
    dirs = r.get_ray_directions(first.camera).data
    light = torch.tensor(environment.unit_light_table(first.lights[0]), device=r.device)
    ids = torch.tensor(meshes.shape_ids(first.shapes), device=r.device)
    ws = torch.zeros(int(r._lib.rtx_mesh_workspace_bytes(n, 0)), dtype=torch.uint8, device=r.device)
    colour = torch.empty((3, n), dtype=torch.float64, device=r.device)
    shapes = {"depth": ((n,), torch.float64), "id": ((n,), torch.int32), "hits": ((n,), torch.int32),
              "position": ((3, n), torch.float64), "normal": ((3, n), torch.float64),
              "geometric_normal": ((3, n), torch.float64), "albedo": ((3, n), torch.float64),
              "lit": ((n,), torch.uint8), "triangle": ((n,), torch.int32), "bary": ((2, n), torch.float64)}
    planes = {k: torch.empty(s, dtype=t, device=r.device) for k, (s, t) in shapes.items()}
    keep = [blob, dirs, light, ids, ws, colour, planes]
    steps, host = {}, {}
    for level in LEVELS:
        table = meshes.mesh_table(scenes.build_scene(scenes.mesh_spec(W, H, level)).shapes)
        host[f"level{level}"] = {"triangles": int(table[meshes.MH_NTRI]), "nodes": int(table[meshes.MH_NNODES])}
        dev = torch.tensor(table, device=r.device)
        keep.append(dev)
        for case, names in CASES.items():
            def passes(dev=dev, names=names):
                outs = [planes[k].data_ptr() if k in names else None for k in MESH_AOV_NAMES]
                L.check(r._lib.rtx_mesh_aovs(blob.data_ptr(), S, dev.data_ptr(), dev.numel(), light.data_ptr(), 1,
                                             ids.data_ptr(), _eye_ptr(blob), 0, dirs.data_ptr(), n, *outs, r._stream()),
                        "rtx_mesh_aovs")

            steps[f"{case}_level{level}"] = passes

        def trace(dev=dev):
            L.check(r._lib.rtx_trace_mesh(blob.data_ptr(), S, dev.data_ptr(), dev.numel(), light.data_ptr(), 1,
                                          _eye_ptr(blob), 0, dirs.data_ptr(), n, 0, colour.data_ptr(), L.OUT_F64_SOA,
                                          ws.data_ptr(), ws.numel(), r._stream()), "rtx_trace_mesh")

        steps[f"d_trace_mesh_cap0_level{level}"] = trace
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    res = {"scene": "mesh_spec", "width": W, "height": H, "pixels": n, "label": a.label, "library": str(L.LIB_PATH.name),
           "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step (one kernel launch: the rays and the tables are on the device); median and "
                     "interquartile range of the timed steps; the readings alternate by rounds in one process",
           "host": host, "readings": {name: summary(us) for name, us in times.items()}}
    rd = res["readings"]
    per_pixel = {case: sum(BYTES[k] for k in names) for case, names in CASES.items()}
    res["derived"] = {"bytes_written_per_pixel": per_pixel, "a_tb_per_s": {}, "b_below_d_by_us": {},
                      "b_below_d_by_more_than_both_iqr": {}}
    for level in LEVELS:
        av, b, d = rd[f"a_all_ten_level{level}"], rd[f"b_depth_id_level{level}"], rd[f"d_trace_mesh_cap0_level{level}"]
        res["derived"]["a_tb_per_s"][f"level{level}"] = round(per_pixel["a_all_ten"] * n / (av["median_us"] * 1e-6) / 1e12, 4)
        gap = d["median_us"] - b["median_us"]
        res["derived"]["b_below_d_by_us"][f"level{level}"] = round(gap, 2)
        res["derived"]["b_below_d_by_more_than_both_iqr"][f"level{level}"] = bool(gap > b["iqr_us"] + d["iqr_us"])
    for name, s in rd.items():
        print(json.dumps({name: s}), flush=True)
    print(json.dumps({"host": host, "derived": res["derived"]}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "readings": len(rd)}))


if __name__ == "__main__":
    main()
