"""What building a mesh scene's table costs on the host and on the GPU.

    python tools/mesh_build_bench.py --out profiles/mesh_build_C2.json [--steps 20] [--levels 2 4 6]

The scenes are ``scenes.mesh_spec(1920, 1080, level)``. Per reading, HIP events around every step (they
enclose the step's host work too: the stream is idle when a step begins), a warm-up, the median and the
interquartile range of ``--steps`` timed steps; the readings alternate by rounds in one process:

* ``host_build_upload``: ``meshes.mesh_table`` with its cache emptied, and the upload of its table;
* ``device_build_upload``: ``meshes.device_inputs`` with its caches emptied, the upload of the arrays and the
  skeleton, rtx_mesh_build and the read-back of its status words (what a HipRenderer with mesh_build = "device" does
  for new content);
* ``build_kernels``: rtx_mesh_build alone, its inputs on the device;
* ``content_digest``: the digest of the meshes' content, which both modes pay on every render;
* ``render_host_table`` / ``render_device_table``: ``render_tile`` from either table (the tables are equal, so
  only the readings' spread may separate them).

No ratio is a pass condition: the file records what was measured. The device-built table is compared with the
host's before anything is timed.
"""

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from python_ray_tracer_amd import meshes, scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import _lib as L  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402


def level_steps(level, W, H, cap, leaf):
    """({reading: step}, facts) of one level."""
    scene = scenes.build_scene(scenes.mesh_spec(W, H, level))
    shapes = scene.shapes
    host, dev = HipRenderer(cap), HipRenderer(cap)
    dev.mesh_build = "device"
    host.mesh_max_leaf = dev.mesh_max_leaf = leaf
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=host.device)
    table = meshes.mesh_table(shapes, leaf)
    inputs, key = meshes.device_inputs_entry(shapes, leaf)
    built = dev._build_mesh_table(key, inputs)
    same = bool(np.array_equal(built.cpu().numpy(), table))
    # the build alone: the inputs on the device, the skeleton built over in place (it keeps what the build reads)
    arrays = [None if a is None else torch.tensor(a, device=dev.device)
              for a in (inputs.vertices, inputs.faces, inputs.tri_mesh, inputs.normals, inputs.smooth, inputs.uvs)]
    ptr = [None if t is None else t.data_ptr() for t in arrays]
    skeleton = torch.tensor(inputs.skeleton, device=dev.device)
    head = np.ascontiguousarray(inputs.skeleton[:meshes.HDR_WORDS])
    T, N = int(inputs.faces.shape[0]), int(inputs.skeleton[meshes.MH_NNODES])
    ws = torch.empty(int(dev._lib.rtx_mesh_build_workspace_bytes(T, N)), dtype=torch.uint8, device=dev.device)

    def host_build_upload():
        meshes._TABLES.clear()
        torch.tensor(meshes.mesh_table(shapes, leaf), device=host.device)

    def device_build_upload():
        meshes._INPUTS.clear()
        meshes._RANGES.clear()
        dev._mesh_tables.clear()
        i, k = meshes.device_inputs_entry(shapes, leaf)
        dev._build_mesh_table(k, i)

    def build_kernels():
        L.check(dev._lib.rtx_mesh_build(ptr[0], int(inputs.vertices.shape[0]), ptr[1], ptr[2], T, ptr[3], ptr[4], ptr[5],
                                        head.ctypes.data, skeleton.data_ptr(), int(skeleton.numel()), inputs.max_leaf,
                                        ws.data_ptr(), ws.numel(), dev._stream()), "rtx_mesh_build")

    steps = {"host_build_upload": host_build_upload, "device_build_upload": device_build_upload,
             "build_kernels": build_kernels, "content_digest": lambda: meshes._content_digest(shapes),
             "render_host_table": lambda: host.render_tile(scene, out="u8", into=out),
             "render_device_table": lambda: dev.render_tile(scene, out="u8", into=out)}
    facts = {"triangles": T, "nodes": N, "table_bytes": int(table.nbytes), "workspace_bytes": int(ws.numel()),
             "device_table_equals_host_table": same, "pins": (arrays, skeleton, ws, out)}
    return steps, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="the readings alternate in this many rounds")
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--leaf", type=int, default=4)
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 4, 6])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_build_bench.py measures on the GPU; none found")
    res = {"scene": "mesh_spec", "width": a.width, "height": a.height, "max_bounces": a.cap, "max_leaf": a.leaf,
           "library": str(L.LIB_PATH.name), "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step, host work included (the stream is idle when a step begins); median and "
                     "interquartile range of the timed steps; the readings alternate by rounds in one process",
           "levels": {}}
    per_round = -(-a.steps // a.rounds)
    for level in a.levels:
        steps, facts = level_steps(level, a.width, a.height, a.cap, a.leaf)
        facts.pop("pins")
        frames = {}
        for name, fn in steps.items():
            for _ in range(a.warmup):
                got = fn()
            if name.startswith("render"):
                frames[name] = got.clone()
        torch.cuda.synchronize()
        facts["frames_equal"] = bool(torch.equal(frames["render_host_table"], frames["render_device_table"]))
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, fn in steps.items():
                times[name] += timed(fn, per_round)
        readings = {name: summary(us) for name, us in times.items()}
        h, d = readings["host_build_upload"], readings["device_build_upload"]
        gap = h["median_us"] - d["median_us"]
        facts["derived"] = {
            "host_over_device_build": round(h["median_us"] / d["median_us"], 2),
            "device_faster_by_more_than_both_iqrs": bool(gap > h["iqr_us"] and gap > d["iqr_us"]),
            "render_device_over_host_table": round(readings["render_device_table"]["median_us"]
                                                   / readings["render_host_table"]["median_us"], 4)}
        res["levels"][str(level)] = {**facts, "readings": readings}
        print(json.dumps({"level": level, **facts, "medians_us": {k: v["median_us"] for k, v in readings.items()},
                          "iqr_us": {k: v["iqr_us"] for k, v in readings.items()}}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "levels": list(res["levels"])}))


if __name__ == "__main__":
    main()
