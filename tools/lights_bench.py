"""Several point lights against the one-light render of the same frame, on the GPU.

    python tools/lights_bench.py --out profiles/lights_C2.json [--steps 30] [--cap 3]

The frame is ``scenes.lights_spec(1920, 1080)``: the README scene (config C2) under its own light and
more, cut to 1, 2, 3 and 8 point lights (the first as a ``ColoredPointLight`` of intensity 1, white, so
that one light too goes through rtx_trace_lights; lights four to eight are EXTRA below). Per reading, HIP
events around every step, a warm-up, the median and the interquartile range of ``--steps`` timed steps;
the readings alternate by rounds in one process:

* (l) ``render_tile`` of the frame under k lights: its rays generated (rtx_ray_directions) and traced by
  rtx_trace_lights;
* (p) ``render_tile`` of the same frame with a plain ``PointLight`` through the existing camera launch:
  the yardstick, the parent's kernels;
* (t) rtx_trace_lights alone on the frame's rays generated once before, under k lights;
* (r) rtx_trace_rays on the same rays: the one-light general kernel, the other yardstick.

Derived: one light against (r) on the same rays, and the cost of each added light, (t_k - t_1) / (k - 1),
against the first. No threshold is a pass condition: the file records what the lights cost.
"""

import argparse
import copy
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import lights, scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import _lib as L  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _eye_ptr  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402

EXTRA = [  # lights four to eight: higher than the scene's own light and on other sides of the spheres
    {"kind": "point", "position": [4.77, 6.87, 5.08], "intensity": 0.5, "color": [0.2, 1.0, 0.3]},
    {"kind": "point", "position": [-4.28, 9.47, 1.69], "intensity": 0.7, "color": [1.0, 0.2, 0.2]},
    {"kind": "point", "position": [2.94, 8.69, 9.75], "intensity": 0.3, "color": [0.9, 0.9, 0.5]},
    {"kind": "point", "position": [-2.07, 7.02, 3.87], "intensity": 0.8, "color": [0.5, 0.3, 0.9]},
    {"kind": "point", "position": [-3.26, 6.59, 6.74], "intensity": 0.25, "color": [0.3, 0.8, 0.8]},
]
COUNTS = (1, 2, 3, 8)


def cut(spec, k):
    """``spec`` with its first ``k`` point lights (EXTRA appended first), the first a ColoredPointLight."""
    out = copy.deepcopy(spec)
    pts = [li for li in out["lights"] if li["kind"] == "point"] + copy.deepcopy(EXTRA)
    pts[0] = dict(pts[0], intensity=1.0)
    out["lights"] = pts[:1] + [li for li in out["lights"] if li["kind"] != "point"] + pts[1:k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the readings alternate in this many rounds")
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--label", default=None, help="a name for this build in the output (an A/B of two libraries)")
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/lights_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.cap
    n = W * H
    spec = scenes.lights_spec(W, H)
    r = HipRenderer(B)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    blob, S = r.scene_blob(plain)
    dirs = r.get_ray_directions(plain.camera).data
    ws_l = torch.zeros(int(r._lib.rtx_lights_workspace_bytes(n, B)), dtype=torch.uint8, device=r.device)
    ws_r = r.workspace(n)
    steps = {"p_render_plain": lambda: r.render_tile(plain, out="u8", into=out)}
    keep = [blob, dirs, ws_l, ws_r, out]

    def trace_rays():
        L.check(r._lib.rtx_trace_rays(blob.data_ptr(), S, _eye_ptr(blob), 0, dirs.data_ptr(), n, r._bounces_arg,
                                      out.data_ptr(), L.OUT_U8_HWC, ws_r.data_ptr(), ws_r.numel(), None, r._stream()),
                "rtx_trace_rays")

    steps["r_trace_rays"] = trace_rays
    for k in COUNTS:
        scene = scenes.build_scene(cut(spec, k))
        table = torch.from_numpy(lights.lights_table(scene.lights)).to(r.device)
        assert table.shape[0] == k
        keep.append(table)
        steps[f"l_render_L{k}"] = lambda scene=scene: r.render_tile(scene, out="u8", into=out)

        def trace(table=table, k=k):
            L.check(r._lib.rtx_trace_lights(blob.data_ptr(), S, table.data_ptr(), k, _eye_ptr(blob), 0, dirs.data_ptr(), n,
                                            B, out.data_ptr(), L.OUT_U8_HWC, ws_l.data_ptr(), ws_l.numel(), r._stream()),
                    "rtx_trace_lights")

        steps[f"t_lights_L{k}"] = trace
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    res = {"scene": "lights_spec", "width": W, "height": H, "pixels": n, "max_bounces": B, "label": a.label,
           "library": str(L.LIB_PATH.name), "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step; median and interquartile range of the timed steps; the readings "
                     "alternate by rounds in one process",
           "readings": {name: summary(us) for name, us in times.items()}}
    med = {name: s["median_us"] for name, s in res["readings"].items()}
    t1 = med["t_lights_L1"]
    res["derived"] = {
        "one_light_over_trace_rays": round(t1 / med["r_trace_rays"], 3),
        "one_light_render_over_plain_render": round(med["l_render_L1"] / med["p_render_plain"], 3),
        "first_light_us": t1,
        "us_per_added_light": {f"L{k}": round((med[f"t_lights_L{k}"] - t1) / (k - 1), 2) for k in COUNTS if k > 1},
        "added_light_over_first": {f"L{k}": round((med[f"t_lights_L{k}"] - t1) / (k - 1) / t1, 3) for k in COUNTS if k > 1},
    }
    for name, s in res["readings"].items():
        print(json.dumps({name: s}), flush=True)
    print(json.dumps({"derived": res["derived"]}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "readings": len(res["readings"])}))


if __name__ == "__main__":
    main()
