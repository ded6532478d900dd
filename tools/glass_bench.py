"""Transmission against the opaque render of the same frame, on the GPU.

    python tools/glass_bench.py --out profiles/glass_C2.json [--steps 30] [--caps 3,5]

The frame is ``scenes.glass_spec(1920, 1080)``: the README scene (config C2) with the small sphere made
of glass and the large one half glass. Per reading, HIP events around every step, a warm-up, the median
and the interquartile range of ``--steps`` timed steps; the readings alternate by rounds in one process:

* (g) ``render_tile`` of the glass frame at each cap: the rays of the frame generated
  (rtx_ray_directions) and traced by rtx_trace_glass;
* (o) ``render_tile`` of the same frame with every gain at 0 at the same cap, through the existing camera
  launch: the yardstick, the parent's kernels;
* (t) rtx_trace_glass alone on the frame's rays generated once before, with the glass table and with a
  table of zero gains (the opaque frame through the glass kernel).

Rays per pixel: of the opaque frame the renderer's own counters; of the glass frame the NumPy
restatement's count on the same frame at a quarter of the size each way (tests/glass_ref.py; the glass
kernel keeps no counters). Time per traced ray is the median over pixels x rays per pixel. No threshold
is a pass condition: the file records what transmission costs.
"""

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import glass, scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import _lib as L  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _eye_ptr  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402


def opaque_spec(spec):
    out = json.loads(json.dumps(spec))
    for sp in out["spheres"]:
        sp["shader"]["transmission_gain"] = 0.0
    return out


def glass_rays_per_pixel(spec, cap, shrink=4):
    """Rays per pixel of the glass frame by the restatement, at 1/shrink of the size each way."""
    from tests import glass_ref

    small = scenes.with_camera(spec, width=spec["camera"]["width"] // shrink, height=spec["camera"]["height"] // shrink)
    counts = glass_ref.Counts()
    gains = [sp["shader"].get("transmission_gain", 0.0) for sp in small["spheres"]]
    glass_ref.render(small, gains, None, cap, counts=counts)
    n = small["camera"]["width"] * small["camera"]["height"]
    return counts.rays / n, counts.transmitted / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the readings alternate in this many rounds")
    ap.add_argument("--caps", default="3,5")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--label", default=None, help="a name for this build in the output (an A/B of two libraries)")
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/glass_bench.py measures on the GPU; none found")
    W, H = a.width, a.height
    n = W * H
    spec = scenes.glass_spec(W, H)
    scene_g = scenes.build_scene(spec)
    scene_o = scenes.build_scene(opaque_spec(spec))
    caps = [int(x) for x in a.caps.split(",")]
    steps, rays = {}, {}
    keep = []
    for B in caps:
        r = HipRenderer(B)
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
        steps[f"g_render_B{B}"] = lambda r=r, out=out: r.render_tile(scene_g, out="u8", into=out)
        steps[f"o_render_B{B}"] = lambda r=r, out=out: r.render_tile(scene_o, out="u8", into=out)
        blob, S = r.scene_blob(scene_g)
        dirs = r.get_ray_directions(scene_g.camera).data
        table = torch.from_numpy(glass.glass_table(scene_g.shapes)).to(r.device)
        zero = table.clone()
        zero[0] = 0.0
        ws = torch.zeros(int(r._lib.rtx_glass_workspace_bytes(n, B)), dtype=torch.uint8, device=r.device)
        keep += [blob, dirs, table, zero, ws, out]

        def trace(t, r=r, blob=blob, S=S, dirs=dirs, ws=ws, out=out, B=B):
            L.check(r._lib.rtx_trace_glass(blob.data_ptr(), S, t.data_ptr(), _eye_ptr(blob), 0, dirs.data_ptr(), n, B,
                                           out.data_ptr(), L.OUT_U8_HWC, ws.data_ptr(), ws.numel(), r._stream()),
                    "rtx_trace_glass")

        steps[f"t_glass_B{B}"] = lambda trace=trace, table=table: trace(table)
        steps[f"t_zero_gains_B{B}"] = lambda trace=trace, zero=zero: trace(zero)
        rc = HipRenderer(B, collect_stats=True)
        rc.render_tile(scene_o, out="u8")
        opaque_rays = sum(rc.stats()["rays"]) / n
        g_rays, g_transmitted = glass_rays_per_pixel(spec, B)
        rays[B] = {"opaque_rays_per_pixel": round(opaque_rays, 4), "glass_rays_per_pixel": round(g_rays, 4),
                   "glass_transmitted_per_pixel": round(g_transmitted, 4)}
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    res = {"scene": "glass_spec", "width": W, "height": H, "pixels": n, "label": a.label,
           "library": str(L.LIB_PATH.name), "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step; median and interquartile range of the timed steps; the readings "
                     "alternate by rounds in one process. glass rays per pixel: the restatement's count at a "
                     "quarter of the size each way; opaque rays per pixel: the renderer's counters",
           "readings": {name: summary(us) for name, us in times.items()}, "caps": {}}
    for B in caps:
        g = res["readings"][f"g_render_B{B}"]["median_us"]
        o = res["readings"][f"o_render_B{B}"]["median_us"]
        res["caps"][f"B{B}"] = dict(
            rays[B], glass_over_opaque=round(g / o, 3),
            glass_ns_per_ray=round(g * 1e3 / (n * rays[B]["glass_rays_per_pixel"]), 4),
            opaque_ns_per_ray=round(o * 1e3 / (n * rays[B]["opaque_rays_per_pixel"]), 4))
    for name, s in res["readings"].items():
        print(json.dumps({name: s}), flush=True)
    print(json.dumps({"caps": res["caps"]}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "readings": len(res["readings"])}))


if __name__ == "__main__":
    main()
