"""The occlusion passes against the existing shadow mask, on the GPU.

    python tools/occlusion_bench.py --out profiles/occlusion_C2.json [--steps 30] [--sides 2,4]

README scene, 1920x1080 (config C2). Per reading, HIP events around every step, a warm-up, the median
and the interquartile range of ``--steps`` timed steps; the readings alternate by rounds in one process:

* (o) the rtx_occlusion launch alone, on the frame's id, position and normal passes rendered once
  before: ``ao``, ``soft_lit`` (light_radius 1) and both, at each side;
* (a) beside them the existing rtx_primary_aovs launch with ``lit`` alone (the primary hit and one
  shadow ray) and with ``id, position, normal`` alone (what rtx_occlusion reads).

The yardstick of a ``soft_lit`` launch is the ``lit``-only launch: it traces side*side shadow rays and
finds no primary hit, so it is expected to take at most side*side times as long
(``soft_over_lit_per_sample`` <= 1). No ratio is a pass condition: the file records what the bundles
cost.
"""

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the readings alternate in this many rounds")
    ap.add_argument("--sides", default="2,4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--light-radius", type=float, default=1.0)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/occlusion_bench.py measures on the GPU; none found")
    W, H = a.width, a.height
    n = W * H
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = HipRenderer(3)
    blob, S = r.scene_blob(scene)
    hit = r.render_aovs(scene, ("id", "position", "normal"))
    steps = {"a_lit": lambda: r.render_aovs(scene, "lit"),
             "a_id_position_normal": lambda: r.render_aovs(scene, ("id", "position", "normal"))}
    sides = [int(x) for x in a.sides.split(",")]
    for side in sides:
        for names in (("ao",), ("soft_lit",), ("ao", "soft_lit")):
            steps[f"o_{'+'.join(names)}_side{side}"] = (
                lambda names=names, side=side: r._occlusion(blob, S, hit, n, names, side, 1e39, a.light_radius))
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    res = {"scene": "readme", "width": W, "height": H, "rays": n, "hits": int((hit["id"] >= 0).sum()),
           "light_radius": a.light_radius, "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step (the launch and the allocation of its outputs); median and interquartile "
                     "range of the timed steps; the readings alternate by rounds in one process",
           "readings": {name: summary(us) for name, us in times.items()}}
    lit = res["readings"]["a_lit"]["median_us"]
    res["soft_over_lit_per_sample"] = {
        f"side{side}": round(res["readings"][f"o_soft_lit_side{side}"]["median_us"] / (side * side * lit), 3)
        for side in sides}
    for name, s in res["readings"].items():
        print(json.dumps({name: s}), flush=True)
    print(json.dumps({"soft_over_lit_per_sample": res["soft_over_lit_per_sample"]}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "readings": len(res["readings"])}))


if __name__ == "__main__":
    main()
