"""The perspective camera against the reference camera's frame, on the GPU.

    python tools/camera_bench.py --out profiles/camera_C2.json [--steps 30] [--ks 1,2,4]

README scene, 1920x1080, 3 bounces (config C2), k x k samples per pixel, float32 and uint8 output.
Per case, HIP events around every step, a warm-up, the median of ``--steps`` timed steps, the cases of
one k alternating by rounds in one process:

* (r) the reference-camera frame, ``HipRenderer(samples=k)`` on the plain scene: the existing path
  (the fused camera kernel with its level-0 culling and wave tiles; for k >= 2 the resolve);
* (p) the same scene through a pinhole ``PerspectiveCamera`` at the reference camera's position whose
  field of view covers the reference screen (it sees the same spheres): rtx_camera_rays, then
  rtx_trace_rays from the shared eye, then the resolve;
* (l) the same with ``lens_radius = 0.05`` (k >= 2): per-ray origins;
* (g) the generator launch alone, pinhole and with the lens, with the bytes it writes (24 or 48 per
  ray) and the achieved rate.

The yardstick of (p) and (l) is (r) at the same k; that of (g) the resolve kernel's recorded rate
(profiles/ssaa_C2.json). No ratio is a pass condition: the file records what the explicit rays cost.
"""

import argparse
import json
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402


def matching_camera(spec: dict, lens_radius: float = 0.0) -> dict:
    """The spec with a PerspectiveCamera at the reference camera's position that covers the reference
    screen (base.py:130-141: x in [-1, 1], y centred on 0.25, at z = 0)."""
    cam = spec["camera"]
    px, py, pz = cam["position"]
    half_height = 1.0 / (float(cam["width"]) / cam["height"])  # the screen's half height
    fov = 2.0 * math.degrees(math.atan(half_height / abs(pz)))
    return scenes.with_camera(spec, target=[px, 0.25, 0.0], fov=fov, lens_radius=lens_radius or None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per case (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the cases of one k alternate in this many rounds")
    ap.add_argument("--ks", default="1,2,4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/camera_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.bounces
    spec = scenes.readme_spec(W, H)
    plain = scenes.build_scene(spec)
    pin = scenes.build_scene(matching_camera(spec))
    lensed = scenes.build_scene(matching_camera(spec, 0.05))
    per_round = -(-a.steps // a.rounds)
    res = {"scene": "readme", "width": W, "height": H, "max_bounces": B, "device": torch.cuda.get_device_name(0),
           "perspective_camera": {k: v for k, v in matching_camera(spec)["camera"].items() if k not in ("width", "height")},
           "method": "HIP events per step; median of the timed steps; the cases of one k alternate by rounds in one "
                     "process", "cases": []}
    for k in [int(x) for x in a.ks.split(",")]:
        n = k * k * W * H
        for out in ("f32", "u8"):
            o = "u8" if out == "u8" else None
            r = HipRenderer(B, color_dtype=torch.float32, samples=k)
            steps = {"r_reference_camera": lambda: r.render_tile(plain, out=o),
                     "p_pinhole": lambda: r.render_tile(pin, out=o)}
            if k >= 2:
                steps["l_lens"] = lambda: r.render_tile(lensed, out=o)
            # how far the two cameras' frames are apart (not the same pixels: another screen sampling)
            diff = float((steps["r_reference_camera"]().to(torch.float64) - steps["p_pinhole"]().to(torch.float64))
                         .abs().mean())
            if out == "f32":  # the generator alone, into the renderer's ray buffers (once per k)
                dirs, origins = r._camera_buffer("dirs", 3 * n), r._camera_buffer("origins", 3 * n)
                steps["g_generator_pinhole"] = lambda: r._generate_rays(pin.camera, k, 1, 1, 0, 1, H, None, dirs)
                if k >= 2:
                    steps["g_generator_lens"] = lambda: r._generate_rays(lensed.camera, k, 1, 1, 0, 1, H, origins, dirs)
            for fn in steps.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in steps}
            for _ in range(a.rounds):
                for name, fn in steps.items():
                    times[name] += timed(fn, per_round)
            case = {"k": k, "out": out, "rays": n, "mean_abs_diff_r_p": diff}
            for name, us in times.items():
                case[name] = s = summary(us)
                if name.startswith("g_"):
                    s["bytes"] = n * (48 if name.endswith("lens") else 24)
                    s["TBps"] = round(s["bytes"] / (s["median_us"] * 1e-6) / 1e12, 3)
            ref = case["r_reference_camera"]["median_us"]
            case["p_over_r"] = round(case["p_pinhole"]["median_us"] / ref, 3)
            if "l_lens" in case:
                case["l_over_r"] = round(case["l_lens"]["median_us"] / ref, 3)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del r
            torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": a.out, "cases": len(res["cases"])}))


if __name__ == "__main__":
    main()
