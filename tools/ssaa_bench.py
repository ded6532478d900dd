"""Supersampled anti-aliasing against its torch workaround, on the GPU.

    hipcc --offload-arch=gfx950 -O3 -o tools/traffic_calib tools/traffic_calib.hip
    python tools/ssaa_bench.py --out profiles/ssaa_C2.json [--steps 30] [--ks 2,4]

README scene, 1920x1080, 3 bounces (config C2), k x k samples per pixel, float32 and uint8 output.
Per case, HIP events around every step, a warm-up, the median of ``--steps`` timed steps:

* (a) ``HipRenderer(samples=k)``: the sample frame's render and the resolve kernel;
* (b) the resolve launch alone on that sample frame, with its achieved rate over the bytes it has to
  move (the float64 samples once, the output once), beside a streaming read of the sample frame's
  bytes (``tools/traffic_calib read``, in a process of its own);
* (c) the workaround without the feature: the plain float64 render at (k W, k H), then
  ``clamp(0, 1).view(3, H, k, W, k).sum((2, 4)) / k**2`` and the cast to float32, or ``quantize``
  for uint8. The plain render path is the same code with and without the feature, so (a) and (c)
  are timed in one process, alternating by rounds.

Pass condition: (a)'s median is no slower than (c)'s beyond (c)'s own run-to-run spread (the
interquartile range of its timed steps, recorded beside it).
"""

import argparse
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer, HipRGBColor, _lib as L  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _sample_scene  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per case (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="(a) and (c) alternate in this many rounds")
    ap.add_argument("--ks", default="2,4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssaa_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.bounces
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    per_round = -(-a.steps // a.rounds)
    calib = REPO / "tools" / "traffic_calib"
    res = {"scene": "readme", "width": W, "height": H, "max_bounces": B, "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step; median of the timed steps; (a) and (c) alternate by rounds in one process",
           "cases": []}
    for k in [int(x) for x in a.ks.split(",")]:
        sample_bytes = 3 * 8 * k * k * W * H
        stream = None
        if calib.exists():  # a process of its own, before this one's next launches
            p = subprocess.run([str(calib), "read", str(sample_bytes), str(a.steps)], capture_output=True, text=True,
                               timeout=120, check=True)
            stream = json.loads(p.stdout.strip().splitlines()[-1])
        big = _sample_scene(scene, k)
        for out, dtype, out_bytes in (("f32", torch.float32, 12 * W * H), ("u8", torch.uint8, 3 * W * H)):
            o = "u8" if out == "u8" else None
            ssaa = HipRenderer(B, color_dtype=torch.float32, samples=k)
            plain = HipRenderer(B, color_dtype=torch.float64)

            def step_a():
                return ssaa.render_tile(scene, out=o)

            def step_c():
                s = plain.render_tile(big)
                c = (s.clamp(0, 1).view(3, H, k, W, k).sum((2, 4)) / (k * k)).view(3, H * W)
                return plain.quantize(HipRGBColor.from_tensor(c), scene.camera) if o else c.to(torch.float32)

            got = step_a()
            kind = L.OUT_U8_HWC if o else L.OUT_F32_SOA

            def step_b():
                ssaa._resolve(ssaa._sample_buf, W, H, 1, got, kind)

            # the workaround's sum is a tree, the kernel's a row-major chain: close, not bit-equal
            want = step_c()
            diff = float((got.to(torch.float64) - want.to(torch.float64)).abs().max())
            for fn in (step_a, step_c, step_b):
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            ta, tb, tc = [], [], []
            for _ in range(a.rounds):
                ta += timed(step_a, per_round)
                tc += timed(step_c, per_round)
                tb += timed(step_b, per_round)
            sa, sb, sc = summary(ta), summary(tb), summary(tc)
            moved = sample_bytes + out_bytes
            sb["bytes"] = moved
            sb["GBps"] = round(moved / (sb["median_us"] * 1e-6) / 1e9, 1)
            case = {"k": k, "out": out, "sample_frame_MB": round(sample_bytes / 1e6, 1),
                    "a_samples_step": sa, "b_resolve_alone": sb, "b_streaming_read": stream, "c_workaround": sc,
                    "a_over_c": round(sa["median_us"] / sc["median_us"], 3),
                    "b_over_a": round(sb["median_us"] / sa["median_us"], 3),
                    "max_abs_diff_a_c": diff,
                    "pass": sa["median_us"] <= sc["median_us"] + sc["iqr_us"]}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            torch.cuda.empty_cache()
    res["pass"] = all(c["pass"] for c in res["cases"])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"pass": res["pass"], "out": a.out}))


if __name__ == "__main__":
    main()
