"""The environment map against the same frame's rays without it, on the GPU.

    python tools/env_bench.py --out profiles/env_C2.json [--steps 30] [--cap 3]

The frame is ``scenes.env_spec(1920, 1080)``: the README scene (config C2) under the procedural sky, once
as a 2048 x 1024 image (32 MiB of texels: beyond L2) and once as a 256 x 128 one (512 KiB) for contrast.
Per reading, HIP events around every step, a warm-up, the median and the interquartile range of
``--steps`` timed steps; the readings alternate by rounds in one process:

* (e) ``render_tile`` of the environment frame: its rays generated (rtx_ray_directions) and traced by
  rtx_trace_lights_env;
* (t) rtx_trace_lights_env alone on the frame's rays generated once before;
* (p) the same rays through rtx_trace_lights with the one-row table (lights[0], 1, 1, 1): the parent's
  kernel, the yardstick;
* (s) rtx_env_sample alone on as many directions as the frame has rays that meet no shape, every level
  (counted with the NumPy restatement at 480 x 270 and scaled by the pixel count), the directions drawn
  from the frame's own.

Derived: (t) - (p), what the lookup costs inside the divergent walk, beside (s), what it costs alone. No
threshold is a pass condition: the file records what the environment costs.
"""

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import ctypes  # noqa: E402

import torch  # noqa: E402

from python_ray_tracer_amd import environment, scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import _lib as L  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _eye_ptr  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402

SIZES = ((2048, 1024), (256, 128))


def count_misses(cap):
    """Rays that meet no shape by level in the README frame at 480 x 270 (the NumPy restatement)."""
    from tests import env_ref

    spec = scenes.readme_spec(480, 270)
    counts = env_ref.Counts()
    env_ref.render(spec, env_ref.Env(scenes.sky_texels(16, 8).astype("float32")), cap, counts=counts)
    return counts.misses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per reading (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the readings alternate in this many rounds")
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/env_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.cap
    n = W * H
    misses = count_misses(B)
    n_miss = int(round(sum(misses) * n / (480 * 270)))
    r = HipRenderer(B)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    blob, S = r.scene_blob(plain)
    dirs = r.get_ray_directions(plain.camera).data
    table = torch.from_numpy(environment.unit_light_table(plain.lights[0])).to(r.device)
    ws = torch.zeros(int(r._lib.rtx_lights_workspace_bytes(n, B)), dtype=torch.uint8, device=r.device)
    pick = torch.randint(0, n, (n_miss,), generator=torch.Generator().manual_seed(0)).to(r.device)
    sdirs = dirs[:, pick].contiguous()
    sout = torch.empty_like(sdirs)
    keep = [blob, dirs, table, ws, out, sdirs, sout]

    def trace_plain():
        L.check(r._lib.rtx_trace_lights(blob.data_ptr(), S, table.data_ptr(), 1, _eye_ptr(blob), 0, dirs.data_ptr(), n, B,
                                        out.data_ptr(), L.OUT_U8_HWC, ws.data_ptr(), ws.numel(), r._stream()),
                "rtx_trace_lights")

    steps = {"p_lights_one_row": trace_plain}
    for ew, eh in SIZES:
        tag = f"{ew}x{eh}"
        scene = scenes.build_scene(scenes.env_spec(W, H, ew, eh))
        light = environment.environment_of(scene.lights)
        gain, turn = environment.env_params(light)
        texels = torch.tensor(light.texels, device=r.device)
        env = L.Env(texels.data_ptr(), ew, eh, (ctypes.c_double * 3)(*gain), turn)
        keep += [texels, env]
        steps[f"e_render_{tag}"] = lambda scene=scene: r.render_tile(scene, out="u8", into=out)

        def trace(env=env):
            L.check(r._lib.rtx_trace_lights_env(blob.data_ptr(), S, table.data_ptr(), 1, _eye_ptr(blob), 0,
                                                dirs.data_ptr(), n, B, out.data_ptr(), L.OUT_U8_HWC, ws.data_ptr(),
                                                ws.numel(), r._stream(), ctypes.byref(env)), "rtx_trace_lights_env")

        def sample(env=env):
            L.check(r._lib.rtx_env_sample(ctypes.byref(env), sdirs.data_ptr(), n_miss, sout.data_ptr(), r._stream()),
                    "rtx_env_sample")

        steps[f"t_lights_env_{tag}"] = trace
        steps[f"s_env_sample_{tag}"] = sample
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = -(-a.steps // a.rounds)
    times = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            times[name] += timed(fn, per_round)
    res = {"scene": "env_spec", "width": W, "height": H, "pixels": n, "max_bounces": B,
           "library": str(L.LIB_PATH.name), "device": torch.cuda.get_device_name(0),
           "misses_480x270_by_level": misses, "sampled_directions": n_miss,
           "image_bytes": {f"{ew}x{eh}": ew * eh * 16 for ew, eh in SIZES},
           "method": "HIP events per step; median and interquartile range of the timed steps; the readings "
                     "alternate by rounds in one process",
           "readings": {name: summary(us) for name, us in times.items()}}
    med = {name: s["median_us"] for name, s in res["readings"].items()}
    res["derived"] = {}
    for ew, eh in SIZES:
        tag = f"{ew}x{eh}"
        res["derived"][tag] = {
            "t_minus_p_us": round(med[f"t_lights_env_{tag}"] - med["p_lights_one_row"], 2),
            "s_us": med[f"s_env_sample_{tag}"],
            "t_over_p": round(med[f"t_lights_env_{tag}"] / med["p_lights_one_row"], 3),
            "render_minus_trace_us": round(med[f"e_render_{tag}"] - med[f"t_lights_env_{tag}"], 2),
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
