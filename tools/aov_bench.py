"""The primary-hit render passes against their composition from the older ops, on the GPU.

    python tools/aov_bench.py --out profiles/aov_C2.json [--steps 30]

Two frames: C2 (README scene, 1920x1080) and C3's scene (16 spheres and the ground, 3840x2160). Per
frame four cases, HIP events around every step, a warm-up, the median of ``--steps`` timed steps, the
cases alternating by rounds in one process:

* (a) ``render_aovs`` with all seven passes: 85 bytes per pixel written (depth 8, id 4, hits 4,
  position, normal and albedo 24 each, lit 1), with the achieved write rate beside the 6.3 TB/s the
  device streams;
* (b) ``render_aovs`` with ``depth`` and ``id`` only (12 bytes per pixel);
* (c) the same two passes composed from what existed before the kernel: ``rtx_ray_directions``, one
  ``rt::intersect`` per sphere, a ``torch.minimum`` chain and an equality scan for the id (S + 1
  launches of the library and 32 bytes per ray and sphere of traffic); checked equal to (b);
* (d) the colour render at ``max_bounces=0`` (float64), for scale only.

Pass condition: (b)'s median is below (c)'s on both frames.
"""

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

import python_ray_tracer_amd.ops  # noqa: E402,F401
from python_ray_tracer_amd import scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import FARAWAY, HipRenderer, _lib as L  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402

STREAM_TBPS = 6.3  # achievable HBM streaming rate of the MI355X
BYTES = {"depth": 8, "id": 4, "hits": 4, "position": 24, "normal": 24, "albedo": 24, "lit": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per case (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the cases alternate in this many rounds")
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/aov_bench.py measures on the GPU; none found")
    per_round = -(-a.steps // a.rounds)
    lib = L.load()
    res = {"device": torch.cuda.get_device_name(0), "streaming_TBps": STREAM_TBPS,
           "method": "HIP events per step; median of the timed steps; cases alternate by rounds in one process",
           "frames": []}
    frames = (("C2", lambda: scenes.readme_spec(1920, 1080)), ("C3", lambda: scenes.random_spec(16, 0, 3840, 2160)))
    for name, make in frames:
        spec = make()
        scene = scenes.build_scene(spec)
        W, H = int(scene.camera.width), int(scene.camera.height)
        n = W * H
        r, r0 = HipRenderer(3), HipRenderer(0)
        blob, S = r.scene_blob(scene)
        cam = torch.tensor(spec["camera"]["position"], dtype=torch.float64, device=blob.device)
        geo = [blob[L.HDR_WORDS + s * L.GEOM_WORDS:L.HDR_WORDS + (s + 1) * L.GEOM_WORDS] for s in range(S)]

        def step_a():
            return r.render_aovs(scene)

        def step_b():
            return r.render_aovs(scene, ("depth", "id"))

        def step_c():
            D = torch.empty((3, n), dtype=torch.float64, device=blob.device)
            L.check(lib.rtx_ray_directions(blob.data_ptr(), W, H, 1, 1, 0, H, D.data_ptr(), L.stream_handle()),
                    "rtx_ray_directions")
            t = [torch.ops.rt.intersect(g, cam, D) for g in geo]
            nearest = t[0]
            for ts in t[1:]:
                nearest = torch.minimum(nearest, ts)
            ident = torch.full((n,), -1, dtype=torch.int32, device=blob.device)
            for s in range(S - 1, -1, -1):  # the smallest index at the nearest distance wins
                ident = torch.where(t[s] == nearest, s, ident)
            return nearest, torch.where(nearest == FARAWAY, -1, ident).to(torch.int32)

        def step_d():
            return r0.render_tile(scene)

        b, c = step_b(), step_c()
        same = bool(torch.equal(b["depth"], c[0]) and torch.equal(b["id"], c[1]))
        steps = {"a": step_a, "b": step_b, "c": step_c, "d": step_d}
        for fn in steps.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, fn in steps.items():
                times[k] += timed(fn, per_round)
        s = {k: summary(v) for k, v in times.items()}
        wrote = sum(BYTES.values()) * n
        s["a"]["bytes_written"] = wrote
        s["a"]["TBps"] = round(wrote / (s["a"]["median_us"] * 1e-6) / 1e12, 3)
        s["a"]["of_streaming"] = round(s["a"]["TBps"] / STREAM_TBPS, 3)
        s["b"]["bytes_written"] = 12 * n
        s["c"]["library_launches"] = S + 1
        frame = {"frame": name, "width": W, "height": H, "spheres": S,
                 "a_all_seven_passes": s["a"], "b_depth_id": s["b"], "c_composed_from_older_ops": s["c"],
                 "d_colour_0_bounces": s["d"], "b_equals_c": same,
                 "b_over_c": round(s["b"]["median_us"] / s["c"]["median_us"], 4),
                 "a_over_d": round(s["a"]["median_us"] / s["d"]["median_us"], 3),
                 "pass": same and s["b"]["median_us"] < s["c"]["median_us"]}
        res["frames"].append(frame)
        print(json.dumps(frame), flush=True)
        del b, c
        torch.cuda.empty_cache()
    res["pass"] = all(f["pass"] for f in res["frames"])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"pass": res["pass"], "out": a.out}))


if __name__ == "__main__":
    main()
