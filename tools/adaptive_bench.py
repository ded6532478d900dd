"""Adaptive anti-aliasing against full supersampling and the plain render, on the GPU.

    python tools/adaptive_bench.py --out profiles/adaptive_C2.json [--steps 30] [--ks 2,4]

README scene, 1920x1080, 3 bounces (config C2), k x k samples per pixel, float32 and uint8 output.
Per case, HIP events around every step, a warm-up, the median and interquartile range of ``--steps``
timed steps, the variants alternating by rounds in one process:

* (a) ``HipRenderer(samples=k, adaptive=True)`` with the default contrast 1/16: the plain frame, its
  passes, the edge mask, the flagged pixels' list (one host read-back), their sample rays, the trace
  and the resolve; (a0) the same with ``contrast=None`` (the geometric test alone);
* (b) ``HipRenderer(samples=k)``: every pixel k x k samples;
* (c) the plain render, one sample per pixel.

Beside them, (a)'s stage times (an event after each stage of the same timed steps' kind, in steps of
their own), the flagged share of both masks, and (a)'s uint8 frame against (b)'s: the largest
difference and the share of pixels that differ by more than 2 in some channel.

Pass condition: (a)'s median is below (b)'s by more than the interquartile ranges of both.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from python_ray_tracer_amd import scenes  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip import HipRenderer  # noqa: E402
from python_ray_tracer_amd.infrastructure.hip.base import _sample_scene  # noqa: E402
from tools.bench_util import summary, timed  # noqa: E402

STAGES = ("base", "passes", "mask", "resolve_base", "nonzero", "dirs", "trace", "scatter")


def stage_times(r, fn, n):
    """Median time (us) of each stage of n adaptive steps: an event when the step starts and one after
    each stage is enqueued (HipRenderer._stage_mark), so a stage's time includes the wait for the
    stages before it only where the host synchronised (``nonzero``: the read-back of the list)."""
    runs = []
    for _ in range(n):
        marks = []

        def mark(name, marks=marks):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

        r._stage_mark = mark
        mark("start")
        fn()
        r._stage_mark = None
        runs.append(marks)
    torch.cuda.synchronize()
    per = {s: [] for s in STAGES}
    for marks in runs:
        for (_, e0), (name, e1) in zip(marks, marks[1:]):
            per[name].append(e0.elapsed_time(e1) * 1e3)
    return {s: round(statistics.median(v), 2) for s, v in per.items() if v}


def kernels_alone(r, scene, k, o, n):
    """Median time (us) of each new launch alone, on the buffers the renderer's latest adaptive render of
    ``scene`` left behind: n calls back to back, an event pair around each (the launches queue up behind
    each other, so host launch time hides), with the rate over the bytes the launch has to move."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    lib, st = r._lib, r._stream()
    W, H = int(scene.camera.width), int(scene.camera.height)
    px = W * H
    b = r._adaptive_bufs
    pixels = torch.nonzero(b["mask"][:px]).view(-1).to(torch.int32)
    nf = int(pixels.numel())
    rays = nf * k * k
    sblob, _ = r.scene_blob(_sample_scene(scene, k))
    res = r.render_tile(scene, out=o)
    kind = L.OUT_U8_HWC if o else L.OUT_F32_SOA
    out_bytes = 3 if o else 12

    def mask():
        L.check(lib.rtx_edge_mask(b["base"].data_ptr(), b["id"].data_ptr(), b["hits"].data_ptr(), b["lit"].data_ptr(), W, H,
                                  r.contrast, b["mask"].data_ptr(), st), "rtx_edge_mask")

    def dirs():
        L.check(lib.rtx_sample_dirs(sblob.data_ptr(), k, W, H, pixels.data_ptr(), nf, b["dirs"].data_ptr(), st),
                "rtx_sample_dirs")

    def scatter():
        L.check(lib.rtx_resolve_scatter(b["samples"].data_ptr(), k, pixels.data_ptr(), nf, W, H, res.data_ptr(), kind, st),
                "rtx_resolve_scatter")

    def nonzero():
        return torch.nonzero(b["mask"][:px]).view(-1).to(torch.int32)

    got = {}
    for name, fn, moved in (("edge_mask", mask, px * (24 + 4 + 4 + 1 + 1)), ("sample_dirs", dirs, nf * 4 + rays * 24),
                            ("resolve_scatter", scatter, rays * 24 + nf * (4 + out_bytes)), ("nonzero", nonzero, None)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        us = statistics.median(timed(fn, n))
        got[name] = {"median_us": round(us, 2)}
        if moved is not None:
            got[name].update(bytes=moved, GBps=round(moved / (us * 1e-6) / 1e9, 1))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to write (default: stdout only)")
    ap.add_argument("--steps", type=int, default=30, help="timed steps per case (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the variants alternate in this many rounds")
    ap.add_argument("--ks", default="2,4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/adaptive_bench.py measures on the GPU; none found")
    W, H, B = a.width, a.height, a.bounces
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    per_round = -(-a.steps // a.rounds)
    res = {"scene": "readme", "width": W, "height": H, "max_bounces": B, "device": torch.cuda.get_device_name(0),
           "method": "HIP events per step; median and interquartile range of the timed steps; the variants "
                     "alternate by rounds in one process; stage times from events after each stage, in steps of "
                     "their own",
           "contrast": 0.0625, "cases": []}
    for k in [int(x) for x in a.ks.split(",")]:
        for out, dtype in (("f32", torch.float32), ("u8", torch.uint8)):
            o = "u8" if out == "u8" else None
            mk = dict(color_dtype=torch.float32)
            variants = {"a_adaptive": HipRenderer(B, samples=k, adaptive=True, **mk),
                        "a0_adaptive_geometric": HipRenderer(B, samples=k, adaptive=True, contrast=None, **mk),
                        "b_samples": HipRenderer(B, samples=k, **mk),
                        "c_plain": HipRenderer(B, **mk)}
            steps = {name: (lambda r=r: r.render_tile(scene, out=o)) for name, r in variants.items()}
            for fn in steps.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in steps}
            for _ in range(a.rounds):
                for name, fn in steps.items():
                    times[name] += timed(fn, per_round)
            case = {"k": k, "out": out}
            for name in steps:
                case[name] = summary(times[name])
            for name in ("a_adaptive", "a0_adaptive_geometric"):
                r = variants[name]
                case[name]["flagged"] = r.last_adaptive["flagged"]
                case[name]["flagged_share"] = round(r.last_adaptive["flagged"] / r.last_adaptive["pixels"], 4)
                case[name]["stages_us"] = stage_times(r, steps[name], a.steps)
            case["a_adaptive"]["kernels_alone"] = kernels_alone(variants["a_adaptive"], scene, k, o, a.steps)
            sa, sb = case["a_adaptive"], case["b_samples"]
            case["a_over_b"] = round(sa["median_us"] / sb["median_us"], 3)
            case["a_over_c"] = round(sa["median_us"] / case["c_plain"]["median_us"], 3)
            case["pass"] = sb["median_us"] - sa["median_us"] > sa["iqr_us"] + sb["iqr_us"]
            # (a)'s uint8 frame against (b)'s
            ua = variants["a_adaptive"].render_tile(scene, out="u8").to(torch.int16)
            ub = variants["b_samples"].render_tile(scene, out="u8").to(torch.int16)
            d = (ua - ub).abs().amax(dim=-1)
            case["u8_vs_b"] = {"max_abs_diff": int(d.max()), "share_differing_by_more_than_2": round(float((d > 2).float().mean()), 6),
                               "share_differing": round(float((d > 0).float().mean()), 6)}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del variants, steps
            torch.cuda.empty_cache()
    res["pass"] = all(c["pass"] for c in res["cases"])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"pass": res["pass"], "out": a.out}))


if __name__ == "__main__":
    main()
