"""What the ``tools/*_bench.py`` share: HIP-event step times and their summary."""

import statistics

import torch


def timed(fn, n):
    """Per-step times (us) of n calls of fn, one HIP event pair per step."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]


def summary(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "q1_us": round(q[0], 2), "q3_us": round(q[2], 2), "iqr_us": round(q[2] - q[0], 2), "steps": len(us)}
