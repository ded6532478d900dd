"""Registers, spills and scratch of every k_render_fast instantiation, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (no GPU needed).

    python tools/resource_usage.py [SOURCE.hip ...]      (default: csrc/rtx_kernels.hip)

Compiles each source for gfx950 with the library's flags (device only, in parallel) and prints one
row per instantiation: template arguments <B, LDS, DEEP, STATS, TP, IMG, NSPH[, WAVES]>, VGPRs, VGPR
spills, scratch bytes per lane, occupancy, SGPRs and LDS bytes, side by side for the sources given
(A/B variants of the kernel file must sit next to it, e.g. csrc/_ab_x.hip, so that its relative
#include resolves). Revisions up to 896f684 carried one more argument after DEEP (a flag of the
retired backward fold, false in every kernel they could launch); it is dropped from the row key, so
that such a revision (tools/ab_build.py --rev) and the present file share rows, and shown as a
trailing "+" where it was true.
"""

from __future__ import annotations

import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from python_ray_tracer_amd import _build  # noqa: E402

FLAGS = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]


def demangle_args(name: str) -> str:
    # <B, LDS, DEEP (bool before round 6's split, int 0/1/2 since), [the retired flag,] STATS, TP, IMG[, NSPH[, WAVES]]>
    m = re.search(r"k_render_fastILi(\d+)ELb(\d)EL[bi](\d)E(?:Lb(\d)E)?Lb(\d)ELi(\d)ELb(\d)E(?:Li(\d+)E)?(?:Li(\d+)E)?", name)
    if not m:
        return name
    g = list(m.groups())
    retired = g.pop(3)
    return "<" + ",".join(x for x in g if x is not None) + ">" + ("+" if retired == "1" else "")


def usage(text: str) -> dict:
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1) if "k_render_fast" in m.group(1) else None
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?):\s+(\S+) \[", line)
        if cur and m:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def main():
    # default: the library's two units (the small-scene kernels live in rtx_small.hip, built with
    # _build.SMALL_FLAGS); each source is a column
    srcs = [Path(s) for s in sys.argv[1:]] or [_build.SRC, _build.SMALL_SRC]
    procs = [subprocess.Popen([_build.hipcc(), *FLAGS, *(_build.SMALL_FLAGS if "small" in s.name else []),
                               "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null", str(s)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for s in srcs]
    res = [{demangle_args(n): u for n, u in usage(p.communicate()[0]).items()} for p in procs]
    print("instantiation".ljust(18) + "".join(f"| {s.stem[:16]:16s} vgpr spill scr occ sgpr   lds " for s in srcs))
    for n in sorted(set().union(*res)):
        row = n.ljust(18)
        for r in res:
            u = r.get(n, {})
            row += "| {:16s} {:>4} {:>5} {:>3} {:>3} {:>4} {:>5} ".format(
                "", u.get("VGPRs", "-"), u.get("VGPRs Spill", "-"), u.get("ScratchSize [bytes/lane]", "-"),
                u.get("Occupancy [waves/SIMD]", "-"), u.get("TotalSGPRs", "-"), u.get("LDS Size [bytes/block]", "-"))
        print(row)


if __name__ == "__main__":
    main()
