"""Registers, spills and scratch of every k_render_fast instantiation, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (no GPU needed).

    python tools/resource_usage.py [SOURCE.hip ...]      (default: every unit of csrc/ that has such kernels)

Compiles each source for gfx950 with the library's flags (device only, in parallel) and prints one
row per instantiation: template arguments <B, LDS, DEEP, STATS, TP, IMG, NSPH[, WAVES]>, VGPRs, VGPR
spills, scratch bytes per lane, occupancy, SGPRs and LDS bytes, side by side for the sources given
(the units of an A/B variant sit in a sibling directory of csrc/, python_ray_tracer_amd/_ab_<name>/,
as tools/ab_build.py lays them out, so that their relative #include resolves). Revisions up to
896f684 carried one more argument after DEEP (a flag of the retired backward fold, false in every
kernel they could launch); it is dropped from the row key, so
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
    # default: the library's device units; each unit's own flags by its stem (_build.UNIT_FLAGS)
    given = [Path(s) for s in sys.argv[1:]]
    srcs = given or [s for s, _ in _build.library_units() if _build.DEVICE_HDR.name in s.read_text()]
    procs = [subprocess.Popen([_build.hipcc(), *FLAGS, *_build.UNIT_FLAGS.get(s.stem, []), "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null", str(s)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for s in srcs]
    res = [{demangle_args(n): u for n, u in usage(p.communicate()[0]).items()} for p in procs]
    if not given:  # a column per unit that instantiates k_render_fast
        srcs, res = zip(*[(s, r) for s, r in zip(srcs, res) if r])
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
