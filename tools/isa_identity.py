"""Do two builds of the library's device units hold the same machine code, kernel by kernel?

    for f in python_ray_tracer_amd/csrc/*.hip; do       (every *.hip with device code)
      hipcc <_build.HIPCC_FLAGS> --cuda-device-only -S -o DIR/$(basename $f .hip).s $f
    done                                  (once in a checkout of the old revision, once in the new one)
    python tools/isa_identity.py OLD_DIR NEW_DIR > profiles/split_isa_identity.txt

Compares text only. A kernel's instruction text is its function body without comments and the
.loc / .file / .cfi lines, with the function-index digits of local labels (.LBB<n>_, .Lfunc_end<n>,
.Ltmp<n>, .LJTI<n>_) stripped: what moving text between files, or dropping a neighbour, may change
without changing the code. Its .amdhsa_* descriptor block and its register, spill and segment-size
metadata are compared as they stand. Prints one row per (kernel, unit) of either build and exits 1
when a kernel that both builds have in a unit differs, or when the new build has a kernel twice.
"""

from __future__ import annotations

import re
import sys
from pathlib import Path

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp|LJTI)\d+")
META = re.compile(r"^\s+(?:- )?\.(agpr_count|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|"
                  r"private_segment_fixed_size|group_segment_fixed_size|kernarg_segment_size|"
                  r"max_flat_workgroup_size|wavefront_size|uses_dynamic_stack):")


def kernels(asm: Path) -> dict:
    """{symbol: (instruction count, normalised body, descriptor block, metadata lines)}"""
    lines = asm.read_text(errors="replace").splitlines()
    desc, meta = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
            desc[m.group(1)] = [ln.split(";")[0].strip() for ln in lines[i:j]]
            i = j
        i += 1
    entry = []  # the metadata's kernel entries: "  - .key:" opens one
    for ln in lines[next((k for k, ln in enumerate(lines) if ln.startswith("amdhsa.kernels:")), len(lines)):]:
        if re.match(r"^  - \.", ln) or not ln.startswith(" "):
            name = next((e.split(":", 1)[1].strip().strip("'") for e in entry if re.match(r"\s+(- )?\.name:", e)), None)
            if name:
                meta[name] = sorted(e.replace("- ", "  ").strip() for e in entry if META.match(e))
            entry = []
        entry.append(ln)
    out = {}
    for sym in desc:
        start = next(k for k, ln in enumerate(lines) if ln.startswith(sym + ":"))
        body = []
        for ln in lines[start + 1:]:
            s = ln.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or s.startswith((".loc", ".file", ".cfi")):
                continue
            body.append(LABEL.sub(lambda m: "." + m.group(1), s))
        n = sum(1 for s in body if not s.endswith(":") and not s.startswith("."))
        out[sym] = (n, body, desc[sym], meta.get(sym))
    return out


def main(old_dir: str, new_dir: str) -> int:
    old = {p.stem: kernels(p) for p in sorted(Path(old_dir).glob("*.s"))}
    new = {p.stem: kernels(p) for p in sorted(Path(new_dir).glob("*.s"))}
    rows, bad = [], 0
    for unit in sorted(set(old) | set(new)):
        a, b = old.get(unit, {}), new.get(unit, {})
        for sym in sorted(set(a) | set(b)):
            if sym in a and sym in b:
                same = a[sym] == b[sym] and a[sym][3] is not None
                what = "identical" if same else "DIFFERENT"
                bad += not same
            else:
                what = "only in the old build" if sym in a else "only in the new build"
            rows.append((sym, unit, (b.get(sym) or a[sym])[0], what))
    homes = {}
    for unit, ks in new.items():
        for sym in ks:
            homes.setdefault(sym, []).append(unit)
    twice = {s: u for s, u in homes.items() if len(u) > 1}
    print(f"{'kernel':110s} {'unit':13s} {'instr':>6s}  result")
    for sym, unit, n, what in rows:
        print(f"{sym:110s} {unit:13s} {n:6d}  {what}")
    n_old, n_new = (sum(len(k) for k in d.values()) for d in (old, new))
    print(f"\nold build: {n_old} kernels; new build: {n_new} kernels in {len(new)} units, "
          f"{sum(w == 'identical' for *_, w in rows)} identical, {bad} different, "
          f"{sum(w == 'only in the old build' for *_, w in rows)} only in the old build, "
          f"{sum(w == 'only in the new build' for *_, w in rows)} only in the new build, "
          f"{len(twice)} in more than one unit of the new build")
    return 1 if bad or twice else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
