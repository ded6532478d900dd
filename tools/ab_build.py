"""Build librtx_hip.so variants for tools/ab.py (A/B timing on identical output).

    python tools/ab_build.py OUT.so [--set kName=VALUE ...] [--rev GIT_REV] [--patch FILE.py]

The shipped kernel has no tuning macros: its tuning values are ``constexpr`` lines in
``csrc/rtx_device.h``. A variant is a copy of the ``csrc/`` sources, of the working tree or of another
revision (``--rev HEAD~3``: the baseline of an A/B), in a sibling directory
``python_ray_tracer_amd/_ab_<name>/`` (so the relative #include of the ABI header resolves), built as
the library is: every ``*.hip`` of the copy is a unit. ``--set kFwdWavesPersist=5`` rewrites the one
``constexpr`` line of that name in the copy; ``--patch`` applies a Python file defining
``patch(src: str) -> str`` to the device header; ``--only-b`` trims the launch switches of
``rtx_kernels.hip``. (In revisions from before the header, ``rtx_kernels.hip`` holds all three.)
(Rounds 2-5 kept a set of named source patches, tools/ab_patches.py; round 6 retired it with the
experiments it served, whose results are in profiles/ and DESIGN.md, and which stay in git history.)
"""

import argparse
import re
import runpy
import shutil
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from python_ray_tracer_amd import _build  # noqa: E402


def trim(src: str, caps: set) -> str:
    """Instantiate only the capped fast kernels of `caps` (timing builds: other caps, unbounded
    renders and stats buffers then launch nothing)."""
    def sub(old, new):
        nonlocal src
        if old not in src:
            raise SystemExit(f"--only-b: pattern not found: {old!r}")
        src = src.replace(old, new)

    for b in range(6):
        if b not in caps:
            sub(f"    case {b}: launch_fast_b<{b}>(p, grid, s); break;\n", "")
    if 6 not in caps:
        sub("    default: launch_fast_b<6>(p, grid, s); break;", "    default: break;")
    sub("{ launch_fast_b<kDeepLevels, 1>(p, grid, s); }", "{}")
    sub("{ launch_fast_b<kDeepLevels, 2>(p, grid, s); }", "{}")
    sub("      launch_fast_lds<B, DEEP, true>(p, grid, s);", "      launch_fast_lds<B, DEEP, false>(p, grid, s);")
    return src


def sources(rev) -> dict:
    """The texts of csrc/'s units and headers by file name: the working tree's, or a revision's."""
    rel = _build.CSRC.relative_to(REPO).as_posix()
    if rev is None:
        return {p.name: p.read_text() for p in _build.CSRC.iterdir() if p.suffix in (".hip", ".h")}

    def git(*args):
        return subprocess.run(["git", *args], cwd=REPO, check=True, capture_output=True, text=True).stdout

    names = [n for n in git("ls-tree", "--name-only", rev, rel + "/").split() if n.endswith((".hip", ".h"))]
    return {Path(n).name: git("show", f"{rev}:{n}") for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--set", action="append", default=[], help="kName=VALUE (a constexpr tuning line)")
    ap.add_argument("--rev", default=None, help="git revision of csrc/ to build")
    ap.add_argument("--patch", default=None, help="a python file defining patch(src) -> src")
    ap.add_argument("--flag", action="append", default=[], help="extra hipcc flag")
    ap.add_argument("--small-flag", action="append", default=None,
                    help="hipcc flag of the small-scene unit only (replaces _build.SMALL_FLAGS)")
    ap.add_argument("--only-b", default=None,
                    help="comma list of bounce caps to instantiate (A/B builds in ~1/10 of the time: no "
                         "other caps, no deep/unbounded kernels, no stats instantiations)")
    a = ap.parse_args()
    files = sources(a.rev)
    device = _build.DEVICE_HDR.name if _build.DEVICE_HDR.name in files else "rtx_kernels.hip"
    for kv in a.set:
        name, val = kv.split("=", 1)
        pat = re.compile(rf"^(constexpr\s+\w+\s+{re.escape(name)}\s*=\s*)([^;]+)(;)", re.M)
        n = 0
        for f in files:
            files[f], k = pat.subn(lambda m: m.group(1) + val + m.group(3), files[f])
            n += k
        if n != 1:
            raise SystemExit(f"--set {name}: {n} matching constexpr lines")
    if a.patch:
        files[device] = runpy.run_path(a.patch)["patch"](files[device])
    if a.only_b is not None:
        files["rtx_kernels.hip"] = trim(files["rtx_kernels.hip"], {int(b) for b in a.only_b.split(",") if b})
    out = Path(a.out).resolve()
    copy = _build.PKG / f"_ab_{out.stem}"
    copy.mkdir()
    try:
        for f, text in files.items():
            (copy / f).write_text(text)
        out.parent.mkdir(parents=True, exist_ok=True)
        flags = _build.UNIT_FLAGS if a.small_flag is None else {"rtx_small": a.small_flag}
        _build.compile_units(out, _build.library_units(copy, flags), a.flag)
    finally:
        shutil.rmtree(copy, ignore_errors=True)
    print(out)


if __name__ == "__main__":
    main()
