"""Primary-hit render passes (rtx_primary_aovs, HipRenderer.render_aovs): what needs no GPU.

The C ABI entry points and their host-side argument checks, the rt::primary_aovs ops (schemas, Meta
shapes, TORCH_CHECKs), the NumPy reference of the passes (tests/aov_ref.py) pinned to the oracle, and
the preconditions that keep the GPU cases of tests/test_gpu_aov.py meaningful.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import aov_ref, specs

REPO = Path(__file__).resolve().parent.parent
W, H = 50, 22

_OUTS = r"double\* depth, int32_t\* id, int32_t\* hits, double\* position, double\* normal,\s*" \
        r"double\* albedo, uint8_t\* lit, void\* stream\);"


def test_header_declares_and_library_exports_the_passes():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"int rtx_primary_aovs\(const double\* scene, int n_spheres, int width, int height,\s*"
                     r"int row_block, int n_parts, int part, int part_run, int n_local_rows,\s*" + _OUTS, text)
    assert re.search(r"int rtx_primary_aovs_rays\(const double\* scene, int n_spheres, const double\* origins, "
                     r"int64_t origin_stride,\s*const double\* dirs, int64_t n,\s*" + _OUTS, text)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION == 3
    for name, bit in L.AOV_PASSES.items():
        assert int(re.search(rf"RTX_AOV_{name.upper()}\s*=\s*(\d+)", text).group(1)) == bit
    assert list(L.AOV_PASSES.values()) == [1, 2, 4, 8, 16, 32, 64] and list(L.AOV_PASSES) == list(aov_ref.PASSES)
    assert int(re.search(r"RTX_AOV_ALL\s*=\s*(\d+)", text).group(1)) == L.AOV_ALL == 127
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L._SIGS["rtx_primary_aovs"] == (i32, [p] + [i32] * 8 + [p] * 8)
    assert L._SIGS["rtx_primary_aovs_rays"] == (i32, [p, i32, p, i64, p, i64] + [p] * 8)
    lib = L.load()
    for name in ("rtx_primary_aovs", "rtx_primary_aovs_rays"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_argument_checks_need_no_gpu():
    """Every bad argument returns RTX_E_ARG (-1) with a message before any HIP call, and zero rays
    return RTX_OK without a launch: the pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)
    outs = dict(depth=p, id=p, hits=p, position=p, normal=p, albedo=p, lit=p)

    def cam(scene=p, S=3, width=W, height=H, rb=1, P=1, part=0, run=1, rows=H, **kw):
        o = {**outs, **kw}
        return lib.rtx_primary_aovs(scene, S, width, height, rb, P, part, run, rows, *o.values(), None)

    def rays(scene=p, S=3, org=p, stride=0, dirs=p, n=8, **kw):
        o = {**outs, **kw}
        return lib.rtx_primary_aovs_rays(scene, S, org, stride, dirs, n, *o.values(), None)

    none = {k: None for k in outs}
    assert cam(scene=None) == -1 and b"null scene" in lib.rtx_last_error()
    assert rays(scene=None) == -1 and b"null scene" in lib.rtx_last_error()
    assert rays(org=None) == -1 and b"null ray" in lib.rtx_last_error()
    assert rays(dirs=None) == -1 and b"null ray" in lib.rtx_last_error()
    assert cam(**none) == -1 and b"no pass" in lib.rtx_last_error()
    assert rays(**none) == -1 and b"no pass" in lib.rtx_last_error()
    for S in (0, -1, 1025):
        assert cam(S=S) == -1 and b"n_spheres" in lib.rtx_last_error(), S
        assert rays(S=S) == -1 and b"n_spheres" in lib.rtx_last_error(), S
    for kw in ({"width": 0}, {"height": -1}, {"rb": 0}, {"P": 0}, {"part": -1}, {"part": 1}, {"run": 0}, {"run": 2},
               {"rows": -1}, {"rows": H + 1}, {"P": 3, "rb": 4, "part": 2, "rows": 7}):
        assert cam(**kw) == -1 and b"geometry" in lib.rtx_last_error(), kw
    for stride in (1, 7, 9, -8):
        assert rays(stride=stride) == -1 and b"origin_stride" in lib.rtx_last_error(), stride
    assert rays(n=-1) == -1 and b"negative" in lib.rtx_last_error()
    # zero rays: nothing to launch (one requested pass is enough to be a valid call)
    assert cam(rows=0) == 0 and cam(P=3, rb=4, part=2, rows=0) == 0
    assert rays(n=0) == 0 and rays(n=0, stride=0, **{**none, "lit": p}) == 0


def test_op_schemas_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "primary_aovs" in ops.OPS and "primary_aovs_rays" in ops.OPS
    assert str(torch.ops.rt.primary_aovs.default._schema) == \
        ("rt::primary_aovs(Tensor scene, int n_spheres, int width, int height, int row_block, int n_parts, int part, "
         "int part_run, int passes, bool check=True) -> Tensor[]")
    assert str(torch.ops.rt.primary_aovs_rays.default._schema) == \
        "rt::primary_aovs_rays(Tensor scene, int n_spheres, Tensor origins, Tensor dirs, int passes, bool check=True) -> Tensor[]"
    S = 3
    blob = torch.empty(L.HDR_WORDS + S * (L.GEOM_WORDS + L.MAT_WORDS), dtype=torch.float64, device="meta")
    want = {"depth": ((), torch.float64), "id": ((), torch.int32), "hits": ((), torch.int32),
            "position": ((3,), torch.float64), "normal": ((3,), torch.float64), "albedo": ((3,), torch.float64),
            "lit": ((), torch.uint8)}

    def check(got, mask, n):
        names = [k for k, b in L.AOV_PASSES.items() if mask & b]
        assert len(got) == len(names)
        for t, k in zip(got, names):
            assert tuple(t.shape) == want[k][0] + (n,) and t.dtype == want[k][1] and t.device.type == "meta", (mask, k)

    dirs = torch.empty(3, 77, dtype=torch.float64, device="meta")
    for mask in (1, 2 | 4, 64, 16 | 32, 127, 1 | 8 | 64):
        check(torch.ops.rt.primary_aovs(blob, S, W, H, 1, 1, 0, 1, mask), mask, W * H)
        check(torch.ops.rt.primary_aovs(blob, S, W, H, 4, 3, 1, 1, mask), mask, W * 8)  # rows 4..7, 16..19
        check(torch.ops.rt.primary_aovs(blob, S, W, H, 4, 3, 1, 2, mask), mask, W * 14)
        check(torch.ops.rt.primary_aovs_rays(blob, S, torch.empty(3, dtype=torch.float64, device="meta"), dirs, mask),
              mask, 77)
    for dev in ("cpu", "meta"):
        b = torch.zeros(blob.shape, dtype=torch.float64, device=dev)
        d = torch.zeros(3, 5, dtype=torch.float64, device=dev)
        for mask in (0, 128, -1, 255):
            with pytest.raises(RuntimeError, match="cpu" == dev and "GPU tensor" or "passes"):
                torch.ops.rt.primary_aovs(b, S, W, H, 1, 1, 0, 1, mask)
            with pytest.raises(RuntimeError, match="cpu" == dev and "GPU tensor" or "passes"):
                torch.ops.rt.primary_aovs_rays(b, S, d[:, 0].contiguous(), d, mask)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.primary_aovs(torch.zeros(blob.shape, dtype=torch.float64), S, W, H, 1, 1, 0, 1, 127)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.primary_aovs_rays(torch.zeros(blob.shape, dtype=torch.float64), S, torch.zeros(3, dtype=torch.float64),
                                       torch.zeros(3, 5, dtype=torch.float64), 127)
    with pytest.raises(RuntimeError, match="geometry"):
        torch.ops.rt.primary_aovs(blob, S, W, H, 1, 2, 2, 1, 127)
    with pytest.raises(RuntimeError, match="too short"):
        torch.ops.rt.primary_aovs(blob, S + 1, W, H, 1, 1, 0, 1, 127)
    with pytest.raises(RuntimeError, match="dirs"):
        torch.ops.rt.primary_aovs_rays(blob, S, torch.empty(3, dtype=torch.float64, device="meta"),
                                       torch.empty(77, 3, dtype=torch.float64, device="meta"), 127)


def test_pass_names():
    from python_ray_tracer_amd.infrastructure.hip import AOV_NAMES
    from python_ray_tracer_amd.infrastructure.hip.base import _aov_names

    assert AOV_NAMES == aov_ref.PASSES
    assert _aov_names(AOV_NAMES) == AOV_NAMES and _aov_names(["lit", "depth"]) == ("depth", "lit")
    assert _aov_names("normal") == ("normal",)
    for bad in (("depth", "colour"), ("Depth",), (), ["z"]):
        with pytest.raises(ValueError, match="passes"):
            _aov_names(bad)


@pytest.mark.parametrize("name", ["readme", "rand16"])
def test_reference_is_the_oracles_own_arithmetic(name):
    """aov_ref against the oracle: lit and the nudged point are O._shade's per shape, and shading
    shape ``id`` at ``depth`` through O.create gives O.render's colour on every hit pixel, exactly (no
    tie in these frames); the colour of every miss is exactly 0."""
    make = {"readme": lambda: scenes.readme_spec(W, H), "rand16": lambda: scenes.random_spec(16, 0, W, H)}[name]
    scene, a = aov_ref.frame(name, make)
    origin, dirs = aov_ref.frame_rays(scene)
    assert not (a["hits"] > 1).any()
    color = O.render(scene, 3)
    miss = a["id"] < 0
    assert np.array_equal(a["depth"][miss], np.full(miss.sum(), O.FARAWAY)) and not a["hits"][miss].any()
    assert not color[:, miss].any()
    for k in ("position", "normal", "albedo", "nudged"):
        assert not a[k][:, miss].any(), k
    assert not a["lit"][miss].any()
    seen = 0
    for si, sp in enumerate(scene.spheres):
        m = a["id"] == si
        if not m.any():
            continue
        seen += int(m.sum())
        d = tuple(c[m] for c in dirs)
        _, _, lit, _, q, _ = O._shade(scene, si, sp, *origin, *d, a["depth"][m])
        assert np.array_equal(a["lit"][m], lit.astype(np.uint8)), si
        assert np.array_equal(a["nudged"][:, m], np.stack(q)), si
        got = np.stack(O.create(scene, si, origin, d, a["depth"][m], 3))
        diff = float(np.abs(got - color[:, m]).max())
        assert diff == 0.0, (si, diff)
    assert seen == int((~miss).sum()) > 0


def test_preconditions_of_the_gpu_cases(golden_meta):
    """What the frames of tests/test_gpu_aov.py contain: misses and hits, shadow, both checker cells,
    ties, image-textured hits well inside their texels."""
    _, a = aov_ref.frame("readme", lambda: scenes.readme_spec(W, H))
    hit = a["id"] >= 0
    assert (int((~hit).sum()), int(hit.sum())) == (355, 745)
    assert int((hit & (a["lit"] == 0)).sum()) == 31
    assert int((hit & (a["albedo"][0] == 0)).sum()) == 156 and int((hit & (a["albedo"][0] == 1)).sum()) == 454
    ground = a["id"] == 2  # the checker sphere: both cells
    assert int((ground & (a["albedo"][1] == 0)).sum()) == 156 and int((ground & (a["albedo"][1] == 1)).sum()) == 160

    spec = golden_meta["cases"]["ties_64x36_B2"]["spec"]
    _, t = aov_ref.frame("ties", lambda: spec)
    assert t["id"].shape == (64 * 36,) and int((t["hits"] > 1).sum()) == 226

    scene, x = aov_ref.frame("textured", lambda: specs.textured_spec(W, H))
    textured = [si for si, sp in enumerate(scene.spheres) if sp.image is not None]
    assert textured == [0, 1] and int(np.isin(x["id"], textured).sum()) == 241
    margin = np.inf  # distance of u (w - 1) and v (h - 1) (shape.py:69-77) from the nearest integer, in texels
    for si in textured:
        sp, m = scene.spheres[si], x["id"] == si
        px, py, pz = x["position"][:, m]
        nx, ny, nz = O._norm(px - sp.cx, py - sp.cy, pz - sp.cz)
        u = (0.5 + np.arctan2(nz, nx) / (2 * np.pi)) % 1
        v = (0.5 - np.arcsin(ny) / np.pi) % 1
        h, w, _ = sp.image.shape
        for c in (u * (w - 1), v * (h - 1)):
            margin = min(margin, float(np.abs(c - np.rint(c)).min()))
    print(f"nearest texel edge: {margin:.3e} texels")
    assert 7.8e-4 < margin < 8.0e-4  # ~1e12 ulp of u, v: a few ulp of atan2 / asin cannot move a texel
