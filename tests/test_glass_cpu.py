"""Transmission (glass spheres; rtx_trace_glass): what needs no GPU.

The C ABI entries and their host-side argument checks, the rt::trace_glass op (schema, Meta shapes,
TORCH_CHECKs), the side table and every host refusal of glass.py, build_scene's two optional shader
keys, the restatement (tests/glass_ref.py) pinned to the oracle bit for bit at zero gain, and the
preconditions that keep the GPU cases of tests/test_gpu_glass.py meaningful: how many rays each case
sends through glass and how many pixels of its uint8 frame that changes.
"""

import ctypes
import json
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import glass, scenes
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import glass_ref as G
from tests import specs

REPO = Path(__file__).resolve().parent.parent


def _ties_spec():
    return json.loads((REPO / "tests" / "golden" / "scenes.json").read_text())["cases"]["ties_64x36_B2"]["spec"]


def _all(gain):
    return lambda spec: [gain] * len(spec["spheres"])


# The GPU cases: key -> (spec, gains of the spec, bounce cap, transmitted rays, hits from inside, pixels whose
# uint8 frame differs from the same scene's without glass). Measured with the restatement.
CASES = {
    "readme": (lambda: scenes.readme_spec(96, 54), lambda s: [0.9, 0.9, 0.0], 3, 2159, 0, 854),
    "main": (lambda: scenes.main_spec(96, 54), lambda s: [0.9, 0.9, 0.0], 3, 1954, 0, 840),
    "ground": (lambda: scenes.readme_spec(50, 22), _all(0.9), 4, 1335, 0, 224),  # the ground too
    "rand16": (lambda: scenes.random_spec(16, 1, 64, 36), _all(0.8), 6, 1553, 0, 137),  # level 6 reached
    "rand64": (lambda: scenes.random_spec(64, 2, 64, 36),  # the culling tree; every other sphere opaque
               lambda s: [0.8 if i % 2 == 0 else 0.0 for i in range(len(s["spheres"]))], 5, 2277, 0, 474),
    "fuzz0": (lambda: specs.fuzz_spec(0), _all(0.7), 3, 1289, 6, 155),
    "fuzz3": (lambda: specs.fuzz_spec(3), _all(0.7), 3, 940, 468, 61),  # the camera inside a glass ball
    "fuzz15": (lambda: specs.fuzz_spec(15), _all(0.7), 3, 476, 0, 5),
    "ties": (_ties_spec, _all(0.8), 2, 2798, 0, 357),  # 251 rays with two shapes at the nearest distance (226 at level 0)
}

_frames: dict = {}


def frame(key):
    """(spec, gains, cap, restatement's frame, its counts, changed uint8 pixels) of a case, computed once."""
    if key not in _frames:
        make, gains_of, cap = CASES[key][:3]
        spec = make()
        gains = gains_of(spec)
        counts = G.Counts()
        col = G.render(spec, gains, None, cap, counts=counts)
        plain = O.render(O.scene_from_spec(spec), cap)
        W, H = spec["camera"]["width"], spec["camera"]["height"]
        changed = int((O.to_uint8(col, W, H) != O.to_uint8(plain, W, H)).any(axis=-1).sum())
        _frames[key] = (spec, gains, cap, col, counts, changed)
    return _frames[key]


def test_header_declares_and_library_exports_the_entries():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"size_t rtx_glass_workspace_bytes\(int64_t n_rays, int max_bounces\);", text)
    assert re.search(r"int rtx_trace_glass\(const double\* scene, int n_spheres, const double\* glass, const double\* origins,\s*"
                     r"int64_t origin_stride, const double\* dirs, int64_t n, int max_bounces, void\* out,\s*"
                     r"int out_kind, void\* workspace, size_t workspace_bytes, void\* stream\);", text)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION == 3
    assert int(re.search(r"RTX_GLASS_MAX_BOUNCES\s*=\s*(\d+)", text).group(1)) == L.GLASS_MAX_BOUNCES == 8
    assert glass.MAX_BOUNCES == 8
    p, i32, i64, size = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert L._SIGS["rtx_glass_workspace_bytes"] == (size, [i64, i32])
    assert L._SIGS["rtx_trace_glass"] == (i32, [p, i32, p, p, i64, p, i64, i32, p, i32, p, size, p])
    lib = L.load()
    for name in ("rtx_glass_workspace_bytes", "rtx_trace_glass"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_workspace_is_bounded_by_the_pool_of_workers():
    lib = L.load()
    ws = lib.rtx_glass_workspace_bytes
    for B in range(9):
        per = (4 * B + 4) * 8 * 8  # a worker's stack: 4B + 4 pending rays of 8 words
        assert ws(1, B) == L.WS_HDR_BYTES + 64 * per and ws(64, B) == ws(1, B) and ws(65, B) == L.WS_HDR_BYTES + 128 * per
        assert ws(0, B) == L.WS_HDR_BYTES
        big = ws(1 << 40, B)
        assert big == ws(1 << 24, B) and big - L.WS_HDR_BYTES <= 256 << 20  # does not grow with the frame
        assert (big - L.WS_HDR_BYTES) % (64 * per) == 0
    assert ws(10, -1) == 0 and ws(10, 9) == 0 and ws(-1, 3) == 0


def test_argument_checks_need_no_gpu():
    """Every bad argument returns an error code with a message before any HIP call, and zero rays
    return RTX_OK without a launch: the pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)

    def call(scene=p, S=3, table=p, origins=p, stride=0, dirs=p, n=8, B=3, out=p, kind=1, ws=p, ws_bytes=1 << 30):
        return lib.rtx_trace_glass(scene, S, table, origins, stride, dirs, n, B, out, kind, ws, ws_bytes, None)

    assert call(scene=None) == -1 and b"null scene" in lib.rtx_last_error()
    assert call(table=None) == -1 and b"null glass" in lib.rtx_last_error()
    for kw in ({"origins": None}, {"dirs": None}):
        assert call(**kw) == -1 and b"null ray" in lib.rtx_last_error(), kw
    assert call(out=None) == -1 and b"null output" in lib.rtx_last_error()
    assert call(ws=None) == -1 and b"null workspace" in lib.rtx_last_error()
    for S in (0, -1, 1025):
        assert call(S=S) == -1 and b"n_spheres" in lib.rtx_last_error(), S
    for B in (-1, 9, 333):
        assert call(B=B) == -1 and b"max_bounces" in lib.rtx_last_error(), B
    for kind in (-1, 3):
        assert call(kind=kind) == -1 and b"out_kind" in lib.rtx_last_error(), kind
    assert call(n=-1) == -1 and b"negative" in lib.rtx_last_error()
    assert call(stride=5) == -1 and b"origin_stride" in lib.rtx_last_error()
    need = lib.rtx_glass_workspace_bytes(8, 3)
    assert call(ws_bytes=need - 1) == -3 and b"workspace too small" in lib.rtx_last_error()
    # zero rays: nothing to launch
    assert call(n=0) == 0 and call(n=0, B=0, kind=2, ws_bytes=L.WS_HDR_BYTES) == 0 and call(n=0, B=8, kind=0) == 0


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "trace_glass" in ops.OPS
    assert str(torch.ops.rt.trace_glass.default._schema) == \
        ("rt::trace_glass(Tensor scene, int n_spheres, Tensor glass, Tensor origins, Tensor dirs, int max_bounces, "
         "int out_kind, bool check=True) -> Tensor")
    S, n = 3, 77

    def args(dev="meta", **kw):
        a = dict(scene=torch.zeros(L.HDR_WORDS + S * (L.GEOM_WORDS + L.MAT_WORDS), dtype=torch.float64, device=dev),
                 S=S, glass=torch.zeros(2, S, dtype=torch.float64, device=dev),
                 origins=torch.zeros(3, dtype=torch.float64, device=dev),
                 dirs=torch.zeros(3, n, dtype=torch.float64, device=dev), B=3, kind=1)
        a.update(kw)
        return tuple(a.values())

    for kind, shape, dtype in ((0, (3, n), torch.float32), (1, (3, n), torch.float64), (2, (n, 3), torch.uint8)):
        out = torch.ops.rt.trace_glass(*args(kind=kind))
        assert out.device.type == "meta" and tuple(out.shape) == shape and out.dtype == dtype
    out = torch.ops.rt.trace_glass(*args(origins=torch.zeros(3, n, dtype=torch.float64, device="meta")))
    assert tuple(out.shape) == (3, n)
    meta = dict(device="meta", dtype=torch.float64)
    for bad, what in (({"glass": torch.zeros(2, S + 1, **meta)}, "glass"),
                      ({"glass": torch.zeros(2 * S, **meta)}, "glass"),
                      ({"glass": torch.zeros(2, S, device="meta", dtype=torch.float32)}, "glass"),
                      ({"dirs": torch.zeros(n, 3, **meta)}, "dirs"),
                      ({"dirs": torch.zeros(3, n, device="meta", dtype=torch.float32)}, "dirs"),
                      ({"origins": torch.zeros(3, n + 1, **meta)}, "origins"),
                      ({"origins": torch.zeros(4, **meta)}, "origins"),
                      ({"B": -1}, "max_bounces"), ({"B": 9}, "max_bounces"), ({"kind": 3}, "out_kind"),
                      ({"S": 0}, "n_spheres"), ({"S": 4}, "too short"),
                      ({"scene": torch.zeros(2, 200, **meta)}, "1-D")):
        with pytest.raises(RuntimeError, match=what):
            torch.ops.rt.trace_glass(*args(**bad))
    # host tensors: refused before anything is launched
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_glass(*args(dev="cpu"))


def _shape(gain=None, ior=1.5, radius=1.0, **extra):
    sh = types.SimpleNamespace(specular_ior=ior, **extra)
    if gain is not None:
        sh.transmission_gain = gain
    return types.SimpleNamespace(shader=sh, radius=radius)


def test_glass_table_and_its_refusals():
    assert glass.glass_table([_shape(), _shape(0.0), _shape(0), _shape(-0.0)]) is None
    assert not glass.is_transmissive([_shape(), _shape(0.0)]) and glass.is_transmissive([_shape(), _shape(0.25)])
    t = glass.glass_table([_shape(0.9, 1.33), _shape(), _shape(0.5, 1, 99999), _shape(0.0, ior=0.5, radius=-1.0)])
    assert t.dtype == np.float64 and t.shape == (2, 4)
    assert t.tolist() == [[0.9, 0.0, 0.5, 0.0], [1.33, 1.0, 1.0, 1.0]]  # an opaque sphere's index is not read
    assert glass.glass_table([_shape(np.float64(0.5))]).tolist() == [[0.5], [1.5]]
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), "0.5", True, [0.5]):
        with pytest.raises(ValueError, match="transmission_gain"):
            glass.glass_table([_shape(), _shape(bad)])
        assert glass.is_transmissive([_shape(bad)])  # (so that the renderer reaches the refusal)
    none = _shape(0.5)
    none.shader.transmission_gain = None
    assert glass.is_transmissive([none])
    with pytest.raises(ValueError, match="transmission_gain"):
        glass.glass_table([none])
    for bad in (0.999, 0.0, -1.5, float("nan"), float("inf"), "1.5", None):
        with pytest.raises(ValueError, match="specular_ior"):
            glass.glass_table([_shape(0.5, ior=bad)])
    for bad in (0.0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="radius"):
            glass.glass_table([_shape(0.5, radius=bad)])
    glass.glass_table([_shape(0.0, ior=0.5, radius=-5.0)])  # opaque: neither is checked (the reference renders it)


def test_check_bounces():
    assert [glass.check_bounces(b) for b in (0, 3, 8, np.int64(5))] == [0, 3, 8, 5]
    with pytest.raises(ValueError, match="finite bounce cap"):
        glass.check_bounces(None)
    for bad in (9, 333, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_bounces in 0..8"):
            glass.check_bounces(bad)


def test_build_scene_carries_the_two_keys():
    spec = scenes.glass_spec(96, 54)
    assert [s["shader"].get("transmission_gain", 0.0) for s in spec["spheres"]] == [0.5, 0.9, 0.0]
    assert [s["shader"]["diffuse_gain"] for s in spec["spheres"]] == [1.0, 0.1, 1.0]
    plain = scenes.readme_spec(96, 54)
    for a, b in zip(spec["spheres"], plain["spheres"]):  # nothing else differs from the README scene
        sa = {k: v for k, v in a["shader"].items() if k not in ("transmission_gain", "diffuse_gain")}
        sb = {k: v for k, v in b["shader"].items() if k != "diffuse_gain"}
        assert sa == sb and a["center"] == b["center"] and a["radius"] == b["radius"]
    assert spec["lights"] == plain["lights"] and spec["camera"] == plain["camera"]
    try:
        scene = scenes.build_scene(G.with_gains(plain, [0.25, 0.0, 0.5], [1.33, 1.5, 2.0]))
    except ImportError as e:  # the HIP classes need the built library
        pytest.fail(f"the package is not built: {e}")
    assert [s.shader.transmission_gain for s in scene.shapes] == [0.25, 0.0, 0.5]
    assert [s.shader.specular_ior for s in scene.shapes] == [1.33, 1.5, 2.0]
    assert glass.glass_table(scene.shapes).tolist() == [[0.25, 0.0, 0.5], [1.33, 1.0, 2.0]]
    scene = scenes.build_scene(plain)  # without the keys: the defaults, an opaque scene
    assert [s.shader.transmission_gain for s in scene.shapes] == [0.0] * 3
    assert [s.shader.specular_ior for s in scene.shapes] == [1.5] * 3 and glass.glass_table(scene.shapes) is None
    import inspect

    from python_ray_tracer_amd.infrastructure.hip import HipShader

    assert list(inspect.signature(HipShader.__init__).parameters) == [
        "self", "reflection_gain", "specular_gain", "specular_roughness", "iridescence_gain", "diffuse_gain",
        "diffuse_color"]


@pytest.mark.parametrize("scene_name", ["readme", "main"])
@pytest.mark.parametrize("cap", [0, 1, 3, 5])
def test_restatement_is_the_oracle_at_zero_gain(scene_name, cap):
    spec = (scenes.readme_spec if scene_name == "readme" else scenes.main_spec)(96, 54)
    counts = G.Counts()
    got = G.render(spec, [0.0] * 3, None, cap, counts=counts)
    stats = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), cap, stats=stats)
    assert np.array_equal(got, want)
    assert counts.rays == sum(stats.rays) and counts.transmitted == 0 and counts.inside == 0


@pytest.mark.parametrize("key", sorted(CASES))
def test_preconditions_of_the_gpu_cases(key):
    spec, gains, cap, col, counts, changed = frame(key)
    want_t, want_inside, want_changed = CASES[key][3:]
    print(f"{key}: {counts}, {changed} uint8 pixels changed, max {col.max():.4f}")
    assert (counts.transmitted, counts.inside, changed) == (want_t, want_inside, want_changed)
    assert counts.clamps == 0  # the exit's max(..., 0) is never taken: no total internal reflection
    assert counts.deepest == cap and np.isfinite(col).all()
    if key == "ties":  # rays with two shapes at the nearest distance: 226 camera rays, 251 over the three levels
        assert (counts.ties0, counts.ties) == (226, 251)


def test_rows_of_the_restatement_are_the_rows_of_the_frame():
    spec, gains, cap, col, _, _ = frame("readme")
    W = spec["camera"]["width"]
    rows = [5, 30, 31, 53]
    got = G.render(spec, gains, None, cap, rows=rows)
    want = col.reshape(3, -1, W)[:, rows].reshape(3, -1)
    assert np.array_equal(got, want)
