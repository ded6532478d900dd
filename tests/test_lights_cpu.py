"""Several point lights (rtx_trace_lights): what needs no GPU.

The restatement (tests/lights_ref.py) pinned to the oracle bit for bit under one unit light, the table
of the lights and the routing rule (lights.py), the spec keys and scenes.lights_spec, the C ABI entries
and their host-side argument checks, the rt::trace_lights op (schema, Meta shapes, TORCH_CHECKs), every
refusal of the renderer, and the preconditions that keep the GPU cases of tests/test_gpu_lights.py
meaningful: what the lights of each case reach, and that no pixel sits on a quantisation step.
"""

import copy
import ctypes
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import lights, scenes
from python_ray_tracer_amd.domain import ColoredPointLight, DomeLight, PointLight, RGBColor, Vector3D
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import lights_ref as R
from tests import specs

REPO = Path(__file__).resolve().parent.parent
W, H = 50, 22  # the 1,100-pixel README frame of the occlusion tests

# Eight lights on different sides with distinct intensities and colours; a case takes the first k. The
# first is the README scene's own (a plain point light); the second and third are lights_spec's. The seven
# added ones stand higher than the first (50 to 82 degrees above the ground against its 37) and at least a
# quarter turn away from it, so that the ground beside the large sphere has places that only the first light
# reaches, places that only others reach, and, next to where the sphere rests, places that none reaches.
EIGHT = scenes.lights_spec(W, H)["lights"][:1] + scenes.lights_spec(W, H)["lights"][2:] + [
    {"kind": "point", "position": [4.77, 6.87, 5.08], "intensity": 0.5, "color": [0.2, 1.0, 0.3]},
    {"kind": "point", "position": [-4.28, 9.47, 1.69], "intensity": 0.7, "color": [1.0, 0.2, 0.2]},
    {"kind": "point", "position": [2.94, 8.69, 9.75], "intensity": 0.3, "color": [0.9, 0.9, 0.5]},
    {"kind": "point", "position": [-2.07, 7.02, 3.87], "intensity": 0.8, "color": [0.5, 0.3, 0.9]},
    {"kind": "point", "position": [-3.26, 6.59, 6.74], "intensity": 0.25, "color": [0.3, 0.8, 0.8]},
]


def with_lights(spec, k, first_colored=False):
    """``spec`` with its dome lights kept and its point lights replaced by the first ``k`` of EIGHT
    (lights[0] stays first). ``first_colored``: the first as a ColoredPointLight of intensity 1, white."""
    out = copy.deepcopy(spec)
    own = out["lights"][0]
    pts = [dict(own)] + copy.deepcopy(EIGHT[1:k])
    if first_colored:
        pts[0]["intensity"] = 1.0
    out["lights"] = pts[:1] + [li for li in out["lights"] if li["kind"] != "point"] + pts[1:]
    return out


def colored(spec):
    """``spec`` with lights[0] as a ColoredPointLight of intensity 1 and white: a multi-light scene of one
    unit light."""
    out = copy.deepcopy(spec)
    out["lights"][0]["intensity"] = 1.0
    return out


def coincident_spec():
    """The README scene with its small sphere twice: every ray that meets it has two shapes at the nearest
    distance, on every level."""
    spec = scenes.lights_spec(W, H)
    spec["spheres"].insert(2, copy.deepcopy(spec["spheres"][1]))
    return spec


def tree_spec():
    """17 spheres with a culling tree (more than 8), one of them a checker and one image-textured."""
    spec = scenes.random_spec(16, 1, W, H)
    img = specs.textured_spec(W, H)["spheres"][0]["shader"]["texture"]
    spec["spheres"][4]["shader"]["texture"] = {"kind": "checker", "color": [1, 1, 1]}
    spec["spheres"][11]["shader"]["texture"] = copy.deepcopy(img)
    return with_lights(spec, 3)


# The GPU cases against the restatement: key -> (spec, cap). Their frames are computed once and shared.
CASES = {
    "two": (lambda: with_lights(scenes.readme_spec(W, H), 2), 3),
    "three": (lambda: scenes.lights_spec(W, H), 3),
    "eight": (lambda: with_lights(scenes.readme_spec(W, H), 8), 3),
    "ties": (coincident_spec, 3),
    "tree": (tree_spec, 3),
    "1x1": (lambda: scenes.lights_spec(1, 1), 3),
    "7x5": (lambda: scenes.lights_spec(7, 5), 3),
    "67x5": (lambda: scenes.lights_spec(67, 5), 3),
}
_frames: dict = {}


def frame(key):
    """(spec, cap, the restatement's frame float64 [3, n], its counts), computed once."""
    if key not in _frames:
        make, cap = CASES[key]
        spec = make()
        counts = R.Counts()
        _frames[key] = (spec, cap, R.render(spec, cap, counts=counts), counts)
    return _frames[key]


def step_distance(col):
    """The smallest distance of 255 * clip(colour) from an integer it does not sit on exactly: a value
    within 1e-9 of a quantisation step could land on the other side within the 1e-12 parity bar. Exact
    integers (a colour clipped to 1.0, or 0.0) are the same on both sides."""
    v = 255.0 * np.clip(col, 0.0, 1.0)
    frac = np.abs(v - np.rint(v))
    inexact = frac[(frac > 0) & (col < 1.0)]
    return float(inexact.min()) if inexact.size else 1.0


# ---- the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene_name", ["readme", "main", "rand64"])
@pytest.mark.parametrize("cap", [0, 1, 2, 3])
def test_restatement_is_the_oracle_under_one_unit_light(scene_name, cap):
    spec = {"readme": lambda: scenes.readme_spec(W, H), "main": lambda: scenes.main_spec(W, H),
            "rand64": lambda: scenes.random_spec(64, 2, 48, 27)}[scene_name]()  # 65 spheres: a culling tree
    osc = O.scene_from_spec(spec)
    table = np.array([[*osc.light_pos, 1.0, 1.0, 1.0]])
    counts = R.Counts()
    got = R.render(spec, cap, counts=counts, table=table)
    stats = O.TraceStats()
    want = O.render(osc, cap, stats=stats)
    assert np.array_equal(got, want)
    assert counts.rays == sum(stats.rays) and counts.reflected_by_others == 0
    # a last light with e = 0 changes nothing, bitwise
    zero = np.vstack([table, [[-3.0, 4.0, -2.0, 0.0, 0.0, 0.0]]])
    assert np.array_equal(R.render(spec, cap, table=zero), want)


def test_a_zero_light_changes_nothing_among_several():
    spec, cap, want, _ = frame("three")
    table = np.vstack([R.table_of(spec), [[-3.0, 4.0, -2.0, 0.0, 0.0, 0.0]]])
    assert np.array_equal(R.render(spec, cap, table=table), want)


def test_rows_of_the_restatement_are_the_rows_of_the_frame():
    spec, cap, want, _ = frame("three")
    rows = [3, 20, 21, 7]
    assert np.array_equal(R.render(spec, cap, rows=rows), want.reshape(3, H, W)[:, rows].reshape(3, -1))


@pytest.mark.parametrize("key", ["two", "three", "eight"])
def test_preconditions_of_the_gpu_cases(key):
    """Each case has pixels lit by the first light only, by another only, by several and by none, and
    reflected rays that exist only because a light other than lights[0] reaches the hit."""
    spec, cap, col, c = frame(key)
    print(f"{key}: {c}, colours up to {col.max():.3f}, nearest quantisation step {step_distance(col):.3e}")
    assert min(c.first_only, c.other_only, c.several, c.none) > 0
    assert c.reflected_by_others > 0
    assert len(R.table_of(spec)) == {"two": 2, "three": 3, "eight": 8}[key]
    assert np.isfinite(col).all()
    plain = O.render(O.scene_from_spec(spec), cap)  # lights[0] alone
    assert int((O.to_uint8(col, W, H) != O.to_uint8(plain, W, H)).any(axis=-1).sum()) > 100


@pytest.mark.parametrize("key", sorted(CASES))
def test_no_pixel_of_a_gpu_case_sits_on_a_quantisation_step(key):
    spec, cap, col, _ = frame(key)
    assert step_distance(col) > 1e-9


def test_preconditions_of_the_ties_and_the_textures():
    spec, cap, col, c = frame("ties")
    assert c.ties > 50 and cap == 3  # rays with two shapes at the nearest distance, on several levels
    solo = R.Counts()
    R.render(scenes.lights_spec(W, H), cap, counts=solo)
    assert solo.ties == 0
    spec, cap, col, c = frame("tree")
    assert len(spec["spheres"]) == 17 and c.several > 0
    kinds = [s["shader"]["texture"]["kind"] for s in spec["spheres"]]
    assert kinds.count("image") == 1 and kinds.count("checker") == 2  # (the ground is a checker too)
    osc = O.scene_from_spec(spec)
    d = O.ray_directions(osc.cam, W, H)
    dist = [O.intersect(sp, *osc.cam, *d) for sp in osc.spheres]
    nearest = np.minimum.reduce(dist)
    for i in (4, 11):  # both textured spheres are seen by the camera (17 and 28 pixels)
        assert int(((dist[i] == nearest) & (nearest != O.FARAWAY)).sum()) > 10, i


# ---- lights.py and the routing rule -----------------------------------------------------------------------------

def _v(*c):
    return Vector3D(*c)


def test_lights_table_and_the_routing_rule():
    two_plain = [PointLight(_v(1, 2, 3)), PointLight(_v(4, 5, 6))]
    assert lights.lights_table(two_plain) is None and not lights.is_multi_light(two_plain)
    assert lights.lights_table([]) is None
    assert lights.lights_table([DomeLight(0.1, RGBColor(1, 1, 1)), PointLight(_v(1, 2, 3))]) is None
    ls = [PointLight(_v(1, 2, 3)), DomeLight(0.1, RGBColor(1, 1, 1)),
          ColoredPointLight(_v(-1, 0, 2), 0.5, RGBColor(1.0, 0.5, 0.25)),
          ColoredPointLight(_v(7, 8, 9)), ColoredPointLight(_v(0, 0, 0), 2, (0.1, 0.2, 0.3)),
          types.SimpleNamespace(position=_v(3, 3, 3))]  # a foreign object with a position: a plain point light
    assert lights.is_multi_light(ls)
    t = lights.lights_table(ls)
    assert t.dtype == np.float64 and t.shape == (5, 6)  # list order kept, the dome light skipped
    assert t.tolist() == [[1, 2, 3, 1, 1, 1], [-1, 0, 2, 0.5, 0.25, 0.125], [7, 8, 9, 1, 1, 1],
                          [0, 0, 0, 2 * 0.1, 2 * 0.2, 2 * 0.3], [3, 3, 3, 1, 1, 1]]
    assert ColoredPointLight(_v(0, 0, 0)).intensity == 1.0 and ColoredPointLight(_v(0, 0, 0)).color == (1.0, 1.0, 1.0)
    assert isinstance(ColoredPointLight(_v(0, 0, 0)), PointLight)
    assert lights.lights_table([ColoredPointLight(_v(0, 0, 0), 0.0, (0, 0, 0))]).tolist() == [[0, 0, 0, 0, 0, 0]]
    for bad in (float("nan"), float("inf"), -float("inf")):
        for li in (ColoredPointLight(_v(bad, 0, 0)), ColoredPointLight(_v(0, 0, 0), bad),
                   ColoredPointLight(_v(0, 0, 0), 1.0, (1.0, bad, 1.0)),
                   ColoredPointLight(_v(0, 0, 0), 1.0, RGBColor(1.0, 1.0, bad))):
            with pytest.raises(ValueError, match="finite"):
                lights.lights_table([PointLight(_v(1, 2, 3)), li])
    with pytest.raises(ValueError, match="finite"):  # a plain light's position is checked too
        lights.lights_table([PointLight(_v(1, float("nan"), 3)), ColoredPointLight(_v(0, 0, 0))])
    for li in (ColoredPointLight(_v(0, 0, 0), -0.5), ColoredPointLight(_v(0, 0, 0), 1.0, (1.0, -0.1, 1.0))):
        with pytest.raises(ValueError, match=">= 0"):
            lights.lights_table([li])
    for li in (ColoredPointLight(_v(0, 0, 0), "1"), ColoredPointLight(_v(0, 0, 0), True),
               ColoredPointLight(_v(0, 0, 0), 1.0, (1.0, None, 1.0)), ColoredPointLight(_v(0, 0, 0), 1.0, (1.0, 1.0))):
        with pytest.raises(ValueError):
            lights.lights_table([li])
    assert lights.MAX_LIGHTS == 8
    eight = [ColoredPointLight(_v(i, 0, 0)) for i in range(8)]
    assert lights.lights_table(eight + [DomeLight(0.1, RGBColor(1, 1, 1))]).shape == (8, 6)
    with pytest.raises(ValueError, match="at most 8 point lights"):
        lights.lights_table(eight + [PointLight(_v(9, 0, 0))])


def test_check_bounces():
    assert lights.MAX_BOUNCES == 16
    assert [lights.check_bounces(b) for b in (0, 3, 16, np.int64(5))] == [0, 3, 16, 5]
    with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
        lights.check_bounces(None)
    for bad in (17, 333, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
            lights.check_bounces(bad)


def test_specs_and_build_scene():
    spec = scenes.lights_spec(96, 54)
    plain = scenes.readme_spec(96, 54)
    assert spec["spheres"] == plain["spheres"] and spec["camera"] == plain["camera"]
    assert spec["lights"][:2] == plain["lights"] and len(spec["lights"]) == 4
    assert all(li["kind"] == "point" and "intensity" in li and "color" in li for li in spec["lights"][2:])
    scene = scenes.build_scene(spec)
    kinds = [type(li).__name__ for li in scene.lights]
    assert kinds == ["PointLight", "DomeLight", "ColoredPointLight", "ColoredPointLight"]
    assert np.array_equal(lights.lights_table(scene.lights), R.table_of(spec))
    assert lights.lights_table(scenes.build_scene(plain).lights) is None
    # either key alone makes the entry a ColoredPointLight; the oracle reads kind and position only
    for extra in ({"intensity": 0.5}, {"color": [0.5, 0.25, 1.0]}):
        s = copy.deepcopy(plain)
        s["lights"][0].update(extra)
        li = scenes.build_scene(s).lights[0]
        assert isinstance(li, ColoredPointLight)
        assert li.intensity == extra.get("intensity", 1.0)
        assert li.color.components() == tuple(extra.get("color", (1.0, 1.0, 1.0)))
        assert O.scene_from_spec(s).light_pos == O.scene_from_spec(plain).light_pos
    for k in (1, 2, 8):
        s = with_lights(plain, k, first_colored=True)
        assert lights.lights_table(scenes.build_scene(s).lights).shape == (k, 6)


# ---- the C ABI --------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entries():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"size_t rtx_lights_workspace_bytes\(int64_t n_rays, int max_bounces\);", text)
    assert re.search(r"int rtx_trace_lights\(const double\* scene, int n_spheres, const double\* lights, int n_lights,\s*"
                     r"const double\* origins, int64_t origin_stride, const double\* dirs, int64_t n,\s*"
                     r"int max_bounces, void\* out, int out_kind, void\* workspace, size_t workspace_bytes,\s*"
                     r"void\* stream\);", text)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION == 3
    assert int(re.search(r"RTX_MAX_POINT_LIGHTS\s*=\s*(\d+)", text).group(1)) == L.MAX_POINT_LIGHTS == lights.MAX_LIGHTS
    assert int(re.search(r"RTX_LIGHTS_MAX_BOUNCES\s*=\s*(\d+)", text).group(1)) == L.LIGHTS_MAX_BOUNCES == 16
    p, i32, i64, size = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert L._SIGS["rtx_lights_workspace_bytes"] == (size, [i64, i32])
    assert L._SIGS["rtx_trace_lights"] == (i32, [p, i32, p, i32, p, i64, p, i64, i32, p, i32, p, size, p])
    lib = L.load()
    for name in ("rtx_lights_workspace_bytes", "rtx_trace_lights"):
        assert name in L.EXPORTS and hasattr(lib, name)


def pool(cap):
    """The largest pool of workers rtx_trace_lights launches at ``cap``, from the library's own workspace
    size: the workspace of a huge ray count holds one stack of 2 cap + 2 rays of 80 bytes per worker."""
    return (int(L.load().rtx_lights_workspace_bytes(1 << 40, cap)) - L.WS_HDR_BYTES) // ((2 * cap + 2) * 80)


def test_workspace_is_bounded_by_the_pool_of_workers():
    ws = L.load().rtx_lights_workspace_bytes
    for B in range(17):
        per = (2 * B + 2) * 10 * 8  # a worker's stack: 2B + 2 pending rays of 10 words
        assert ws(1, B) == L.WS_HDR_BYTES + 64 * per and ws(64, B) == ws(1, B) and ws(65, B) == L.WS_HDR_BYTES + 128 * per
        assert ws(0, B) == L.WS_HDR_BYTES
        big = ws(1 << 40, B)
        assert big == ws(1 << 24, B) and big - L.WS_HDR_BYTES <= 256 << 20  # does not grow with the frame
        assert (big - L.WS_HDR_BYTES) % (64 * per) == 0
    assert ws(10, -1) == 0 and ws(10, 17) == 0 and ws(-1, 3) == 0
    assert pool(0) == pool(3) == 196608 and pool(16) % 64 == 0


def test_argument_checks_need_no_gpu():
    """Every bad argument returns an error code with a message before any HIP call, and zero rays
    return RTX_OK without a launch: the pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)

    def call(scene=p, S=3, table=p, nl=2, origins=p, stride=0, dirs=p, n=8, B=3, out=p, kind=1, ws=p, ws_bytes=1 << 30):
        return lib.rtx_trace_lights(scene, S, table, nl, origins, stride, dirs, n, B, out, kind, ws, ws_bytes, None)

    assert call(scene=None) == -1 and b"null scene" in lib.rtx_last_error()
    assert call(table=None) == -1 and b"null lights" in lib.rtx_last_error()
    for kw in ({"origins": None}, {"dirs": None}):
        assert call(**kw) == -1 and b"null ray" in lib.rtx_last_error(), kw
    assert call(out=None) == -1 and b"null output" in lib.rtx_last_error()
    assert call(ws=None) == -1 and b"null workspace" in lib.rtx_last_error()
    for S in (0, -1, 1025):
        assert call(S=S) == -1 and b"n_spheres" in lib.rtx_last_error(), S
    for nl in (0, -1, 9):
        assert call(nl=nl) == -1 and b"n_lights" in lib.rtx_last_error(), nl
    for B in (-1, 17, 333):
        assert call(B=B) == -1 and b"max_bounces" in lib.rtx_last_error(), B
    for kind in (-1, 3):
        assert call(kind=kind) == -1 and b"out_kind" in lib.rtx_last_error(), kind
    assert call(n=-1) == -1 and b"negative" in lib.rtx_last_error()
    assert call(stride=5) == -1 and b"origin_stride" in lib.rtx_last_error()
    need = lib.rtx_lights_workspace_bytes(8, 3)
    assert call(ws_bytes=need - 1) == -3 and b"workspace too small" in lib.rtx_last_error()
    assert call(n=1 << 30, B=16, ws_bytes=lib.rtx_lights_workspace_bytes(1 << 30, 16) - 1) == -3
    # zero rays: nothing to launch
    assert call(n=0) == 0 and call(n=0, B=0, kind=2, ws_bytes=L.WS_HDR_BYTES) == 0 and call(n=0, B=16, kind=0, nl=8) == 0


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "trace_lights" in ops.OPS
    assert str(torch.ops.rt.trace_lights.default._schema) == \
        ("rt::trace_lights(Tensor scene, int n_spheres, Tensor lights, Tensor origins, Tensor dirs, int max_bounces, "
         "int out_kind, bool check=True) -> Tensor")
    S, n = 3, 77

    def args(dev="meta", **kw):
        a = dict(scene=torch.zeros(L.HDR_WORDS + S * (L.GEOM_WORDS + L.MAT_WORDS), dtype=torch.float64, device=dev),
                 S=S, lights=torch.zeros(3, 6, dtype=torch.float64, device=dev),
                 origins=torch.zeros(3, dtype=torch.float64, device=dev),
                 dirs=torch.zeros(3, n, dtype=torch.float64, device=dev), B=3, kind=1)
        a.update(kw)
        return tuple(a.values())

    for kind, shape, dtype in ((0, (3, n), torch.float32), (1, (3, n), torch.float64), (2, (n, 3), torch.uint8)):
        out = torch.ops.rt.trace_lights(*args(kind=kind))
        assert out.device.type == "meta" and tuple(out.shape) == shape and out.dtype == dtype
    out = torch.ops.rt.trace_lights(*args(origins=torch.zeros(3, n, dtype=torch.float64, device="meta"), B=16))
    assert tuple(out.shape) == (3, n)
    meta = dict(device="meta", dtype=torch.float64)
    for bad, what in (({"lights": torch.zeros(3, 5, **meta)}, "lights"),
                      ({"lights": torch.zeros(18, **meta)}, "lights"),
                      ({"lights": torch.zeros(0, 6, **meta)}, "lights"),
                      ({"lights": torch.zeros(9, 6, **meta)}, "lights"),
                      ({"lights": torch.zeros(3, 6, device="meta", dtype=torch.float32)}, "lights"),
                      ({"dirs": torch.zeros(n, 3, **meta)}, "dirs"),
                      ({"dirs": torch.zeros(3, n, device="meta", dtype=torch.float32)}, "dirs"),
                      ({"origins": torch.zeros(3, n + 1, **meta)}, "origins"),
                      ({"origins": torch.zeros(4, **meta)}, "origins"),
                      ({"B": -1}, "max_bounces"), ({"B": 17}, "max_bounces"), ({"kind": 3}, "out_kind"),
                      ({"S": 0}, "n_spheres"), ({"S": 4}, "too short"),
                      ({"scene": torch.zeros(2, 200, **meta)}, "1-D")):
        with pytest.raises(RuntimeError, match=what):
            torch.ops.rt.trace_lights(*args(**bad))
    # host tensors: refused before anything is launched
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.trace_lights(*args(dev="cpu"))


# ---- the renderer's refusals ------------------------------------------------------------------------------------

class _NoDevice:
    """Stands where the renderer keeps its library and its device: any use of either fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after a use of the library or the device ({name})")


def _renderer(monkeypatch, **kw):
    """A HipRenderer that never saw its constructor (which needs the GPU), with the fields the host
    refusals read; every torch.cuda call and every use of the library or the device fails."""
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer

    def no_gpu(*a, **k):
        raise AssertionError("the refusal came after a torch.cuda call")

    for name in ("current_device", "set_device", "current_stream", "is_current_stream_capturing"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    r = object.__new__(HipRenderer)
    fields = dict(_lib=_NoDevice(), device=_NoDevice(), max_bounces=3, samples=1, adaptive=False, color_dtype=torch.float64,
                  _light_tables=_NoDevice(), _glass_tables=_NoDevice(), _scene_cache=_NoDevice())
    fields.update(kw)
    r.__dict__.update(fields)
    return r


def test_every_refusal_of_the_renderer_comes_before_any_gpu_use(monkeypatch):
    from python_ray_tracer_amd.infrastructure.hip import HipVector3D

    scene = scenes.build_scene(scenes.lights_spec(W, H))
    plain = scenes.build_scene(scenes.readme_spec(W, H))
    r = _renderer(monkeypatch)
    with pytest.raises(ValueError, match="render_batch.*ColoredPointLight.*one by one"):
        r.render_batch([plain, scene])
    with pytest.raises(ValueError, match=r"submit_tiles.*ColoredPointLight.*TileGather\(native=False\)"):
        r.submit_tiles(None, 0, scene, 1, 1, 0, None)
    o = scene.camera.position
    d = HipVector3D(np.array([0.0]), np.array([0.0]), np.array([1.0]))
    with pytest.raises(ValueError, match="shade_hits.*ColoredPointLight.*render the scene"):
        r.shade_hits(scene.shapes[0], scene, o, d, np.array([1.0]))
    with pytest.raises(ValueError, match="shade_hits.*ColoredPointLight"):
        scene.shapes[0].shader.create(scene.shapes[0], scene, o, d, np.array([1.0]), ray_tracer=r)
    with pytest.raises(ValueError, match="blob.*ColoredPointLight.*packs the scene itself"):
        r.render_tile(scene, blob=torch.zeros(8, dtype=torch.float64), n_spheres=3)
    for call in (r.render, r.render_tile, lambda s: r.raytrace_scene(o, d, s)):
        for cap in (None, 17):
            r.max_bounces = cap
            with pytest.raises(ValueError, match=r"HipRenderer\(max_bounces=B\)"):
                call(scene)
    r.max_bounces = 3
    r.adaptive, r.samples = True, 2
    with pytest.raises(ValueError, match="ColoredPointLight.*adaptive=False"):
        r.render(scene)
    r.adaptive, r.samples = False, 1
    both = scenes.build_scene(scenes.lights_spec(W, H))
    both.shapes[1].shader.transmission_gain = 0.9
    for call in (r.render, lambda s: r.raytrace_scene(o, d, s)):
        with pytest.raises(ValueError, match="ColoredPointLight and a transmissive sphere.*plain\\s+PointLights"):
            call(both)
    # a bad light is refused by every entry, whatever it would do with the scene
    bad = scenes.build_scene(scenes.lights_spec(W, H))
    bad.lights[2].intensity = -1.0
    for call in (r.render, lambda s: r.render_batch([s]), lambda s: r.raytrace_scene(o, d, s)):
        with pytest.raises(ValueError, match=">= 0"):
            call(bad)
    nine = scenes.build_scene(scenes.lights_spec(W, H))
    nine.lights += [ColoredPointLight(HipVector3D(i, 5, 0)) for i in range(6)]
    with pytest.raises(ValueError, match="at most 8 point lights"):
        r.render(nine)
    # lights[0] must still be a point light: the packer's AttributeError stays (a scene without lights has no
    # ColoredPointLight either: its IndexError is the one-light path's, as before)
    from python_ray_tracer_amd.infrastructure.hip.scene_pack import scene_key

    broken = scenes.build_scene(scenes.lights_spec(W, H))
    broken.lights = broken.lights[1:]  # the dome light first
    assert lights.lights_table(broken.lights).shape == (2, 6)
    with pytest.raises(AttributeError):
        scene_key(broken)
    empty = scenes.build_scene(scenes.lights_spec(W, H))
    empty.lights = []
    assert lights.lights_table(empty.lights) is None
    with pytest.raises(IndexError):
        scene_key(empty)


def test_the_new_methods_live_in_the_base_class():
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer, base

    assert base._LightScenes in HipRenderer.__mro__
    for name in ("_lights_table", "_lights_workspace", "_trace_lights"):
        assert name in vars(base._LightScenes) and name not in vars(HipRenderer)
    for method in (HipRenderer.render_aovs, HipRenderer.render_occlusion, HipRenderer.edge_mask):
        assert "multi-light scene" in method.__doc__ and "lights[0]" in method.__doc__


def test_the_row_tile_gather_of_a_multi_light_scene_goes_through_render_tile(monkeypatch):
    """render_image_pipeline on several ranks: tile_gather_for asks for the render_tile(into=) path, never the
    native plan (submit_tiles refuses a multi-light scene); a plain scene keeps the default."""
    import torch.distributed as dist

    from python_ray_tracer_amd import distributed

    made = []

    class Gather:
        def __init__(self, renderer, width, height, **kw):
            made.append(kw["native"])

    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(distributed, "TileGather", Gather)
    distributed.tile_gather_for(types.SimpleNamespace(), scenes.build_scene(scenes.lights_spec(W, H)))
    distributed.tile_gather_for(types.SimpleNamespace(), scenes.build_scene(scenes.readme_spec(W, H)))
    assert made == [False, None]
