"""Transmission (glass spheres; rtx_trace_glass): what needs no GPU.

The C ABI entries and their host-side argument checks, the rt::trace_glass op (schema, Meta shapes,
TORCH_CHECKs), the side table and every host refusal of glass.py, build_scene's two optional shader
keys, the restatement (tests/glass_ref.py) pinned to the oracle bit for bit at zero gain, and the
preconditions that keep the GPU cases of tests/test_gpu_glass.py meaningful: how many rays each case
sends through glass and how many pixels of its uint8 frame that changes. For the cases of
tests/test_gpu_glass_limits.py also how many pending rays the kernel's walk holds (G.pending_need)
against the 4B + 4 its stack has, how much glass a frame larger than the pool of workers puts among
the workers' second items, and how many exits of the grazing rays take the clamp.
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
    # the ends of the cap range: 0 (nothing is pushed), 1, 7 and 8 (36 stack entries, the budget-limited pool of
    # workers); the 65-sphere scenes take the culling-tree search, and reach levels 7 and 8 (the README scene stops at 6)
    "cap0": (lambda: scenes.readme_spec(32, 18), _all(0.8), 0, 0, 0, 0),  # the opaque frame
    "cap1": (lambda: scenes.random_spec(16, 1, 48, 27), _all(0.8), 1, 589, 0, 41),
    "cap7": (lambda: scenes.random_spec(64, 2, 48, 27), _all(0.8), 7, 2276, 79, 332),
    "cap8": (lambda: scenes.random_spec(64, 2, 48, 27), _all(0.8), 8, 2318, 83, 332),
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


def _changed_mask(a, b, W, H):
    """Per pixel: does the uint8 frame of ``a`` differ from that of ``b``."""
    return (O.to_uint8(a, W, H) != O.to_uint8(b, W, H)).any(axis=-1).reshape(-1)


def frame_need(spec, gains, cap, iors=None):
    """G.pending_need of the frame of ``spec``: per pixel, the pending-ray stack an unbounded walk holds."""
    osc, g, iors = G.scene_of(spec, gains, iors)
    d = O.ray_directions(osc.cam, osc.width, osc.height)
    return G.pending_need(osc, g, iors, tuple(float(c) for c in osc.cam), d, cap)


# ---- the pending-ray stack at its capacity (tests/test_gpu_glass_limits.py) ----------------------------------

def coincident_spec(k, matt=0):
    """tie_spec's construction (tests/golden/make_golden.py) with k coincident spheres instead of two,
    at 32x18: sphere 1 of the README scene another k - 1 times at index 2, each copy with a constant
    texture of its own and specular_gain 0.6. Every ray that hits one of them is at a k-way tie, and
    with every gain at 0.8 a lit camera ray there pushes 2k rays at B = 1, into a stack of 8. The first
    ``matt`` copies (the last of the tie in scene order) get specular_gain 0.0 instead: no reflected
    ray, one push less each."""
    spec = scenes.readme_spec(32, 18)
    for j in range(k - 1):
        dup = json.loads(json.dumps(spec["spheres"][1]))
        dup["shader"]["texture"] = {"kind": "const", "color": [0.1 + 0.2 * j, 0.9 - 0.2 * j, 0.2 + 0.1 * j]}
        dup["shader"]["specular_gain"] = 0.6 if j >= matt else 0.0
        spec["spheres"].insert(2, dup)
    return spec


_stacks: dict = {}


def stack_case(k, matt=0):
    """(spec, gains, the restatement's frame at B = 1, its counts, the opaque frame, pending_need per
    pixel) of coincident_spec(k, matt) with every gain 0.8, computed once."""
    if (k, matt) not in _stacks:
        spec = coincident_spec(k, matt)
        gains = [0.8] * len(spec["spheres"])
        counts = G.Counts()
        col = G.render(spec, gains, None, 1, counts=counts)
        _stacks[(k, matt)] = (spec, gains, col, counts, O.render(O.scene_from_spec(spec), 1), frame_need(spec, gains, 1))
    return _stacks[(k, matt)]


# ---- frames larger than the pool of workers (a worker's second item) -----------------------------------------

def pool(cap):
    """The largest pool of workers rtx_trace_glass launches at ``cap``, from the library's own workspace
    size: the workspace of a huge ray count holds one stack of 4 cap + 4 rays of 64 bytes per worker."""
    return (int(L.load().rtx_glass_workspace_bytes(1 << 40, cap)) - L.WS_HDR_BYTES) // ((4 * cap + 4) * 64)


# key -> (spec, gains, cap, changed uint8 pixels among the pixels [pool:], the workers' second items). Both
# frames' second laps reach the spheres (640x360 at B = 3 and 480x270 at B = 8 have ground there only: 0).
LAPS = {
    "lap_B3": (lambda: scenes.readme_spec(800, 450), [0.9, 0.9, 0.0], 3, 11025),  # 360,000 rays, a pool of 196,608
    "lap_B8": (lambda: scenes.readme_spec(640, 360), [0.9, 0.9, 0.0], 8, 9554),  # 230,400 rays, a pool of 116,480
}
_laps: dict = {}


def lap_frame(key):
    """(spec, gains, cap, the restatement's frame, the opaque frame, the pool at this cap), computed once.
    Fails, never skips, when the pool was retuned and the frame no longer ends in the second lap."""
    if key not in _laps:
        make, gains, cap = LAPS[key][:3]
        spec = make()
        n, p = spec["camera"]["width"] * spec["camera"]["height"], pool(cap)
        assert p < n < 2 * p, (f"{key}: {n} rays do not end in the second lap of a pool of {p} workers: the pool was "
                               f"retuned, pick another frame (and re-measure LAPS)")
        _laps[key] = (spec, gains, cap, G.render(spec, gains, None, cap), O.render(O.scene_from_spec(spec), cap), p)
    return _laps[key]


# ---- grazing rays: the limb of a glass ball, where the exit's max(..., 0) is taken ---------------------------

GRAZING_RAYS = 200000
# (sphere of the README scene, its specular_ior) -> exits clamped over the whole trace at B = 2 (through_ball
# alone, on every hit of the sphere, clamps 57 / 1,809 / 10,446 of 178,088 and 36 / 745 / 3,895 of 189,473; the
# trace sends 156,796 and 189,473 rays through glass)
GRAZING = {(0, 1.5): 57, (0, 2.4): 1615, (0, 10.0): 9175, (1, 1.5): 36, (1, 2.4): 745, (1, 10.0): 3895}
_grazing: dict = {}


def grazing_rays(si):
    """Parallel rays (0, 0, 1) from z = cz - 5 past the limb of sphere ``si`` of the README scene: impact
    parameter r (1 - eps), eps log-uniform in [1e-16, 1e-6], azimuth uniform. (origins, dirs), 3 arrays each."""
    s = scenes.readme_spec(32, 18)["spheres"][si]
    (cx, cy, cz), r, n = (float(v) for v in s["center"]), float(s["radius"]), GRAZING_RAYS
    rng = np.random.default_rng(1)
    eps = 10.0 ** rng.uniform(-16.0, -6.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    b = r * (1.0 - eps)
    return ((cx + b * np.cos(phi), cy + b * np.sin(phi), np.full(n, cz - 5.0)), (np.zeros(n), np.zeros(n), np.ones(n)))


def grazing_case(si, ior):
    """(spec with the gains, gains, iors, origins, dirs, the restatement's colours at B = 2, its counts) for
    sphere ``si`` made of glass of index ``ior`` with gain 0.9, the others opaque; computed once."""
    if (si, ior) not in _grazing:
        gains, iors = [0.0] * 3, [1.5] * 3
        gains[si], iors[si] = 0.9, ior
        spec = scenes.readme_spec(32, 18)  # (the rays are the caller's: the frame size is not used)
        osc, g, io = G.scene_of(spec, gains, iors)
        o, d = grazing_rays(si)
        counts = G.Counts()
        col = np.stack(G.trace(osc, g, io, o, d, 2, counts=counts))
        _grazing[(si, ior)] = (G.with_gains(spec, gains, iors), gains, iors, o, d, col, counts)
    return _grazing[(si, ior)]


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


def _walked_need(osc, gains, iors, origin, d, cap):
    """pending_need of one ray by the kernel's walk taken literally: a stack of (origin, direction,
    level), pop one, push its rays shape by shape, and the high-water mark of the stack."""
    one = (lambda v: np.array([v], dtype=np.float64))  # noqa: E731
    stack = [(tuple(one(c) for c in origin), tuple(one(c) for c in d), 0)]
    high = 1
    while stack:
        o, dr, level = stack.pop()
        if level >= cap:
            continue
        dist = [O.intersect(sp, *o, *dr) for sp in osc.spheres]
        nearest = min(float(t[0]) for t in dist)
        if nearest == O.FARAWAY:
            continue
        for si, sp in enumerate(osc.spheres):
            if float(dist[si][0]) != nearest:
                continue
            _, _, lit, _, q, r = O._shade(osc, si, sp, *o, *dr, dist[si])
            if bool(np.all(lit)) and sp.specular_gain != 0:
                stack.append((q, r, level + 1))
            if gains[si] != 0:
                c, o2, d2 = G.through_ball(sp, iors[si], *o, *dr, dist[si])
                if c[0] < 0:
                    stack.append((o2, d2, level + 1))
            high = max(high, len(stack))
    return high


def test_pending_need_is_the_walk_taken_literally():
    """The vectorised recursion of G.pending_need against a scalar stack machine, ray by ray, on the two
    frames with ties: five coincident spheres at B = 1 and the golden tie spec at B = 2 (every fourth ray)."""
    for spec, gains, cap, step in ((coincident_spec(5), [0.8] * 7, 1, 1), (_ties_spec(), [0.8] * 4, 2, 4)):
        osc, g, iors = G.scene_of(spec, gains)
        cam = tuple(float(c) for c in osc.cam)
        d = np.stack(O.ray_directions(osc.cam, osc.width, osc.height))[:, ::step]
        need = G.pending_need(osc, g, iors, cam, tuple(d), cap)
        walked = [_walked_need(osc, g, iors, cam, d[:, i], cap) for i in range(d.shape[1])]
        assert need.tolist() == walked
        assert max(walked) > cap + 1  # the ties are in the sample


def test_pending_need_without_and_with_ties():
    for cap in (3, 8):  # no ties: a depth-first walk holds at most one sibling per level
        need = frame_need(scenes.readme_spec(32, 18), [0.9, 0.9, 0.0], cap)
        assert need.min() == 1 and need.max() == 3 <= cap + 1
    spec, gains, cap = frame("ties")[:3]
    need = frame_need(spec, gains, cap)
    assert need.max() == 5 <= 4 * cap + 4  # the 5 of DESIGN.md §14
    assert np.bincount(need).tolist() == [0, 918, 951, 201, 116, 118]


@pytest.mark.parametrize("key", ["cap0", "cap1", "cap7", "cap8"])
def test_the_ends_of_the_cap_range_fit_the_stack(key):
    spec, gains, cap = frame(key)[:3]
    need = frame_need(spec, gains, cap)
    print(f"{key}: the walk holds up to {need.max()} pending rays of {4 * cap + 4}")
    assert need.max() == {"cap0": 1, "cap1": 2, "cap7": 7, "cap8": 7}[key] <= 4 * cap + 4
    if key == "cap0":  # nothing is transmitted: the opaque frame, bit for bit
        assert np.array_equal(frame(key)[3], O.render(O.scene_from_spec(spec), 0))


def test_preconditions_of_the_stack_at_capacity():
    """Four coincident spheres fill the 8 entries of B = 1 exactly on 53 pixels; a fifth overflows them
    on the same 53 and on no other: by 2 entries, or, when it sends no reflected ray, by exactly 1."""
    for k, matt, transmitted, changed, full in ((4, 0, 520, 57, 8), (5, 0, 573, 54, 10), (5, 1, 573, 55, 9)):
        spec, gains, col, counts, plain, need = stack_case(k, matt)
        moved = int(_changed_mask(col, plain, 32, 18).sum())
        print(f"k = {k}, {matt} matt: {counts}, {moved} uint8 pixels changed, need {np.bincount(need).tolist()}")
        assert len(spec["spheres"]) == k + 2 and np.isfinite(col).all()
        assert (counts.transmitted, counts.ties0, counts.ties, counts.deepest, moved) == (transmitted, 53, 55, 1, changed)
        hist = [0] * (full + 1)
        hist[1], hist[2], hist[full] = 231, 292, 53  # rays that push at most one ray, two, and the lit k-way ties
        assert np.bincount(need).tolist() == hist
    over = stack_case(5)[5] > 8
    assert int(over.sum()) == 53 and np.array_equal(over, stack_case(4)[5] == 8)
    assert np.array_equal(over, stack_case(5, 1)[5] == 9)
    assert (stack_case(4)[5] <= 8).all()


@pytest.mark.parametrize("key", sorted(LAPS))
def test_preconditions_of_the_second_lap(key):
    spec, gains, cap, col, plain, p = lap_frame(key)
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    moved = _changed_mask(col, plain, W, H)
    print(f"{key}: pool {p}, {W * H} rays, {int(moved[p:].sum())} of {int(moved.sum())} changed uint8 pixels in lap 2")
    assert int(moved[p:].sum()) == LAPS[key][3] and np.isfinite(col).all()
    assert frame_need(spec, gains, cap).max() == 3 <= 4 * cap + 4


@pytest.mark.parametrize("case", sorted(GRAZING), ids=lambda c: f"sphere{c[0]}-ior{c[1]}")
def test_preconditions_of_the_grazing_rays(case):
    si, ior = case
    spec, gains, iors, o, d, col, counts = grazing_case(si, ior)
    osc = G.scene_of(spec, gains, iors)[0]
    hit = O.intersect(osc.spheres[si], *o, *d) != O.FARAWAY
    print(f"sphere {si}, ior {ior}: {counts}, {int(hit.sum())} rays hit the sphere")
    assert int(hit.sum()) == {0: 178088, 1: 189473}[si]  # the others round to a miss
    assert counts.clamps == GRAZING[case] > 0
    assert counts.inside == 0 and counts.deepest == 2 and counts.ties == 0 and np.isfinite(col).all()
    assert counts.transmitted == {0: 156796, 1: 189473}[si]
    assert G.pending_need(osc, gains, iors, o, d, 2).max() == 2 <= 12


def test_rows_of_the_restatement_are_the_rows_of_the_frame():
    spec, gains, cap, col, _, _ = frame("readme")
    W = spec["camera"]["width"]
    rows = [5, 30, 31, 53]
    got = G.render(spec, gains, None, cap, rows=rows)
    want = col.reshape(3, -1, W)[:, rows].reshape(3, -1)
    assert np.array_equal(got, want)
