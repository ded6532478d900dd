"""Occlusion passes (rtx_occlusion, HipRenderer.render_occlusion): what needs no GPU.

The C ABI entry point and its host-side argument checks, the host tables against their point-by-point
restatement, the frame's orthonormality, the rt::occlusion op (schema, Meta shapes, TORCH_CHECKs), the
restatement (tests/occlusion_ref.py) pinned to aov_ref's ``lit`` at light_radius 0, and the
preconditions that keep the GPU cases of tests/test_gpu_occlusion.py meaningful.
"""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import occlusion, scenes
from python_ray_tracer_amd.camera import lens_table
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import aov_ref, specs
from tests import occlusion_ref as R

REPO = Path(__file__).resolve().parent.parent
W, H = 50, 22

# The scenes of the GPU cases: key -> (spec, side, light_radius, floor of pixels with 0 < ao < 1, floor of
# pixels with 0 < soft_lit < 1). tests/test_gpu_occlusion.py runs them; here the restatement's counts.
SCENES = {
    "rand16": (lambda: scenes.random_spec(16, 1, 64, 36), 3, 2.0, 100, 15),  # 17 spheres: the tree path
    "rand64": (lambda: scenes.random_spec(64, 2, 64, 36), 2, 2.0, 400, 50),
    "rand200": (lambda: scenes.random_spec(200, 3, 48, 27), 2, 2.0, 300, 40),  # above the LDS table's 128
    "fuzz0": (lambda: specs.fuzz_spec(0), 2, 1.0, 15, 15),
    "fuzz3": (lambda: specs.fuzz_spec(3), 2, 1.0, 15, 0),  # camera inside: every pixel hits, no penumbra
    "fuzz15": (lambda: specs.fuzz_spec(15), 2, 1.0, 15, 15),
}
MEASURED = {"rand16": (142, 23), "rand64": (529, 77), "rand200": (384, 61), "fuzz0": (121, 32), "fuzz3": (212, 0),
            "fuzz15": (18, 47)}
README_AO = {1: 0, 2: 352, 3: 506, 8: 631}  # pixels with 0 < ao < 1 of readme_spec(50, 22) by side
MAIN_SOFT = {0.25: (49, 40), 1.0: (174, 150), 2.0: (387, 300)}  # light_radius -> (penumbra pixels, floor)


def PINHOLE():
    """The main scene seen by a pinhole PerspectiveCamera from the side and above, 37 x 23."""
    return scenes.with_camera(scenes.main_spec(37, 23), position=[2.5, 1.5, -1.5], target=[0, 0.3, 3], fov=50.0)


def partial(x) -> int:
    return int(((x > 0) & (x < 1)).sum())


def readme():
    return scenes.readme_spec(W, H)


def main_scene():
    return scenes.main_spec(W, H)


def test_header_declares_and_library_exports_the_entry():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"int rtx_occlusion\(const double\* scene, int n_spheres, const int32_t\* id, const double\* position,\s*"
                     r"const double\* normal, int64_t n, const double\* table, int side, const double\* rot,\s*"
                     r"double max_distance, double light_radius, float\* ao, float\* soft_lit, void\* stream\);", text)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION == 3
    for name, bit in (("AO", L.OCC_AO), ("SOFT", L.OCC_SOFT), ("ALL", L.OCC_ALL)):
        assert int(re.search(rf"RTX_OCC_{name}\s*=\s*(\d+)", text).group(1)) == bit
    assert L.OCC_PASSES == {"ao": 1, "soft_lit": 2} and tuple(L.OCC_PASSES) == R.PASSES == occlusion.PASSES
    p, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert L._SIGS["rtx_occlusion"] == (i32, [p, i32, p, p, p, i64, p, i32, p, f64, f64, p, p, p])
    lib = L.load()
    assert "rtx_occlusion" in L.EXPORTS and hasattr(lib, "rtx_occlusion")


def test_argument_checks_need_no_gpu():
    """Every bad argument returns RTX_E_ARG (-1) with a message before any HIP call, and zero rays
    return RTX_OK without a launch: the pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)

    def occ(scene=p, S=3, ident=p, position=p, normal=p, n=8, table=p, side=3, rot=p, max_distance=1e39,
            light_radius=0.0, ao=p, soft=p):
        return lib.rtx_occlusion(scene, S, ident, position, normal, n, table, side, rot, max_distance, light_radius,
                                 ao, soft, None)

    assert occ(scene=None) == -1 and b"null scene" in lib.rtx_last_error()
    for kw in ({"ident": None}, {"position": None}, {"normal": None}):
        assert occ(**kw) == -1 and b"null primary-hit pass" in lib.rtx_last_error(), kw
    for kw in ({"table": None}, {"rot": None}):
        assert occ(**kw) == -1 and b"null sample table" in lib.rtx_last_error(), kw
    assert occ(ao=None, soft=None) == -1 and b"no pass" in lib.rtx_last_error()
    for S in (0, -1, 1025):
        assert occ(S=S) == -1 and b"n_spheres" in lib.rtx_last_error(), S
    for side in (0, -1, 9):
        assert occ(side=side) == -1 and b"side" in lib.rtx_last_error(), side
    assert occ(n=-1) == -1 and b"negative" in lib.rtx_last_error()
    for d in (0.0, -1.0, 1.0000001e39, float("inf"), float("nan")):
        assert occ(max_distance=d) == -1 and b"max_distance" in lib.rtx_last_error(), d
    for r in (-1e-300, -1.0, float("inf"), float("nan")):
        assert occ(light_radius=r) == -1 and b"light_radius" in lib.rtx_last_error(), r
    # zero rays: nothing to launch (one requested pass is enough to be a valid call)
    assert occ(n=0) == 0 and occ(n=0, ao=None) == 0 and occ(n=0, soft=None, side=8, max_distance=5e-324) == 0


@pytest.mark.parametrize("side", range(1, 9))
def test_hemisphere_table_is_the_restatement(side):
    t = occlusion.hemisphere_table(side)
    assert t.dtype == np.float64 and t.shape == (3, side * side)
    assert np.array_equal(t, R.hemisphere_table_ref(side))
    assert np.array_equal(t[:2], lens_table(side))
    assert (t[2] >= 0).all()
    assert float(np.abs(np.sqrt((t * t).sum(axis=0)) - 1.0).max()) <= 4e-16


def test_rotation_table_is_the_restatement():
    r = occlusion.rotation_table()
    assert r.dtype == np.float64 and r.shape == (2, 64)
    assert np.array_equal(r, R.rotation_table_ref())
    assert float(np.abs(np.sqrt((r * r).sum(axis=0)) - 1.0).max()) <= 4e-16
    assert len({(float(c), float(s)) for c, s in r.T}) == 64


def test_host_argument_checks():
    for bad in (0, 9, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="side"):
            occlusion.check_side(bad)
        with pytest.raises(ValueError, match="side"):
            occlusion.hemisphere_table(bad)
    assert occlusion.check_max_distance(None) == 1e39 == occlusion.check_max_distance(1e39)
    assert occlusion.check_max_distance(0.5) == 0.5
    for bad in (0, -1.0, 1.1e39, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="max_distance"):
            occlusion.check_max_distance(bad)
    assert occlusion.check_light_radius(0) == 0.0 and occlusion.check_light_radius(2.5) == 2.5
    for bad in (-1e-9, float("inf"), float("nan"), None, "1", False):
        with pytest.raises(ValueError, match="light_radius"):
            occlusion.check_light_radius(bad)
    assert occlusion.pass_names(("soft_lit", "ao")) == ("ao", "soft_lit") and occlusion.pass_names("ao") == ("ao",)
    for bad in (("ao", "lit"), ("AO",), (), ["shadow"]):
        with pytest.raises(ValueError, match="passes"):
            occlusion.pass_names(bad)


def test_renderer_signatures_and_names():
    from python_ray_tracer_amd.infrastructure.hip import OCC_NAMES, HipRenderer

    assert OCC_NAMES == R.PASSES
    assert str(inspect.signature(HipRenderer.render_occlusion)) == (
        "(self, scene, passes=('ao', 'soft_lit'), side: 'int' = 3, max_distance: 'float | None' = None, "
        "light_radius: 'float' = 0.0, row_block: 'int' = 1, n_parts: 'int' = 1, part: 'int' = 0, "
        "part_run: 'int' = 1) -> 'dict'")
    assert str(inspect.signature(HipRenderer.trace_occlusion)) == (
        "(self, ray_origin, dirs, scene, passes=('ao', 'soft_lit'), side: 'int' = 3, "
        "max_distance: 'float | None' = None, light_radius: 'float' = 0.0) -> 'dict'")


def test_frame_is_orthonormal():
    """T, B, n within 1e-15 of orthonormal for 200 k random unit vectors and the poles and axes (about
    5.7e-16 measured)."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal((3, 200_000))
    v /= np.sqrt((v * v).sum(axis=0))
    extra = np.array([[0, 0, 1], [0, 0, -1], [1, 0, -0.0], [0.6, 0.8, 0]], dtype=np.float64).T
    n = np.concatenate([v, extra], axis=1)
    T, B = (np.stack(f) for f in R.frame(*n))
    worst = 0.0
    for a, b, want in ((T, T, 1), (B, B, 1), (T, B, 0), (T, n, 0), (B, n, 0)):
        worst = max(worst, float(np.abs((a * b).sum(axis=0) - want).max()))
    print(f"orthonormality: {worst:.3e}")
    assert np.isfinite(T).all() and np.isfinite(B).all() and worst <= 1e-15


def test_hash_spreads_over_the_rotations():
    _, a = aov_ref.frame("readme", readme)
    hit = a["id"] >= 0
    r = [R.rotation_index(*(float(c) for c in a["position"][:, i])) for i in np.nonzero(hit)[0]]
    assert min(r) >= 0 and max(r) <= 63 and len(set(r)) == 64
    assert R.rotation_index(0.0, 0.0, 0.0) == 0 and R.rotation_index(1.0, 2.0, 3.0) != R.rotation_index(3.0, 2.0, 1.0)


def test_op_schema_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "occlusion" in ops.OPS
    assert str(torch.ops.rt.occlusion.default._schema) == \
        ("rt::occlusion(Tensor scene, int n_spheres, Tensor id, Tensor position, Tensor normal, Tensor table, Tensor rot, "
         "float max_distance, float light_radius, int passes, bool check=True) -> Tensor[]")
    S, n = 3, 77

    def args(dev="meta", n=n, side=3, **kw):
        a = dict(scene=torch.zeros(L.HDR_WORDS + S * (L.GEOM_WORDS + L.MAT_WORDS), dtype=torch.float64, device=dev),
                 S=S, id=torch.zeros(n, dtype=torch.int32, device=dev),
                 position=torch.zeros(3, n, dtype=torch.float64, device=dev),
                 normal=torch.zeros(3, n, dtype=torch.float64, device=dev),
                 table=torch.zeros(3, side * side, dtype=torch.float64, device=dev),
                 rot=torch.zeros(2, 64, dtype=torch.float64, device=dev), max_distance=1e39, light_radius=0.0, passes=3)
        a.update(kw)
        return tuple(a.values())

    for mask in (1, 2, 3):
        for side in (1, 3, 8):
            got = torch.ops.rt.occlusion(*args(side=side, passes=mask))
            assert len(got) == bin(mask).count("1")
            for t in got:
                assert tuple(t.shape) == (n,) and t.dtype == torch.float32 and t.device.type == "meta"
    assert [tuple(t.shape) for t in torch.ops.rt.occlusion(*args(n=0))] == [(0,), (0,)]
    for dev in ("cpu", "meta"):
        for mask in (0, 4, -1, 7):
            with pytest.raises(RuntimeError, match="cpu" == dev and "GPU tensor" or "passes"):
                torch.ops.rt.occlusion(*args(dev, passes=mask))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.occlusion(*args("cpu"))
    bad = {
        "too short": dict(S=S + 1),
        "id must be": dict(id=torch.zeros(n, dtype=torch.int64, device="meta")),
        "position must be": dict(position=torch.zeros(3, n + 1, dtype=torch.float64, device="meta")),
        "normal must be": dict(normal=torch.zeros(n, 3, dtype=torch.float64, device="meta")),
        "table must": dict(table=torch.zeros(3, 10, dtype=torch.float64, device="meta")),
        "hemisphere table": dict(table=torch.zeros(2, 9, dtype=torch.float64, device="meta")),
        "rot must be": dict(rot=torch.zeros(2, 32, dtype=torch.float64, device="meta")),
        "max_distance": dict(max_distance=0.0),
        "light_radius": dict(light_radius=-1.0),
    }
    for match, kw in bad.items():
        with pytest.raises(RuntimeError, match=match):
            torch.ops.rt.occlusion(*args(**kw))
    for kw in (dict(table=torch.zeros(3, 81, dtype=torch.float64, device="meta")), dict(max_distance=float("nan")),
               dict(max_distance=2e39), dict(light_radius=float("inf")), dict(light_radius=float("nan"))):
        with pytest.raises(RuntimeError):
            torch.ops.rt.occlusion(*args(**kw))


@pytest.mark.parametrize("key", ["readme", "main", *SCENES])
def test_soft_lit_of_a_point_light_is_lit(key):
    """light_radius = 0: every sample is the reference's own shadow ray, so the restatement's soft_lit
    is aov_ref's lit, exactly, on every scene of the GPU cases."""
    make, side = {"readme": (readme, 3), "main": (main_scene, 3)}.get(key) or SCENES[key][:2]
    o = R.frame_occlusion(key, make, side=side, light_radius=0.0, passes=("soft_lit",))
    assert np.array_equal(o["soft_lit"], o["lit"].astype(np.float32))
    assert int(o["lit"].sum()) > 0


def test_preconditions_of_the_gpu_cases():
    """What the frames of tests/test_gpu_occlusion.py contain, on the restatement: the measured counts
    of partly occluded and penumbra pixels, all above the floors the GPU tests assert."""
    _, a = aov_ref.frame("readme", readme)
    assert (int((a["id"] < 0).sum()), int((a["id"] >= 0).sum())) == (355, 745)
    default = None
    for side, want in README_AO.items():
        o = R.frame_occlusion("readme", readme, side=side, passes=("ao",))
        assert partial(o["ao"]) == want and (o["ao"][a["id"] < 0] == 1).all(), side
        assert side < 2 or want >= 300
        default = o["ao"] if side == 3 else default
    near = R.frame_occlusion("readme", readme, side=3, max_distance=0.5, passes=("ao",))["ao"]
    assert partial(near) == 116 and int(((near == 1) & (a["id"] >= 0)).sum()) == 619
    assert int((near != default).sum()) == 522
    for radius, (want, floor) in MAIN_SOFT.items():
        o = R.frame_occlusion("main", main_scene, side=3, light_radius=radius, passes=("soft_lit",))
        assert partial(o["soft_lit"]) == want >= floor and not o["soft_lit"][o["id"] < 0].any(), radius
    for key, (make, side, radius, ao_floor, soft_floor) in SCENES.items():
        o = R.frame_occlusion(key, make, side=side, light_radius=radius)
        assert (partial(o["ao"]), partial(o["soft_lit"])) == MEASURED[key], key
        assert partial(o["ao"]) >= ao_floor and partial(o["soft_lit"]) >= soft_floor, key
    assert int((R.frame_occlusion("fuzz3", SCENES["fuzz3"][0], side=2, light_radius=1.0)["id"] >= 0).sum()) == 468
    # the pinhole case: its rays from the camera's restatement (tests/camera_ref.py)
    from python_ray_tracer_amd.domain import PerspectiveCamera, Vector3D
    from tests import camera_ref

    spec = PINHOLE()
    c = spec["camera"]
    cam = PerspectiveCamera(Vector3D(*c["position"]), c["width"], c["height"], Vector3D(*c["target"]), fov=c["fov"])
    _, d = camera_ref.rays_ref(cam, 1, range(c["height"]), lens=False)
    oscene = O.scene_from_spec(spec)
    a = aov_ref.aovs(oscene, tuple(float(v) for v in c["position"]), tuple(d))
    o = R.occlusion(oscene, a["id"], a["position"], a["normal"], side=2, light_radius=2.0)
    assert (int((a["id"] >= 0).sum()), partial(o["ao"]), partial(o["soft_lit"])) == (629, 153, 283)
    o = R.frame_occlusion("readme67", lambda: scenes.readme_spec(67, 5), side=2, passes=("ao",))
    assert partial(o["ao"]) == 155
    o = R.frame_occlusion("readme1", lambda: scenes.readme_spec(1, 1), side=2)
    assert o["id"].tolist() == [-1] and o["ao"].tolist() == [1.0] and o["soft_lit"].tolist() == [0.0]
