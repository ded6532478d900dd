"""Adaptive anti-aliasing (HipRenderer(samples=k, adaptive=True); rtx_edge_mask, rtx_sample_dirs,
rtx_resolve_scatter): what needs no GPU.

The constructor's and the methods' refusals, the C ABI entry points and their host-side argument
checks, the rt::edge_mask / sample_dirs / resolve_scatter ops (schemas, Meta shapes, TORCH_CHECKs),
the planning guard and the NumPy restatement (tests/adaptive_ref.py) on hand-made frames.
"""

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from python_ray_tracer_amd import scenes, tiling
from python_ray_tracer_amd.infrastructure.hip import HipRenderer
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import adaptive_ref as A

REPO = Path(__file__).resolve().parent.parent
NEW = ("rtx_edge_mask", "rtx_sample_dirs", "rtx_resolve_scatter")


def test_constructor_refusals_come_before_the_library_and_the_gpu():
    for kw in ({"samples": 1, "adaptive": True}, {"adaptive": True}):
        with pytest.raises(ValueError, match="adaptive"):
            HipRenderer(3, **kw)
    for bad in (1, 0, "yes", None, 2.0):
        with pytest.raises(ValueError, match="adaptive"):
            HipRenderer(3, samples=2, adaptive=bad)
    for bad in (-1e-9, -1, float("nan"), float("inf"), -float("inf"), "0.1", True, [0.1]):
        with pytest.raises(ValueError, match="contrast"):
            HipRenderer(3, samples=2, adaptive=True, contrast=bad)
        with pytest.raises(ValueError, match="contrast"):  # checked whether or not it is used
            HipRenderer(3, contrast=bad)
    assert tiling.check_adaptive(True, 2, None) == (True, math.inf)
    assert tiling.check_adaptive(True, 8, 0) == (True, 0.0)
    assert tiling.check_adaptive(False, 1, 0.0625) == (False, 0.0625)
    assert tiling.check_adaptive(np.bool_(True), 3, np.float32(0.25)) == (True, 0.25)
    import inspect

    sig = inspect.signature(HipRenderer.__init__).parameters
    assert sig["adaptive"].default is False and sig["contrast"].default == 0.0625 == 1 / 16


def _bare(**attrs):
    """A HipRenderer that never saw its constructor (no library, no device): a refusal that reaches
    for either would fail with something other than the ValueError asked for."""
    r = object.__new__(HipRenderer)
    for k, v in {"samples": 2, "adaptive": True, **attrs}.items():
        setattr(r, k, v)
    return r


def test_method_refusals_come_before_any_gpu_use():
    scene = scenes.build_scene(scenes.readme_spec(8, 4))
    r = _bare()
    for kw in ({"n_parts": 2}, {"n_parts": 3, "part": 1}, {"row_block": 4, "n_parts": 2, "part": 1, "out": "u8"}):
        with pytest.raises(ValueError, match="adaptive"):
            r.render_tile(scene, **kw)
    with pytest.raises(ValueError, match="adaptive"):
        r.render_tile(scene, 4, 2, 0)
    with pytest.raises(ValueError, match="adaptive"):
        r.render_tile(scene, blob=torch.zeros(200, dtype=torch.float64), n_spheres=3)
    with pytest.raises(ValueError, match="adaptive"):
        r.render_batch([scene, scene])
    with pytest.raises(ValueError, match="adaptive"):
        r.render_batch([scene], out="u8")
    with pytest.raises(ValueError, match="adaptive"):
        r.submit_tiles(None, 0, scene, 4, 1, 0, None)
    # what samples >= 2 refuses stays refused (an adaptive renderer has samples >= 2)
    from python_ray_tracer_amd.infrastructure.hip import HipVector3D

    with pytest.raises(ValueError, match="samples=2"):
        r.raytrace_scene(scene.camera.position, HipVector3D(0.0, 0.0, 1.0), scene)
    for what in ("shade_hits", "render_aovs", "trace_aovs"):
        with pytest.raises(ValueError, match="samples=2"):
            r._need_camera(what)


def test_frame_and_ray_count_guard():
    assert tiling.check_adaptive_count(4, 1920, 1080) == 0
    assert tiling.check_adaptive_count(4, 1920, 1080, 0) == 0
    assert tiling.check_adaptive_count(4, 1920, 1080, 1000) == 16000
    assert tiling.check_adaptive_count(8, 7680, 4320, 7680 * 4320) == 64 * 7680 * 4320 < 2**31
    assert tiling.check_adaptive_count(2, 1 << 15, 1 << 14, (1 << 29) - 1) == 2**31 - 4
    with pytest.raises(ValueError, match="2\\^31"):
        tiling.check_adaptive_count(2, 1 << 16, 1 << 15)  # the frame alone: exactly 2^31 pixels
    with pytest.raises(ValueError, match="2\\^31"):
        tiling.check_adaptive_count(2, 1 << 15, 1 << 14, 1 << 29)  # exactly 2^31 sample rays
    with pytest.raises(ValueError, match="2\\^31"):
        tiling.check_adaptive_count(8, 8192, 8192, 8192 * 8192)
    with pytest.raises(ValueError, match="flagged"):
        tiling.check_adaptive_count(2, 4, 4, 17)  # more flagged pixels than pixels
    with pytest.raises(ValueError, match="flagged"):
        tiling.check_adaptive_count(2, 4, 4, -1)


def test_header_sigs_and_exports_agree_and_the_abi_is_still_3():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"int rtx_edge_mask\(const double\* color_f64, const int32_t\* id, const int32_t\* hits, "
                     r"const uint8_t\* lit,\s*int width, int height, double contrast, uint8_t\* mask_out, "
                     r"void\* stream\);", text)
    assert re.search(r"int rtx_sample_dirs\(const double\* sample_scene, int k, int width, int height, "
                     r"const int32_t\* pixels_i32,\s*int n_flagged, double\* dirs_out, void\* stream\);", text)
    assert re.search(r"int rtx_resolve_scatter\(const double\* samples_f64, int k, const int32_t\* pixels_i32, "
                     r"int n_flagged,\s*int width, int height, void\* out, int out_kind, void\* stream\);", text)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION == 3
    p, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert L._SIGS["rtx_edge_mask"] == (i32, [p, p, p, p, i32, i32, f64, p, p])
    assert L._SIGS["rtx_sample_dirs"] == (i32, [p, i32, i32, i32, p, i32, p, p])
    assert L._SIGS["rtx_resolve_scatter"] == (i32, [p, i32, p, i32, i32, i32, p, i32, p])
    lib = L.load()
    layout = (ctypes.c_int * 8)()
    assert lib.rtx_abi_version(layout, 8) == 3
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value


def test_argument_checks_need_no_gpu():
    """Every bad argument returns RTX_E_ARG (-1) with a message before any HIP call, and zero flagged
    pixels return RTX_OK without a launch: the pointers below are never dereferenced."""
    lib = L.load()
    p = ctypes.c_void_p(4096)
    err = lib.rtx_last_error

    def mask(color=p, ident=p, hits=p, lit=p, width=8, height=4, contrast=0.0625, out=p):
        return lib.rtx_edge_mask(color, ident, hits, lit, width, height, contrast, out, None)

    def dirs(scene=p, k=2, width=8, height=4, pixels=p, n=5, out=p):
        return lib.rtx_sample_dirs(scene, k, width, height, pixels, n, out, None)

    def scatter(samples=p, k=2, pixels=p, n=5, width=8, height=4, out=p, kind=L.OUT_F64_SOA):
        return lib.rtx_resolve_scatter(samples, k, pixels, n, width, height, out, kind, None)

    for name in ("color", "ident", "hits", "lit", "out"):
        assert mask(**{name: None}) == -1 and b"null" in err(), name
    for name in ("scene", "pixels", "out"):
        assert dirs(**{name: None}) == -1 and b"null" in err(), name
    for name in ("samples", "pixels", "out"):
        assert scatter(**{name: None}) == -1 and b"null" in err(), name
    for kw in ({"width": 0}, {"width": -3}, {"height": 0}, {"height": -1}, {"width": 1 << 16, "height": 1 << 15},
               {"width": 2**31 - 1, "height": 2**31 - 1}):
        assert mask(**kw) == -1 and b"geometry" in err(), kw
        assert dirs(**kw) == -1 and b"geometry" in err(), kw
        assert scatter(**kw) == -1 and b"geometry" in err(), kw
    for c in (-1e-300, -1.0, -math.inf, math.nan):
        assert mask(contrast=c) == -1 and b"contrast" in err(), c
    for k in (0, -1, 9, 64):
        assert dirs(k=k) == -1 and b"1..8" in err(), k
        assert scatter(k=k) == -1 and b"1..8" in err(), k
    for kind in (-1, 3, 17):
        assert scatter(kind=kind) == -1 and b"out_kind" in err(), kind
    for n in (-1, -(2**31)):
        assert dirs(n=n) == -1 and b"negative" in err(), n
        assert scatter(n=n) == -1 and b"negative" in err(), n
    # n_flagged*k*k >= 2^31: exactly 2^31 and beyond, in a frame large enough to hold the pixels
    big = {"width": 1 << 15, "height": 1 << 15}
    for k, n in ((2, 1 << 29), (4, 1 << 27), (8, 1 << 25), (3, 238609295), (8, 2**31 - 1)):
        assert n * k * k >= 2**31
        assert dirs(k=k, n=n, **big) == -1 and b"2^31" in err(), (k, n)
        assert scatter(k=k, n=n, **big) == -1 and b"2^31" in err(), (k, n)
    # no flagged pixel: nothing to launch (and no list to point at)
    assert dirs(n=0) == 0 and dirs(n=0, pixels=None) == 0
    assert scatter(n=0) == 0 and scatter(n=0, pixels=None) == 0
    for kind in (L.OUT_F32_SOA, L.OUT_F64_SOA, L.OUT_U8_HWC):
        assert scatter(n=0, kind=kind) == 0


def test_op_schemas_meta_shapes_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    for name in ("edge_mask", "sample_dirs", "resolve_scatter"):
        assert name in ops.OPS
    assert str(torch.ops.rt.edge_mask.default._schema) == \
        "rt::edge_mask(Tensor color, Tensor id, Tensor hits, Tensor lit, int width, int height, float contrast) -> Tensor"
    assert str(torch.ops.rt.sample_dirs.default._schema) == \
        "rt::sample_dirs(Tensor sample_scene, int k, int width, int height, Tensor pixels) -> Tensor"
    assert str(torch.ops.rt.resolve_scatter.default._schema) == \
        ("rt::resolve_scatter(Tensor samples, int k, Tensor pixels, int width, int height, Tensor(a!) out, "
         "int out_kind) -> ()")
    W, H, k, nf = 7, 5, 3, 11
    n = W * H

    def frame(dev, n=n, color=torch.float64, ident=torch.int32, lit=torch.uint8):
        return (torch.zeros(3, n, dtype=color, device=dev), torch.zeros(n, dtype=ident, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=lit, device=dev))

    m = torch.ops.rt.edge_mask(*frame("meta"), W, H, 0.0625)
    assert tuple(m.shape) == (n,) and m.dtype == torch.uint8 and m.device.type == "meta"
    assert tuple(torch.ops.rt.edge_mask(*frame("meta"), W, H, math.inf).shape) == (n,)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.edge_mask(*frame("cpu"), W, H, 0.0625)
    for bad in ({"n": n - 1}, {"color": torch.float32}, {"ident": torch.int64}, {"lit": torch.bool}):
        with pytest.raises(RuntimeError):
            torch.ops.rt.edge_mask(*frame("meta", **bad), W, H, 0.0625)
    with pytest.raises(RuntimeError, match="contrast"):
        torch.ops.rt.edge_mask(*frame("meta"), W, H, -0.5)
    with pytest.raises(RuntimeError, match="contrast"):
        torch.ops.rt.edge_mask(*frame("meta"), W, H, math.nan)
    with pytest.raises(RuntimeError, match="geometry"):
        torch.ops.rt.edge_mask(*frame("meta"), 0, H, 0.0625)

    blob = torch.empty(L.HDR_WORDS, dtype=torch.float64, device="meta")
    pix = torch.empty(nf, dtype=torch.int32, device="meta")
    d = torch.ops.rt.sample_dirs(blob, k, W, H, pix)
    assert tuple(d.shape) == (3, nf * k * k) and d.dtype == torch.float64 and d.device.type == "meta"
    assert tuple(torch.ops.rt.sample_dirs(blob, 1, W, H, pix[:0]).shape) == (3, 0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.sample_dirs(torch.zeros(L.HDR_WORDS, dtype=torch.float64), k, W, H, torch.zeros(nf, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="1..8"):
        torch.ops.rt.sample_dirs(blob, 9, W, H, pix)
    with pytest.raises(RuntimeError, match="pixels"):
        torch.ops.rt.sample_dirs(blob, k, W, H, torch.empty(nf, dtype=torch.int64, device="meta"))
    with pytest.raises(RuntimeError, match="header"):
        torch.ops.rt.sample_dirs(blob[:10], k, W, H, pix)

    s = torch.empty(3, nf * k * k, dtype=torch.float64, device="meta")
    outs = {L.OUT_F32_SOA: torch.empty(3, n, dtype=torch.float32, device="meta"),
            L.OUT_F64_SOA: torch.empty(3, n, dtype=torch.float64, device="meta"),
            L.OUT_U8_HWC: torch.empty(H, W, 3, dtype=torch.uint8, device="meta")}
    for kind, out in outs.items():
        assert torch.ops.rt.resolve_scatter(s, k, pix, W, H, out, kind) is None
        for other, wrong in outs.items():
            if other != kind:
                with pytest.raises(RuntimeError, match="out must be"):
                    torch.ops.rt.resolve_scatter(s, k, pix, W, H, wrong, kind)
    with pytest.raises(RuntimeError, match="samples"):
        torch.ops.rt.resolve_scatter(s[:, :-1], k, pix, W, H, outs[1], 1)
    with pytest.raises(RuntimeError, match="out must be"):
        torch.ops.rt.resolve_scatter(s, k, pix, W, H, torch.empty(3, n - 1, dtype=torch.float64, device="meta"), 1)
    with pytest.raises(RuntimeError, match="out_kind"):
        torch.ops.rt.resolve_scatter(s, k, pix, W, H, outs[1], 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.resolve_scatter(torch.zeros(3, nf * k * k, dtype=torch.float64), k,
                                     torch.zeros(nf, dtype=torch.int32), W, H, torch.zeros(3, n, dtype=torch.float64), 1)


# ---------------------------------------------------------------- the NumPy restatement, by hand
def _flat(color=0.5, ident=0, hits=1, lit=1, w=3, h=3):
    n = w * h
    return (np.full((3, n), color, dtype=np.float64), np.full(n, ident, dtype=np.int32),
            np.full(n, hits, dtype=np.int32), np.full(n, lit, dtype=np.uint8))


def test_mask_ref_flat_frames_and_the_geometric_test():
    for c in (0.0, 0.0625, None):
        assert not A.mask_ref(*_flat(), 3, 3, c).any()
    # another id in the centre: all nine pixels (the criterion is symmetric, 8 neighbours)
    col, ident, hits, lit = _flat()
    ident[4] = 2
    assert A.mask_ref(col, ident, hits, lit, 3, 3, None).all()
    # in a corner: the corner and its three neighbours
    col, ident, hits, lit = _flat()
    ident[0] = -1
    assert A.mask_ref(col, ident, hits, lit, 3, 3, None).tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0]
    # a shadow edge (lit) in the last column: the two right columns
    col, ident, hits, lit = _flat()
    lit[[2, 5, 8]] = 0
    assert A.mask_ref(col, ident, hits, lit, 3, 3, None).tolist() == [0, 1, 1] * 3
    # a tie flags its own pixel only
    col, ident, hits, lit = _flat()
    hits[4] = 2
    assert A.mask_ref(col, ident, hits, lit, 3, 3, None).tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert A.mask_ref(*_flat(hits=0), 3, 3, 0.0).sum() == 0  # misses everywhere: no edge
    # a 1 x 1 frame flags only a tie
    assert A.mask_ref(*_flat(w=1, h=1), 1, 1, 0.0).tolist() == [0]
    assert A.mask_ref(*_flat(w=1, h=1, hits=3), 1, 1, None).tolist() == [1]


def test_mask_ref_colour_test_is_strict_and_in_float64():
    # 1 x N rows: no neighbour wraps round the end of a row
    col, ident, hits, lit = _flat(w=5, h=1)
    col[1] = [0.25, 0.25, 0.25 + 0.0625, 0.25 + 0.0625, 0.25 + 0.0625 + 2.0**-40]  # one channel is enough
    assert A.mask_ref(col, ident, hits, lit, 5, 1, 0.0625).tolist() == [0, 0, 0, 0, 0]  # |a-b| == contrast: not flagged
    col[1, 3] = np.nextafter(0.25 + 0.0625, 1.0)
    assert A.mask_ref(col, ident, hits, lit, 5, 1, 0.0625).tolist() == [0, 0, 0, 0, 0]  # its neighbours are an ulp and 2^-40 away
    col[1, 2] = np.nextafter(0.25 + 0.0625, 1.0)
    assert A.mask_ref(col, ident, hits, lit, 5, 1, 0.0625).tolist() == [0, 1, 1, 0, 0]
    assert A.mask_ref(col, ident, hits, lit, 5, 1, None).tolist() == [0] * 5
    assert A.mask_ref(col, ident, hits, lit, 5, 1, 0.0).tolist() == [0, 1, 1, 1, 1]  # any difference
    # as a 5 x 1 column the same values flag the same pixels
    assert A.mask_ref(col, ident, hits, lit, 1, 5, 0.0625).tolist() == [0, 1, 1, 0, 0]
    # a row's last pixel and the next row's first are no neighbours, the diagonal ones are
    col, ident, hits, lit = _flat(color=0.0, w=3, h=3)
    col[:, 2] = 1.0
    assert A.mask_ref(col, ident, hits, lit, 3, 3, 0.5).tolist() == [0, 1, 1, 0, 1, 1, 0, 0, 0]


def test_mask_ref_compares_clipped_colours_and_sends_nan_to_0():
    col, ident, hits, lit = _flat(color=1.0, w=4, h=1)
    col[0] = [1.0, 190.3, 7.0, 1.0]  # all clip to 1: no edge
    assert A.mask_ref(col, ident, hits, lit, 4, 1, 0.0).tolist() == [0, 0, 0, 0]
    col[0] = [0.0, -3.0, np.nan, 0.0]  # all 0 after the clip (NaN -> 0)
    col[1:] = 0.0
    assert A.mask_ref(col, ident, hits, lit, 4, 1, 0.0).tolist() == [0, 0, 0, 0]
    col[0] = [0.0, 0.0, np.nan, 190.3]  # NaN is 0, 190.3 is 1
    assert A.mask_ref(col, ident, hits, lit, 4, 1, 0.99).tolist() == [0, 0, 1, 1]
    assert np.array_equal(A.clip01([np.nan, -1.0, 0.5, 190.3, -0.0]), [0.0, 0.0, 0.5, 1.0, 0.0])


def test_sample_order_and_scatter_ref():
    # pixel (r, c) = (1, 2) of a 3-wide frame, k = 2: sample pixels (2, 4) (2, 5) (3, 4) (3, 5)
    rows, cols = A.sample_pixels([5, 0], 2, 3)
    assert rows.tolist() == [2, 2, 3, 3, 0, 0, 1, 1] and cols.tolist() == [4, 5, 4, 5, 0, 1, 0, 1]
    frame = np.arange(3 * 4 * 6, dtype=np.float64).reshape(3, 24) / 100.0
    got = A.gather_samples(frame, [5], 2, 3)
    assert np.array_equal(got, frame[:, [2 * 6 + 4, 2 * 6 + 5, 3 * 6 + 4, 3 * 6 + 5]])
    vals = np.array([0.1, 0.2, 0.3, 0.7, 0.6, 0.9, 0.15, 0.35, 0.05])
    acc = 0.0
    for v in vals:
        acc = acc + v
    s = np.stack([np.concatenate([vals, [190.3, -4.0] + [0.5] * 7]), np.zeros(18), np.ones(18)])
    out = A.scatter_ref(s, 3, 2)
    assert out.shape == (3, 2) and out[0, 0] == acc / 9.0 and out[0, 1] == (((0.0 + 1.0) + 0.0) + 3.5) / 9.0
    assert out[1].tolist() == [0.0, 0.0] and out[2].tolist() == [1.0, 1.0]
    assert A.scatter_ref(np.zeros((3, 0)), 4, 0).shape == (3, 0)
    assert A.pixel_list([0, 1, 1, 0, 1]).tolist() == [1, 2, 4] and A.pixel_list([0, 1]).dtype == np.int32
    # adaptive_ref: flagged pixels from the sample frame, the others their clipped base sample
    base = np.array([[1.5, 0.25], [-1.0, 0.5], [0.75, 190.3]])
    big = np.full((3, 2 * 4), 0.5)  # W = 2, H = 1, k = 2
    out = A.adaptive_ref(base, big, [0, 1], 2, 2, 1)
    assert out.tolist() == [[1.0, 0.5], [0.0, 0.5], [0.75, 0.5]]
