"""Supersampled anti-aliasing (HipRenderer(samples=k), rtx_resolve_samples): what needs no GPU.

The C ABI entry point and its host-side argument checks, the rt::resolve_samples op (schema, Meta
shapes, TORCH_CHECKs), the planning helpers (sample tiling, derived scene key, the 2^31 guard) and
the NumPy reference of the resolve itself.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from python_ray_tracer_amd import scenes, tiling
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from python_ray_tracer_amd.infrastructure.hip import scene_pack
from tests.ssaa_ref import resolve_ref, to_u8

REPO = Path(__file__).resolve().parent.parent


def test_header_declares_and_library_exports_resolve():
    text = (REPO / "include" / "rtx_hip.h").read_text()
    assert re.search(r"int rtx_resolve_samples\(const double\* samples, int k, int width, int n_rows, int n_frames,\s*"
                     r"void\* out, int out_kind, void\* stream\);", text)
    assert int(re.search(r"#define\s+RTX_ABI_VERSION\s+(\d+)", text).group(1)) == L.ABI_VERSION >= 2
    assert "rtx_resolve_samples" in L.EXPORTS and "rtx_resolve_samples" in L._SIGS
    lib = L.load()
    assert hasattr(lib, "rtx_resolve_samples")


def test_resolve_argument_checks_need_no_gpu():
    """Every bad argument returns RTX_E_ARG (-1) with a message, before any HIP call."""
    lib = L.load()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused on the host

    def call(samples=p, k=2, width=8, rows=4, frames=1, out=p, kind=L.OUT_F64_SOA):
        lib.rtx_last_error()
        return lib.rtx_resolve_samples(samples, k, width, rows, frames, out, kind, None)

    assert call(samples=None) == -1 and b"null" in lib.rtx_last_error()
    assert call(out=None) == -1 and b"null" in lib.rtx_last_error()
    for k in (0, -1, 9, 64):
        assert call(k=k) == -1 and b"1..8" in lib.rtx_last_error(), k
    for kw in ({"width": 0}, {"width": -3}, {"rows": 0}, {"rows": -1}, {"frames": 0}, {"frames": -2}):
        assert call(**kw) == -1 and b"geometry" in lib.rtx_last_error(), kw
    for kind in (-1, 3, 17):
        assert call(kind=kind) == -1 and b"out_kind" in lib.rtx_last_error(), kind
    # k*k*width*n_rows*n_frames >= 2^31: exactly 2^31, just above, and products that overflow 64 bits
    for k, w, r, f in ((2, 1 << 15, 1 << 14, 1), (1, 1 << 16, 1 << 15, 1), (8, 1 << 13, 1 << 12, 1),
                       (4, 1 << 12, 1 << 12, 8), (8, 2**31 - 1, 2**31 - 1, 2**31 - 1), (3, 15451, 15451, 1)):
        assert k * k * w * r * f >= 2**31
        assert call(k=k, width=w, rows=r, frames=f) == -1 and b"2^31" in lib.rtx_last_error(), (k, w, r, f)


def test_resolve_op_schema_meta_and_host_checks():
    import python_ray_tracer_amd.ops as ops

    assert "resolve_samples" in ops.OPS
    assert str(torch.ops.rt.resolve_samples.default._schema) == \
        "rt::resolve_samples(Tensor samples, int k, int width, int rows, int out_kind) -> Tensor"
    k, W, rows = 3, 20, 5
    ns = k * rows * k * W
    want = {L.OUT_F32_SOA: ((3, rows * W), torch.float32), L.OUT_F64_SOA: ((3, rows * W), torch.float64),
            L.OUT_U8_HWC: ((rows, W, 3), torch.uint8)}
    for kind, (shape, dtype) in want.items():
        one = torch.ops.rt.resolve_samples(torch.empty(3, ns, dtype=torch.float64, device="meta"), k, W, rows, kind)
        assert tuple(one.shape) == shape and one.dtype == dtype and one.device.type == "meta"
        many = torch.ops.rt.resolve_samples(torch.empty(4, 3, ns, dtype=torch.float64, device="meta"), k, W, rows, kind)
        assert tuple(many.shape) == (4,) + shape and many.dtype == dtype
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.rt.resolve_samples(torch.zeros(3, ns, dtype=torch.float64), k, W, rows, L.OUT_F64_SOA)
    # a short samples tensor and a float32 one: refused, on the host and on the Meta device alike
    for dev in ("cpu", "meta"):
        with pytest.raises(RuntimeError):
            torch.ops.rt.resolve_samples(torch.zeros(3, ns - 1, dtype=torch.float64, device=dev), k, W, rows, 1)
        with pytest.raises(RuntimeError):
            torch.ops.rt.resolve_samples(torch.zeros(3, ns, dtype=torch.float32, device=dev), k, W, rows, 1)
    meta = torch.empty(3, ns, dtype=torch.float64, device="meta")
    with pytest.raises(RuntimeError, match="samples per plane"):
        torch.ops.rt.resolve_samples(torch.empty(3, ns + 1, dtype=torch.float64, device="meta"), k, W, rows, 1)
    with pytest.raises(RuntimeError, match="Double"):
        torch.ops.rt.resolve_samples(torch.empty(3, ns, dtype=torch.float32, device="meta"), k, W, rows, 1)
    with pytest.raises(RuntimeError, match="1..8"):
        torch.ops.rt.resolve_samples(meta, 9, W, rows, 1)
    with pytest.raises(RuntimeError, match="out_kind"):
        torch.ops.rt.resolve_samples(meta, k, W, rows, 3)
    with pytest.raises(RuntimeError):
        torch.ops.rt.resolve_samples(torch.empty(2, ns, dtype=torch.float64, device="meta"), k, W, rows, 1)


@pytest.mark.parametrize("k", [2, 3])
def test_sample_tiling_covers_each_row_with_its_k_sample_rows(k):
    for H in (1, 17, 22):
        for rb in (1, 4):
            shares = [(P, p, 1) for P in range(1, 6) for p in range(P)]
            shares += [(P, p, 2) for P in range(2, 6) for p in range(P - 1)]
            for P, p, run in shares:
                rows = tiling.tile_rows(H, rb, P, p, run)
                assert tiling.n_sample_rows(H, rb, P, p, run, k) == k * tiling.n_local_rows(H, rb, P, p, run)
                got = tiling.sample_tile_rows(H, rb, P, p, run, k)
                want = (k * rows[:, None] + np.arange(k)[None, :]).reshape(-1)  # local order: k*lr + sy
                assert np.array_equal(got, want), (H, rb, P, p, run)
    assert tiling.sample_tiling(22, 4, k) == (22 * k, 4 * k)


def test_sample_key_changes_only_the_camera_size():
    scene = scenes.build_scene(scenes.readme_spec(50, 22))
    key = scene_pack.scene_key(scene)
    for k in (1, 2, 3, 8):
        static, (pos, W, H) = scene_pack.sample_key(key, k)
        assert static is key[0] and pos == key[1][0] and (W, H) == (50 * k, 22 * k)
    # it is the key of the same scene with that camera: what the renderer's launch path packs
    big = scenes.build_scene({**scenes.readme_spec(50, 22), "camera": {"position": [0, 0.2, -2], "width": 150,
                                                                     "height": 66}})
    assert scenes.readme_spec(50, 22)["camera"]["position"] == [0, 0.2, -2]
    assert scene_pack.sample_key(key, 3) == scene_pack.scene_key(big)


def test_sample_count_guard_and_samples_argument():
    assert tiling.check_sample_count(2, 1920, 1080) == 4 * 1920 * 1080
    assert tiling.check_sample_count(8, 4096, 2048, 3) == 64 * 4096 * 2048 * 3 < 2**31
    with pytest.raises(ValueError, match="2\\^31"):
        tiling.check_sample_count(2, 1 << 15, 1 << 14)  # exactly 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        tiling.check_sample_count(8, 7680, 4320, 2)
    for k in (1, 2, 8, np.int64(3)):
        assert tiling.check_samples(k) == int(k)
    from python_ray_tracer_amd.infrastructure.hip import HipRenderer

    for bad in (0, 9, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="samples"):
            tiling.check_samples(bad)
        with pytest.raises(ValueError, match="samples"):  # refused before the library or a GPU is touched
            HipRenderer(3, samples=bad)


def test_numpy_reference_of_the_resolve():
    """The helper the GPU tests compare against: order of the adds, clipping per sample, one division."""
    s = np.zeros((3, 4 * 6), dtype=np.float64)  # k = 2, W = 3, rows = 2
    s[0, [0, 1, 6, 7]] = [190.3, 0.25, -4.0, 0.5]  # pixel (0, 0) of channel 0: clipped to 1, .25, 0, .5
    out = resolve_ref(s, 2, 3, 2)
    assert out.shape == (3, 6) and out[0, 0] == (((0.0 + 1.0) + 0.25) + 0.0 + 0.5) / 4.0 and not out[1:].any()
    vals = np.array([0.1, 0.2, 0.3, 0.7, 0.6, 0.9, 0.15, 0.35, 0.05])
    acc = 0.0
    for v in vals:
        acc = acc + v
    assert resolve_ref(np.tile(vals, (3, 1)), 3, 1, 1)[0, 0] == acc / 9.0
    assert np.array_equal(to_u8(np.full((3, 2), 1.0), 2, 1), np.full((1, 2, 3), 255, dtype=np.uint8))
    assert resolve_ref(np.zeros((4, 3, 24)), 2, 3, 2).shape == (4, 3, 6)
