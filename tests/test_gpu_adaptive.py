"""Adaptive anti-aliasing on the GPU: HipRenderer(samples=k, adaptive=True) and its three kernels.

The contract (include/rtx_hip.h) decides every value: the mask is integer compares and
strict float64 compares of clipped colours, a sample direction is camera_dir of a pixel of the sample
frame, a flagged pixel is the resolve of its samples. So each kernel alone is bit-exact against its
NumPy restatement (tests/adaptive_ref.py), and a whole render is the restatement applied to the
oracle's frames within the project's 1e-12 bar (an average of clipped samples is no further off than
its worst sample; an unflagged pixel is one clipped sample).
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from python_ray_tracer_amd.infrastructure.hip import scene_pack
from tests import adaptive_ref as A
from tests import aov_ref
from tests.ssaa_ref import spec_at, to_f32, to_u8

pytestmark = pytest.mark.gpu

ATOL = 1e-12
W, H = 50, 22  # no multiple of a wave or block tile
SHAPES = ((1, 1), (2, 1), (1, 3), (50, 22), (67, 5), (257, 3))  # (width, height)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import python_ray_tracer_amd.ops  # noqa: F401
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


# ---------------------------------------------------------------- each kernel alone, bit for bit
def _frame(rng, w, h, contrast):
    """Random passes and colours of a w x h frame. Every pass is constant over runs of columns (the
    same in every row), so pixels without an edge exist; sprinkled over them, rare ties and colours
    below 0, above 1, exactly 0 and 1 and NaN, and pairs of neighbours exactly ``contrast`` apart."""
    n = w * h

    def runs(length, draw):
        return np.repeat(draw(w // length + 1), length, axis=-1)[..., :w]

    ident = np.tile(runs(7, lambda m: rng.integers(-1, 3, size=m)), h).astype(np.int32)
    lit = np.tile(runs(11, lambda m: rng.integers(0, 2, size=m)), h).astype(np.uint8)
    col = np.tile(runs(5, lambda m: rng.integers(0, 5, size=(3, m)) / 4.0), (1, h))  # 0, .25, .5, .75, 1
    hits = np.where(rng.random(n) < 0.01, 2, 1).astype(np.int32)
    special = np.array([-0.75, 190.3, np.nan, 0.0, 1.0])
    odd = rng.random((3, n)) < 0.005
    odd[:, 0] |= n > 1  # (at least one, in the first pixel)
    col[odd] = special[rng.integers(0, special.size, size=int(odd.sum()))]
    step = 0.0625 if not np.isfinite(contrast) or contrast == 0.0 else contrast
    for i in rng.integers(0, n, size=max(1, n // 16)):  # pairs exactly one step apart, beside and below
        for j in (i + 1, i + w):
            if j < n:
                col[:, j] = col[:, i]
                col[1, i], col[1, j] = 0.25, 0.25 + step
    return col, ident, hits, lit


@pytest.mark.parametrize("contrast", [0.0, 0.0625, float("inf")])
def test_edge_mask_alone_is_bit_exact(hip, contrast):
    rng = np.random.default_rng(7)
    for w, h in SHAPES:
        col, ident, hits, lit = _frame(rng, w, h, contrast)
        want = A.mask_ref(col, ident, hits, lit, w, h, None if np.isinf(contrast) else contrast)
        got = torch.ops.rt.edge_mask(torch.from_numpy(col).cuda(), torch.from_numpy(ident).cuda(),
                                     torch.from_numpy(hits).cuda(), torch.from_numpy(lit).cuda(), w, h, contrast)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (w * h,)
        assert np.array_equal(got.cpu().numpy(), want), (w, h, contrast, int((got.cpu().numpy() != want).sum()))
        if w * h > 100:  # both classes of pixel, so neither branch can hide
            assert 0 < int(want.sum()) < w * h, (w, h, contrast, int(want.sum()))


def _samples(rng, shape):
    """Random float64 samples mixed with negatives, values above 1, exact 0.0 and 1.0, 190.3 and
    denormals."""
    s = rng.uniform(-0.5, 1.5, size=shape)
    pick = rng.integers(0, 12, size=shape)
    s[pick == 0] = 0.0
    s[pick == 1] = 1.0
    s[pick == 2] = 190.3
    s[pick == 3] = 5e-324
    s[pick == 4] = 2.2250738585072014e-308 / 4
    return s


def _camera_blob(hip, w, h):
    """The packed scene of the README spheres with a w x h camera, on the device."""
    scene = scenes.build_scene(scenes.readme_spec(w, h))
    blob = scene_pack.pack_key(*scene_pack.scene_key(scene))
    return scene, torch.from_numpy(blob).cuda()


@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_sample_dirs_alone_is_bit_exact(hip, k):
    L = hip._lib
    lib = L.load()
    rng = np.random.default_rng(20 + k)
    for w, h in SHAPES:
        n = w * h
        scene, sblob = _camera_blob(hip, k * w, k * h)
        # a list with pixel 0 and pixel n-1 (the endpoint fix of the last sample column and row)
        mid = rng.choice(np.arange(1, n - 1), size=min(n - 2, 37), replace=False) if n > 2 else np.zeros(0, np.int64)
        pixels = np.unique(np.concatenate([[0, n - 1], mid])).astype(np.int32)
        got = torch.ops.rt.sample_dirs(sblob, k, w, h, torch.from_numpy(pixels).cuda())
        assert tuple(got.shape) == (3, pixels.size * k * k) and got.dtype == torch.float64
        rows, cols = A.sample_pixels(pixels, k, w)
        # rtx_ray_directions at (k w, k h), gathered at the same sample pixels
        full = torch.empty((3, k * w * k * h), dtype=torch.float64, device="cuda")
        L.check(lib.rtx_ray_directions(sblob.data_ptr(), k * w, k * h, 1, 1, 0, k * h, full.data_ptr(),
                                       L.stream_handle()), "rtx_ray_directions")
        idx = torch.from_numpy(rows * (k * w) + cols).cuda()
        assert torch.equal(got, full[:, idx]), (k, w, h)
        # and the oracle's get_ray_directions of those rows
        cam = tuple(float(c) for c in (scene.camera.position.x, scene.camera.position.y, scene.camera.position.z))
        urows, inv = np.unique(rows, return_inverse=True)
        ref = np.stack(O.ray_directions_rows(cam, k * w, k * h, urows)).reshape(3, urows.size, k * w)
        assert np.array_equal(got.cpu().numpy(), ref[:, inv, cols]), (k, w, h)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_resolve_scatter_alone_is_bit_exact(hip, k):
    L = hip._lib
    rng = np.random.default_rng(300 + k)
    kinds = ((L.OUT_F64_SOA, torch.float64, lambda c, w, h: c), (L.OUT_F32_SOA, torch.float32, lambda c, w, h: to_f32(c)),
             (L.OUT_U8_HWC, torch.uint8, lambda c, w, h: to_u8(c, w, h)))
    for w, h in SHAPES:
        n = w * h
        pixels = np.sort(rng.choice(n, size=max(1, n // 3), replace=False)).astype(np.int32)
        nf = pixels.size
        s = _samples(rng, (3, nf * k * k))
        want = A.scatter_ref(s, k, nf)
        assert want.shape == (3, nf) and want.min() >= 0.0 and want.max() <= 1.0
        dev_s, dev_p = torch.from_numpy(s).cuda(), torch.from_numpy(pixels).cuda()
        listed = np.zeros(n, dtype=bool)
        listed[pixels] = True
        for kind, dtype, conv in kinds:
            sentinel = 7 if dtype == torch.uint8 else -3.5
            shape = (h, w, 3) if dtype == torch.uint8 else (3, n)
            out = torch.full(shape, sentinel, dtype=dtype, device="cuda")
            assert torch.ops.rt.resolve_scatter(dev_s, k, dev_p, w, h, out, kind) is None
            got = out.cpu().numpy()
            full = np.zeros((3, n))
            full[:, pixels] = want
            ref = conv(full, w, h)
            if dtype == torch.uint8:
                got, ref = got.reshape(n, 3).T, ref.reshape(n, 3).T
            assert np.array_equal(got[:, listed], ref[:, listed]), (k, w, h, kind)
            assert (got[:, ~listed] == sentinel).all(), (k, w, h, kind)  # every unlisted pixel untouched
            # an empty list: OK, nothing written
            out.fill_(sentinel)
            torch.ops.rt.resolve_scatter(dev_s[:, :0], k, dev_p[:0], w, h, out, kind)
            assert bool((out == sentinel).all())


# ---------------------------------------------------------------- end to end, against the oracle
CASES = {
    "readme_B3": ("readme", lambda: scenes.readme_spec(W, H), 3),
    "main_unbounded": ("main", lambda: scenes.main_spec(W, H), None),
    "rand16_B4": ("rand16", lambda: scenes.random_spec(16, 0, W, H), 4),
    "rand64_B5": ("rand64", lambda: scenes.random_spec(64, 0, W, H), 5),  # the persistent kernel
    "ties_64x36_B2": ("ties", None, 2),  # tests/golden: 9.8% of the pixels are ties
}
RUNS = [(name, 2) for name in sorted(CASES)] + [("readme_B3", 3), ("readme_B3", 4)]
_CACHE: dict = {}


def _case(name, golden_meta):
    """(spec, bounce cap, oracle base frame, passes of aov_ref): computed once, read-only."""
    if name not in _CACHE:
        key, make, B = CASES[name]
        spec = golden_meta["cases"][name]["spec"] if make is None else make()
        base = O.render(O.scene_from_spec(spec), B)
        base.setflags(write=False)
        _CACHE[name] = (spec, B, base, aov_ref.frame(key, lambda: spec)[1])
    return _CACHE[name]


def _sample_frame(name, k, golden_meta):
    """The oracle's frame at (k W, k H): computed once per case and k, read-only."""
    if (name, k) not in _CACHE:
        spec, B, _, _ = _case(name, golden_meta)
        frame = O.render(O.scene_from_spec(spec_at(spec, k)), B)
        frame.setflags(write=False)
        _CACHE[name, k] = frame
    return _CACHE[name, k]


@pytest.mark.parametrize("contrast", [0.0625, None])
@pytest.mark.parametrize("name,k", RUNS)
def test_render_parity_with_the_oracle(hip, golden_meta, tmp_path, name, k, contrast):
    spec, B, base, a = _case(name, golden_meta)
    w, h = spec["camera"]["width"], spec["camera"]["height"]
    n = w * h
    m = A.mask_ref(base, a["id"], a["hits"], a["lit"], w, h, contrast)
    share = float(m.mean())
    print(f"{name} k={k} contrast={contrast}: flagged share {share:.3f}")
    assert 0.05 < share < 0.95, (name, contrast, share)
    if name.startswith("ties"):
        assert int((a["hits"] > 1).sum()) == 226
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(B, samples=k, adaptive=True, contrast=contrast, collect_stats=True)
    got_mask = r.edge_mask(scene)
    assert got_mask.dtype == torch.uint8 and tuple(got_mask.shape) == (n,)
    assert np.array_equal(got_mask.cpu().numpy(), m), (name, contrast, int((got_mask.cpu().numpy() != m).sum()))

    want = A.adaptive_ref(base, _sample_frame(name, k, golden_meta), m, k, w, h)
    r.reset_stats()
    got = r.render(scene).data
    flagged = int(m.sum())
    assert r.last_adaptive == {"flagged": flagged, "pixels": n}
    assert r.stats()["pixels"] == n + flagged * k * k
    assert got.shape == (3, n) and got.dtype == torch.float64
    g = got.cpu().numpy()
    err = float(np.abs(g - want).max())
    print(f"{name} k={k} contrast={contrast}: max|gpu - adaptive_ref(oracle)| = {err:.3e}")
    assert err <= ATOL, (name, k, contrast, err)
    assert g.min() >= 0.0 and g.max() <= 1.0

    r32 = hip.HipRenderer(B, samples=k, adaptive=True, contrast=contrast, color_dtype=torch.float32)
    assert torch.equal(r32.render(scene).data, got.to(torch.float32)), (name, k)

    # uint8: the quantised reference, except where the reference's 255*value is within 1e-9 of an integer
    v = 255.0 * want
    near = np.abs(v - np.rint(v)) < 1e-9
    near &= (want > 0.0) & (want < 1.0)  # (exact 0 and 1 quantise the same on both sides of any error)
    if near.any():
        print(f"{name} k={k}: {int(near.any(axis=0).sum())} pixels within 1e-9 of a uint8 step, not compared")
    keep = ~np.moveaxis(near.reshape(3, h, w), 0, -1)
    u8 = r.render_tile(scene, out="u8")
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (h, w, 3)
    assert np.array_equal(u8.cpu().numpy()[keep], to_u8(want, w, h)[keep]), (name, k)
    assert torch.equal(r.quantize(r.render(scene), scene.camera), u8)
    into = torch.full((h, w, 3), 9, dtype=torch.uint8, device="cuda")
    assert r.render_tile(scene, out="u8", into=into) is into and torch.equal(into, u8)
    if contrast is not None:  # the saved PNG of the pipeline: the same bytes
        from PIL import Image

        from python_ray_tracer_amd.application import render_image_pipeline

        render_image_pipeline(scene, tmp_path / "adaptive.png", r)
        png = np.asarray(Image.open(tmp_path / "adaptive.png").convert("RGB"))
        assert png.shape == (h, w, 3) and np.array_equal(png, u8.cpu().numpy())


@pytest.mark.parametrize("name,k", RUNS)
def test_contrast_0_flagged_pixels_equal_full_supersampling(hip, golden_meta, name, k):
    """Both renders are within 1e-12 of the oracle's resolve on a flagged pixel, so within 2e-12 of
    each other; an unflagged pixel (all 8 neighbours of one colour, shape and light) is its one sample."""
    spec, B, base, a = _case(name, golden_meta)
    w, h = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(B, samples=k, adaptive=True, contrast=0.0)
    m = r.edge_mask(scene).bool()
    assert np.array_equal(m.cpu().numpy(), A.mask_ref(base, a["id"], a["hits"], a["lit"], w, h, 0.0).astype(bool))
    assert 0.05 < float(m.float().mean()) <= 1.0
    got = r.render(scene).data
    full = hip.HipRenderer(B, samples=k).render(scene).data
    diff = float((got - full)[:, m].abs().max())
    print(f"{name} k={k}: max|adaptive - samples={k}| on flagged pixels = {diff:.3e}")
    assert diff <= 2e-12, (name, k, diff)


def test_adaptive_false_is_todays_renderer(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    for k in (1, 2, 3):
        plain = hip.HipRenderer(3, samples=k)
        off = hip.HipRenderer(3, samples=k, adaptive=False, contrast=None)
        assert torch.equal(off.render(scene).data, plain.render(scene).data)
        assert torch.equal(off.render_tile(scene, out="u8"), plain.render_tile(scene, out="u8"))
        assert torch.equal(off.render_tile(scene, 4, 3, 1), plain.render_tile(scene, 4, 3, 1))
        assert torch.equal(off.render_batch([scene, scene]), plain.render_batch([scene, scene]))
        assert off.adaptive is False and off._adaptive_bufs == {} and off.last_adaptive is None
        assert plain.adaptive is False and plain._adaptive_bufs == {}
        with pytest.raises(ValueError, match="adaptive"):
            off.edge_mask(scene)


def test_refusals_and_grow_only_buffers(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(3, samples=2, adaptive=True)
    with pytest.raises(ValueError, match="adaptive"):
        r.render_tile(scene, 4, 2, 0)
    with pytest.raises(ValueError, match="adaptive"):
        r.render_tile(scene, blob=torch.zeros(200, dtype=torch.float64, device="cuda"), n_spheres=3)
    with pytest.raises(ValueError, match="adaptive"):
        r.render_batch([scene])
    with pytest.raises(ValueError, match="adaptive"):
        r.submit_tiles(None, 0, scene, 4, 1, 0, None)
    with pytest.raises(ValueError, match="samples=2"):
        r.render_aovs(scene)
    rays = r.get_ray_directions(scene.camera)
    first = r.raytrace_scene(scene.camera.position, rays, scene).data  # the lazy pipeline: a camera render
    assert torch.equal(first, r.render(scene).data)
    assert rays.data.shape == (3, W * H)  # materialised: no pixel grid to refine
    with pytest.raises(ValueError, match="samples=2"):
        r.raytrace_scene(scene.camera.position, rays, scene)
    with pytest.raises(ValueError, match="into"):
        r.render_tile(scene, into=torch.empty(5, device="cuda"))
    ptrs = {k: v.data_ptr() for k, v in r._adaptive_bufs.items()}
    assert set(ptrs) == {"base", "id", "hits", "lit", "mask", "dirs", "samples"}
    small = scenes.build_scene(scenes.readme_spec(20, 10))
    r.render(small)
    r.render(scene)
    assert {k: v.data_ptr() for k, v in r._adaptive_bufs.items()} == ptrs  # renderer-owned, grow-only


def test_uncapped_render_still_raises_recursion_error(hip):
    spec = scenes.readme_spec(8, 8)
    spec["spheres"] = [{"center": [0, 0.2, -2], "radius": -5.0,
                        "shader": {"reflection_gain": 1, "specular_gain": 1.0, "specular_roughness": 0.5,
                                   "iridescence_gain": 0, "diffuse_gain": 0.5,
                                   "texture": {"kind": "const", "color": [1, 1, 1]}}}]
    spec["lights"][0]["position"] = [0, 0.2, -2]
    with pytest.raises(RecursionError):
        hip.HipRenderer(samples=2, adaptive=True).render(scenes.build_scene(spec))


def test_the_ops_compose_the_renderers_frame(hip):
    """The documented op pipeline: base render, passes, mask, list, sample
    directions, trace, clip-and-convert, scatter: the renderer's frame, bit for bit."""
    L = hip._lib
    k, B = 3, 3
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(B, samples=k, adaptive=True)
    blob, S = r.scene_blob(scene)
    _, blob_k = _camera_blob(hip, k * W, k * H)
    ops = torch.ops.rt
    ws = torch.zeros(ops.workspace_bytes(W * H, B), dtype=torch.uint8, device="cuda")
    base = ops.render_tile(blob, S, W, H, 1, 1, 0, B, L.OUT_F64_SOA, ws)
    ident, hits, lit = ops.primary_aovs(blob, S, W, H, 1, 1, 0, 1, L.AOV_ID | L.AOV_HITS | L.AOV_LIT)
    mask = ops.edge_mask(base, ident, hits, lit, W, H, 0.0625)
    assert torch.equal(mask, r.edge_mask(scene))
    pixels = torch.nonzero(mask).view(-1).to(torch.int32)
    dirs = ops.sample_dirs(blob_k, k, W, H, pixels)
    ws_s = torch.zeros(ops.workspace_bytes(dirs.shape[1], B), dtype=torch.uint8, device="cuda")
    samples = ops.trace(blob_k, S, blob_k[L.H_CAM:L.H_CAM + 3], dirs, B, L.OUT_F64_SOA, ws_s)
    for kind, want in ((L.OUT_F64_SOA, r.render(scene).data), (L.OUT_U8_HWC, r.render_tile(scene, out="u8"))):
        out = ops.resolve_samples(base, 1, W, H, kind)
        ops.resolve_scatter(samples, k, pixels, W, H, out, kind)
        assert torch.equal(out, want), kind
