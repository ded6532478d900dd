"""Supersampled anti-aliasing on the GPU: HipRenderer(samples=k) and rtx_resolve_samples.

The contract (include/rtx_hip.h): a pixel is the float64 sum of its k x k samples, each
clipped to [0, 1], rows top to bottom and left to right, divided once by k*k; the samples are the
pixels of the same scene rendered from the same camera position at (k W, k H). So the resolve alone
is bit-exact against the NumPy reference (tests/ssaa_ref.py), and a supersampled render is the
reference applied to the oracle's frame at (k W, k H), within the project's 1e-12 bar: an average of
clipped samples cannot be further off than the worst sample. uint8 output must be identical.
"""

import socket

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes, tiling
from tests.ssaa_ref import resolve_ref, spec_at, to_f32, to_u8

pytestmark = pytest.mark.gpu

ATOL = 1e-12
W, H = 50, 22  # no multiple of a wave or block tile


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


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
    s[pick == 5] = rng.uniform(0.0, 1.0, size=shape)[pick == 5]
    return s


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_resolve_alone_is_bit_exact(hip, k):
    import python_ray_tracer_amd.ops  # noqa: F401

    L = hip._lib
    rng = np.random.default_rng(100 + k)
    for w, rows in ((1, 1), (50, 22), (67, 5), (257, 3)):
        for F in (1, 3):
            s = _samples(rng, (F, 3, k * rows * k * w))
            want = resolve_ref(s, k, w, rows)
            assert want.min() >= 0.0 and want.max() <= 1.0
            dev = torch.from_numpy(s if F > 1 else s[0]).cuda()
            for kind, ref in ((L.OUT_F64_SOA, want), (L.OUT_F32_SOA, to_f32(want)), (L.OUT_U8_HWC, to_u8(want, w, rows))):
                got = torch.ops.rt.resolve_samples(dev, k, w, rows, kind).cpu().numpy()
                assert np.array_equal(got, ref if F > 1 else ref[0]), (k, w, rows, F, kind)


CASES = {
    "readme_B3": (lambda: scenes.readme_spec(W, H), 3),
    "main_unbounded": (lambda: scenes.main_spec(W, H), None),
    "rand16_B4": (lambda: scenes.random_spec(16, 0, W, H), 4),
    "rand64_B5": (lambda: scenes.random_spec(64, 0, W, H), 5),  # the persistent kernel
}
_ORACLE: dict = {}


def _oracle_resolved(name, k):
    """resolve_ref of the oracle's frame at (k W, k H): computed once per case, never modified."""
    if (name, k) not in _ORACLE:
        make, B = CASES[name]
        ref = resolve_ref(O.render(O.scene_from_spec(spec_at(make(), k)), B), k, W, H)
        ref.setflags(write=False)
        _ORACLE[name, k] = ref
    return _ORACLE[name, k]


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_parity_with_the_resolved_oracle(hip, name, k):
    make, B = CASES[name]
    want = _oracle_resolved(name, k)
    scene = scenes.build_scene(make())
    r = hip.HipRenderer(B, samples=k)
    got = r.render(scene).data
    assert got.shape == (3, W * H) and got.dtype == torch.float64
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"{name} k={k}: max|gpu - resolve_ref(oracle)| = {err:.3e}")
    assert err <= ATOL, (name, k, err)
    assert np.array_equal(r.render_tile(scene, out="u8").cpu().numpy(), to_u8(want, W, H)), (name, k)
    # the pipeline's save_image quantises the resolved colour: the same bytes
    assert torch.equal(r.quantize(r.render(scene), scene.camera), r.render_tile(scene, out="u8"))
    r32 = hip.HipRenderer(B, samples=k, color_dtype=torch.float32)
    assert torch.equal(r32.render(scene).data, got.to(torch.float32)), (name, k)


def test_samples_1_is_the_plain_renderer(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    plain, one = hip.HipRenderer(3), hip.HipRenderer(3, samples=1)
    assert torch.equal(one.render(scene).data, plain.render(scene).data)
    assert torch.equal(one.render_tile(scene, out="u8"), plain.render_tile(scene, out="u8"))
    assert torch.equal(one.render_batch([scene, scene]), plain.render_batch([scene, scene]))
    assert one._sample_buf is None and one.samples == 1
    assert float(plain.render(scene).data.max()) > 1.0  # samples=1 colour stays unclipped ...
    two = hip.HipRenderer(3, samples=2)
    col = two.render(scene).data
    assert 0.0 <= float(col.min()) and float(col.max()) <= 1.0  # ... samples >= 2 colour is clipped
    assert two._sample_buf is not None and two._sample_buf.numel() >= 3 * 4 * W * H


def test_deferred_rays_land_in_the_sample_frame(hip, golden_meta):
    """Ties are deferred to the general kernel, which writes them where the fast kernel would have:
    into the sample frame, before the resolve reads it."""
    spec = golden_meta["cases"]["ties_64x36_B2"]["spec"]
    assert (spec["camera"]["width"], spec["camera"]["height"]) == (64, 36)
    st = O.TraceStats()
    frame = O.render(O.scene_from_spec(spec_at(spec, 2)), 2, stats=st)
    assert st.ties > 1000
    want = resolve_ref(frame, 2, 64, 36)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(2, samples=2, collect_stats=True)
    got = r.render(scene).data.cpu().numpy()
    assert np.abs(got - want).max() <= ATOL
    assert np.array_equal(r.render_tile(scene, out="u8").cpu().numpy(), to_u8(want, 64, 36))
    r.reset_stats()
    r.render(scene)
    s = r.stats()
    assert s["deferred"] > 0 and s["pixels"] == 4 * 64 * 36
    assert s["rays"] == st.rays and s["hits"] == st.hits


def test_uncapped_deep_chains_land_in_the_sample_frame(hip):
    """Uncapped, chains past the fast kernel's levels (deferred at level 30, continued, finished by
    the general kernel): rays inside a negative-radius mirror sphere lit from its centre reflect
    until they meet the small sphere or its shadow (a reflection is traced only from a lit hit)."""
    shader = {"reflection_gain": 1, "specular_gain": 1.0, "specular_roughness": 0.5, "iridescence_gain": 0.05,
              "diffuse_gain": 0.5}
    spec = scenes.readme_spec(24, 16)
    spec["spheres"] = [
        {"center": [0, 0.2, 0], "radius": -5.0, "shader": {**shader, "texture": {"kind": "const", "color": [0.9, 0.7, 0.4]}}},
        {"center": [1.0, 0.5, 1.5], "radius": 1.06, "shader": {**shader, "texture": {"kind": "const", "color": [0.4, 0.7, 0.9]}}}]
    spec["lights"][0]["position"] = [0, 0.2, 0]
    st = O.TraceStats()
    frame = O.render(O.scene_from_spec(spec_at(spec, 2)), None, stats=st)
    assert 61 < len(st.rays) <= 333 and st.rays[31] > 0 and st.rays[61] > 0  # chains pass levels 30 and 60, and end
    want = resolve_ref(frame, 2, 24, 16)
    scene = scenes.build_scene(spec)
    got = hip.HipRenderer(None, samples=2).render(scene).data.cpu().numpy()
    assert np.abs(got - want).max() <= ATOL
    rs = hip.HipRenderer(None, samples=2, collect_stats=True)
    assert np.array_equal(rs.render_tile(scene, out="u8").cpu().numpy(), to_u8(want, 24, 16))
    s = rs.stats()
    n = min(len(st.rays), hip._lib.S_LEVELS)
    assert s["pixels"] == 4 * 24 * 16 and s["deferred"] > 0
    assert s["rays"][:n] == st.rays[:n] and s["hits"][:n] == st.hits[:n]


def test_row_tiles_equal_the_rows_of_the_whole_frame(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    rb = 4
    for dtype in (torch.float64, torch.float32):
        r = hip.HipRenderer(3, samples=2, color_dtype=dtype)
        full = r.render(scene).data
        full_u8 = r.render_tile(scene, out="u8")
        layouts = [(3, [(p, 1) for p in range(3)], 1, 1)]  # a 3-way interleave
        n_parts, shares = tiling.runs(3, 1, 2)  # and runs (root_run, run) = (1, 2) over 3 ranks
        layouts.append((n_parts, shares, 1, 2))
        for P, tiles, root_run, run in layouts:
            for out, ref in ((None, full), ("u8", full_u8)):
                n = tiling.part_len(H, W, rb, len(tiles), ref.element_size(), out, root_run, run)
                buf = torch.full((len(tiles), n), 7, dtype=ref.dtype, device=ref.device)
                for i, (first, k_run) in enumerate(tiles):
                    rows = torch.as_tensor(tiling.tile_rows(H, rb, P, first, k_run), device=ref.device)
                    tile = r.render_tile(scene, rb, P, first, out=out, part_run=k_run)
                    want = ref[rows] if out == "u8" else ref.view(3, H, W)[:, rows].reshape(3, -1)
                    assert torch.equal(tile, want), (P, first, k_run, out)
                    shp = tiling.tile_shape(H, W, rb, P, first, out, k_run)
                    assert tuple(tile.shape) == shp
                    view = buf[i, :int(np.prod(shp))].view(shp)
                    assert r.render_tile(scene, rb, P, first, out=out, into=view, part_run=k_run) is view
                    assert torch.equal(view, tile)
                assert torch.equal(r.assemble_rows(buf, W, H, rb, out, root_run, run), ref), (P, out)
    with pytest.raises(ValueError, match="into"):
        r.render_tile(scene, rb, 3, 0, into=torch.empty(5, device="cuda"))
    with pytest.raises(ValueError, match="blob"):
        r.render_tile(scene, blob=torch.zeros(200, dtype=torch.float64, device="cuda"), n_spheres=3)


def test_batch_equals_single_frames(hip):
    base = scenes.random_spec(16, 0, 40, 18)
    frames = [scenes.build_scene(scenes.with_camera(base, scenes.orbit_position(f, 8))) for f in range(3)]
    r = hip.HipRenderer(3, samples=2)
    batch = r.render_batch(frames)
    u8 = r.render_batch(frames, out="u8")
    assert batch.shape == (3, 3, 40 * 18) and u8.shape == (3, 18, 40, 3)
    for f, sc in enumerate(frames):
        assert torch.equal(batch[f], r.render(sc).data), f
        assert torch.equal(u8[f], r.render_tile(sc, out="u8")), f


def test_pipeline_writes_the_resolved_png_and_refusals(hip, tmp_path):
    from PIL import Image

    from python_ray_tracer_amd.application import render_image_pipeline

    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(3, samples=2)
    render_image_pipeline(scene, tmp_path / "aa.png", r)
    png = np.asarray(Image.open(tmp_path / "aa.png").convert("RGB"))
    assert png.shape == (H, W, 3)
    assert np.array_equal(png, to_u8(_oracle_resolved("readme_B3", 2), W, H))
    # supersampling needs the camera: materialised or foreign rays and shade_hits are refused
    rays = r.get_ray_directions(scene.camera)
    assert rays.data.shape == (3, W * H)  # materialises the W x H rays
    with pytest.raises(ValueError, match="samples=2"):
        r.raytrace_scene(scene.camera.position, rays, scene)
    with pytest.raises(ValueError, match="samples=2"):
        r.shade_hits(scene.shapes[0], scene, scene.camera.position, hip.HipVector3D(rays.x, rays.y, rays.z),
                     torch.ones(W * H, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="samples=2"):
        r.submit_tiles(None, 0, scene, 4, 1, 0, None)


def test_one_rank_group_gathers_resolved_tiles(hip):
    """TileGather with a supersampling renderer: native=None takes render_tile(into=) and the gather
    (tiles are resolved before they travel), native=True is refused."""
    import torch.distributed as dist

    from python_ray_tracer_amd.application import render_frame_distributed
    from python_ray_tracer_amd.distributed import TileGather

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        scene = scenes.build_scene(scenes.readme_spec(W, H))
        r = hip.HipRenderer(3, samples=2, device=dev)
        with pytest.raises(ValueError, match="native"):
            TileGather(r, W, H, row_block=4, native=True)
        assert TileGather(r, W, H, row_block=4).plan is None
        assert TileGather(hip.HipRenderer(3, device=dev), W, H, row_block=4).plan is not None
        assert torch.equal(render_frame_distributed(scene, r, row_block=4), r.render(scene).data)
        assert torch.equal(render_frame_distributed(scene, r, row_block=4, gather="u8"), r.render_tile(scene, out="u8"))
    finally:
        dist.destroy_process_group()
