"""GPU parity: the HIP path (C ABI via HipRenderer) against the reference fixtures and the CPU oracle.

Tolerances. Geometry, the hit / shadow / checker decisions and the bounce structure are float64 with
the reference's operation order and no contraction, so they match exactly; the only non-correctly-
rounded operations are sin (iridescence) and pow (x^5, x^2.5 in the specular), where NumPy's SIMD
versions and the device's differ by 1-2 ulp. Hence colour is compared at max-abs <= 1e-12 (float64
output; the largest unclipped values are ~1e2), uint8 output must be identical, and per-level ray
counts must equal the oracle's.
"""

import json

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from tests.conftest import GOLDEN, golden_png
from tests.specs import HUGE_LAYOUTS, huge_tail_spec
from tests.specs import fuzz_spec as _fuzz_spec
from tests.specs import textured_spec as _textured_spec

pytestmark = pytest.mark.gpu

ATOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H

    return H


def _render(H, spec, B, dtype=torch.float64, stats=False):
    r = H.HipRenderer(max_bounces=B, color_dtype=dtype, collect_stats=stats)
    scene = scenes.build_scene(spec)
    col = r.raytrace_scene(scene.camera.position, r.get_ray_directions(scene.camera), scene)
    return r, col.data.cpu().numpy()


def test_golden_cases(hip, golden_meta, golden_renders):
    for name, case in golden_meta["cases"].items():
        _, got = _render(hip, case["spec"], case["max_bounces"])
        ref = golden_renders[name]
        err = np.abs(got - ref).max()
        assert err <= ATOL, (name, err)
        W, H = case["spec"]["camera"]["width"], case["spec"]["camera"]["height"]
        assert np.array_equal(O.to_uint8(got, W, H), O.to_uint8(ref, W, H)), name


def test_render_png_byte_exact(hip, tmp_path):
    """main.py's scene with the reference's unbounded bounces -> the committed render.png."""
    r = hip.HipRenderer()  # max_bounces=None, like the reference
    scene = scenes.build_scene(scenes.main_spec(960, 540))
    from python_ray_tracer_amd.application import render_image_pipeline

    out = tmp_path / "render.png"
    render_image_pipeline(scene, out, r)
    from PIL import Image

    assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), golden_png("render_main_960x540.png"))


@pytest.mark.parametrize("tag", ["main", "readme"])
def test_1080p_B3_full_size(hip, golden_meta, tag):
    """BASELINE configs[1] size: 1920x1080, 3 bounces, against the oracle at full size and the
    reference's own uint8 output; kernel ray counters against the oracle's."""
    m = golden_meta[f"ref_1080p_B3_{tag}"]
    r, got = _render(hip, m["spec"], 3, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(m["spec"]), 3, stats=st)
    assert np.abs(got - want).max() <= ATOL
    assert np.array_equal(O.to_uint8(got, 1920, 1080), golden_png(f"ref_1080p_B3_{tag}.png"))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits
    assert s["pixels"] == 1920 * 1080 and s["deferred"] == 0
    # float32 output = float64 output rounded once
    _, got32 = _render(hip, m["spec"], 3, dtype=torch.float32)
    assert np.array_equal(got32, got.astype(np.float32))


# The colour drift the kernel's reassociations introduce ("Where the kernel departs from
# the reference's association": the forward fold and the fused shading sums) measured over every golden
# case and both 1080p goldens: the worst |GPU - reference| must stay at or below this ceiling, well
# under the 1e-12 parity bar, so that a regression towards the bar shows here first.
DRIFT_CEIL = 2e-13


def test_reassociation_drift_is_pinned(hip, golden_meta, golden_renders):
    worst = {}
    for name, case in golden_meta["cases"].items():
        _, got = _render(hip, case["spec"], case["max_bounces"])
        worst[name] = float(np.abs(got - golden_renders[name]).max())
    for tag in ("main", "readme"):
        spec = golden_meta[f"ref_1080p_B3_{tag}"]["spec"]
        _, got = _render(hip, spec, 3)
        worst[f"1080p_B3_{tag}"] = float(np.abs(got - O.render(O.scene_from_spec(spec), 3)).max())
    print("max |gpu - reference| per golden:", json.dumps(worst))
    assert max(worst.values()) <= DRIFT_CEIL, worst


def test_ties_take_the_general_kernel(hip, golden_meta, golden_renders):
    case = golden_meta["cases"]["ties_64x36_B2"]
    r, got = _render(hip, case["spec"], 2, stats=True)
    assert np.abs(got - golden_renders["ties_64x36_B2"]).max() <= ATOL
    s = r.stats()
    assert s["deferred"] > 100 and s["ties"] >= s["deferred"]
    # no cap: ties deferred by the first pass are forwarded through the continuation pass
    r, got = _render(hip, case["spec"], None, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(case["spec"]), None, stats=st)
    assert np.abs(got - want).max() <= ATOL
    assert r.stats()["rays"] == st.rays and r.stats()["hits"] == st.hits


@pytest.mark.parametrize("case", ["ties_64x36_B2", "main_160x90_B3", "rand16_128x72_B4"])
def test_general_launch_skipped_only_when_nothing_is_deferred(hip, golden_meta, golden_renders, case):
    """HipRenderer probes the deferred count of a capped render's first launch and skips the
    general kernel (RTX_F_NO_GENERAL) on later renders of the same scene only if it was 0; every
    render still equals the golden one (the tie scene keeps its general launch)."""
    c = golden_meta["cases"][case]
    r = hip.HipRenderer(max_bounces=c["max_bounces"])
    scene = scenes.build_scene(c["spec"])
    for _ in range(3):
        got = r.render_tile(scene).cpu().numpy()  # .cpu() synchronises: the probe has landed
        assert np.abs(got - golden_renders[case]).max() <= ATOL
    (state,) = r._defers.values()
    assert state is (case != "ties_64x36_B2")
    # the skip is per tile: another part of the same scene probes on its own
    r.render_tile(scene, 8, 2, 1)
    assert len(r._defers) == 2
    # another camera is another key
    spec2 = {**c["spec"], "camera": {**c["spec"]["camera"], "position": [0.05, 0.3, -2.0]}}
    r.render_tile(scenes.build_scene(spec2))
    assert len(r._defers) == 3


def test_uncapped_skips_continuation_and_general_only_when_nothing_is_deferred(hip):
    """The probe also serves uncapped renders (round 6): once the first render of a key has deferred
    nothing, later renders skip the continuation pass and the general kernel (RTX_F_NO_GENERAL); a
    scene whose chains all outlive the first pass's level-30 record keeps them. Every render of both
    equals the oracle's, three times over (the later ones with the flag decided)."""
    spec = scenes.random_spec(16, 3, 64, 36)  # no chain reaches level 30
    trap = scenes.readme_spec(12, 8)  # every chain passes level 30 (test_deep_chains_resume_...)
    trap["spheres"] = [{"center": [0, 0.2, -2], "radius": -5.0,
                        "shader": {"reflection_gain": 1, "specular_gain": 1.0, "specular_roughness": 0.5,
                                   "iridescence_gain": 0.05, "diffuse_gain": 0.5,
                                   "texture": {"kind": "const", "color": [0.9, 0.7, 0.4]}}}]
    trap["lights"][0]["position"] = [0, 0.2, -2]
    for sp, cap, skips in ((spec, None, True), (trap, 40, False)):
        want = O.render(O.scene_from_spec(sp), cap)
        r = hip.HipRenderer(max_bounces=cap, color_dtype=torch.float64)
        assert r.max_bounces is None or r.max_bounces > hip._lib.FAST_MAX_BOUNCES  # the uncapped pipeline
        scene = scenes.build_scene(sp)
        for _ in range(3):
            got = r.render_tile(scene).cpu().numpy()  # .cpu() synchronises: the probe has landed
            assert np.abs(got - want).max() <= ATOL, (cap, np.abs(got - want).max())
        (state,) = r._defers.values()
        assert state is skips, cap


@pytest.mark.parametrize("cap", [3, None])
def test_scene_above_the_lds_table(hip, cap):
    """Scenes of more spheres than the LDS table holds (kLdsMaxSpheres = 128) run the builds that read
    the sphere table from global memory. test_large_scene_without_lds_table renders through the
    counting (STATS) builds. Here the renderer's first render is a recording launch (it learns the
    dispatch order), so it runs the counting build too; the second, with the deferral probe landed
    and the order learnt, is the counter-free one a plain render runs: the persistent launch (camera
    frame) and, uncapped, its first pass, continuation pass and general kernel. Then the explicit-ray
    mode (HipCameraRays materialised), counter-free from its first launch. 150 spheres against the
    oracle; the counters of a counting render too."""
    spec = scenes.random_spec(150, 7, 56, 32)
    osc = O.scene_from_spec(spec)
    st = O.TraceStats()
    want = O.render(osc, cap, stats=st)
    r = hip.HipRenderer(max_bounces=cap, color_dtype=torch.float64)
    scene = scenes.build_scene(spec)
    for _ in range(2):  # (the first a recording launch; the second counter-free, the deferral probe landed)
        got = r.render_tile(scene).cpu().numpy()
        assert np.abs(got - want).max() <= ATOL, (cap, np.abs(got - want).max())
    dirs = r.get_ray_directions(scene.camera)
    assert dirs.data.shape[-1] == 56 * 32 or dirs.data.numel() == 3 * 56 * 32  # materialised: the explicit-ray mode
    rays = r.raytrace_scene(scene.camera.position, dirs, scene).data.cpu().numpy()
    assert np.abs(rays - want).max() <= ATOL
    rs = hip.HipRenderer(max_bounces=cap, collect_stats=True)
    rs.render(scene)
    s = rs.stats()
    n = min(len(st.rays), hip._lib.S_LEVELS)
    assert s["rays"][:n] == st.rays[:n] and s["hits"][:n] == st.hits[:n]


def test_camera_ex_flags_are_checked(hip):
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    r = hip.HipRenderer(max_bounces=2)
    scene = scenes.build_scene(scenes.random_spec(4, 0, 16, 8))
    blob, S = r.scene_blob(scene)
    out = torch.empty((3, 128), dtype=torch.float64, device="cuda")
    ws = r.workspace(128)
    rc = r._lib.rtx_render_camera_ex(blob.data_ptr(), S, 16, 8, 1, 1, 0, 8, 2, out.data_ptr(), L.OUT_F64_SOA,
                                     ws.data_ptr(), ws.numel(), None, L.stream_handle(), 4, None)
    assert rc != 0 and b"flags" in r._lib.rtx_last_error()
    # the deferred count lands in a device word: 0 for a tie-free scene
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    L.check(r._lib.rtx_render_camera_ex(blob.data_ptr(), S, 16, 8, 1, 1, 0, 8, 2, out.data_ptr(), L.OUT_F64_SOA,
                                        ws.data_ptr(), ws.numel(), None, L.stream_handle(), 0, cnt.data_ptr()),
            "rtx_render_camera_ex")
    assert int(cnt.item()) == 0


@pytest.mark.parametrize("B", [0, 1, 2, 4, 5, 6, 7, 8, 9, 12])
def test_every_bounce_cap(hip, B):
    spec = scenes.random_spec(16, 0, 128, 72)
    _, got = _render(hip, spec, B)
    want = O.render(O.scene_from_spec(spec), B)
    assert np.abs(got - want).max() <= ATOL, B


def test_c3_c4_scenes_reduced_size(hip):
    for spec, B in ((scenes.random_spec(16, 0, 480, 270), 4), (scenes.random_spec(64, 0, 320, 180), 5),
                    (scenes.with_camera(scenes.random_spec(16, 0, 320, 180), scenes.orbit_position(100)), 3)):
        r, got = _render(hip, spec, B, stats=True)
        st = O.TraceStats()
        want = O.render(O.scene_from_spec(spec), B, stats=st)
        assert np.abs(got - want).max() <= ATOL
        assert r.stats()["rays"] == st.rays


def test_row_tiles_reassemble(hip):
    from python_ray_tracer_amd import tiling

    spec = scenes.readme_spec(200, 117)
    scene = scenes.build_scene(spec)
    full_u8 = None
    for dtype in (torch.float64, torch.float32):
        r = hip.HipRenderer(max_bounces=3, color_dtype=dtype)
        full = r.render(scene).data
        full_u8 = r.quantize(r.render(scene), scene.camera)
        for P, rb in ((2, 8), (3, 5), (8, 8), (5, 1)):
            for out, ref, isz in ((None, full, full.element_size()), ("u8", full_u8, 1)):
                n = tiling.part_len(117, 200, rb, P, isz, out)
                # tiles rendered straight into the gather buffers (render_tile(into=)), then the
                # device un-permute (rtx_assemble_rows) and the host one (tiling.assemble)
                buf = torch.full((P, n), 7, dtype=ref.dtype, device=ref.device)
                for p in range(P):
                    shp = tiling.tile_shape(117, 200, rb, P, p, out)
                    view = buf[p, :int(np.prod(shp))].view(shp)
                    r.render_tile(scene, rb, P, p, out=out, into=view)
                    assert torch.equal(view, r.render_tile(scene, rb, P, p, out=out))
                assert torch.equal(r.assemble_rows(buf, 200, 117, rb, out), ref), (P, rb, out)
                assert torch.equal(tiling.assemble(buf.cpu(), 117, 200, rb, out), ref.cpu()), (P, rb, out)
                assert torch.equal(r.assemble_rows(buf.cpu(), 200, 117, rb, out), ref)  # host tiles
    with pytest.raises(ValueError):
        r.render_tile(scene, 8, 2, 0, into=torch.empty(5, device="cuda"))
    blob, S = r.scene_blob(scene)
    with pytest.raises(ValueError):
        r.render_tile(scene, blob=blob, n_spheres=S + 1)
    assert torch.equal(r.render_tile(scene, blob=blob, n_spheres=S), full)


def test_row_tile_shares_reassemble(hip):
    """Weighted shares (distributed.ROOT_SHARES): the root renders root_run parts and every other
    rank run parts of the root_run + (world-1)*run interleave, each share one render_tile(...,
    part_run=) launch; the device un-permute (rtx_assemble_runs) and the host one give the
    single-GPU frame bit for bit."""
    from python_ray_tracer_amd import tiling

    spec = scenes.readme_spec(200, 117)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(max_bounces=3, color_dtype=torch.float32)
    full = r.render(scene).data
    full_u8 = r.quantize(r.render(scene), scene.camera)
    for world, root_run, run, rb in ((4, 1, 2, 8), (8, 1, 2, 8), (3, 2, 3, 5), (5, 1, 3, 1)):
        n_parts, shares = tiling.runs(world, root_run, run)
        for out, ref, isz in ((None, full, full.element_size()), ("u8", full_u8, 1)):
            n = tiling.part_len(117, 200, rb, world, isz, out, root_run, run)
            buf = torch.full((world, n), 7, dtype=ref.dtype, device=ref.device)
            for k, (first, k_run) in enumerate(shares):
                shp = tiling.tile_shape(117, 200, rb, n_parts, first, out, k_run)
                view = buf[k, :int(np.prod(shp))].view(shp)
                r.render_tile(scene, rb, n_parts, first, out=out, into=view, part_run=k_run)
            case = (world, root_run, run, rb, out)
            assert torch.equal(r.assemble_rows(buf, 200, 117, rb, out, root_run, run), ref), case
            assert torch.equal(tiling.assemble(buf.cpu(), 117, 200, rb, out, root_run, run), ref.cpu()), case
    # a frame smaller than one cycle: the root's share holds every row, the peers' are empty (their
    # launches render nothing; an empty output needs no buffer)
    small = scenes.build_scene(scenes.readme_spec(40, 10))
    want = r.render(small).data
    n_parts, shares = tiling.runs(3, 2, 3)
    buf = torch.zeros((3, tiling.part_len(10, 40, 8, 3, 4, None, 2, 3)), dtype=torch.float32, device=want.device)
    for k, (first, k_run) in enumerate(shares):
        shp = tiling.tile_shape(10, 40, 8, n_parts, first, None, k_run)
        assert (shp[1] == 0) == (k > 0), shp
        r.render_tile(small, 8, n_parts, first, into=buf[k, :int(np.prod(shp))].view(shp), part_run=k_run)
        assert r.render_tile(small, 8, n_parts, first, part_run=k_run).shape == shp
    assert torch.equal(r.assemble_rows(buf, 40, 10, 8, None, 2, 3), want)


def test_render_batch_matches_single_frames(hip):
    """rtx_render_frames: an orbit animation (C5 camera path) and a batch of different scenes in
    ONE launch equal one render per frame bit for bit, on the fast kernel (B=3) and beyond its cap
    (B=10: the general kernel renders every ray of every frame)."""
    base = scenes.random_spec(16, 0, 96, 54)
    orbit = [scenes.build_scene(scenes.with_camera(base, scenes.orbit_position(k, 8))) for k in range(5)]
    mixed = [scenes.build_scene(scenes.random_spec(16, seed, 96, 54)) for seed in (1, 2, 3)]
    for B in (3, 10):
        r = hip.HipRenderer(max_bounces=B)
        for frames in (orbit, mixed):
            batch = r.render_batch(frames)
            assert batch.shape == (len(frames), 3, 96 * 54)
            u8 = r.render_batch(frames, out="u8")
            for f, sc in enumerate(frames):
                assert torch.equal(batch[f], r.render_tile(sc)), (B, f)
                assert torch.equal(u8[f], r.render_tile(sc, out="u8")), (B, f)
    want = O.render(O.scene_from_spec(scenes.with_camera(base, scenes.orbit_position(3, 8))), 3)
    got = hip.HipRenderer(max_bounces=3).render_batch(orbit)[3].cpu().numpy()
    assert np.abs(got - want).max() <= ATOL
    with pytest.raises(ValueError):
        r.render_batch([orbit[0], scenes.build_scene(scenes.random_spec(15, 0, 96, 54))])


def test_render_batch_ties_return_to_their_frame(hip, golden_meta, golden_renders):
    """Deferred (tied) rays of a multi-frame launch carry their frame index to the general kernel."""
    spec = golden_meta["cases"]["ties_64x36_B2"]["spec"]
    cams = ([0, 0.2, -2], [0.3, 0.25, -2.5], [0, 0.2, -2], [-0.2, 0.1, -1.8])
    frames = [scenes.build_scene(scenes.with_camera(spec, c)) for c in cams]
    r = hip.HipRenderer(max_bounces=2, collect_stats=True)
    batch = r.render_batch(frames)
    assert r.stats()["deferred"] > 200
    single = hip.HipRenderer(max_bounces=2)
    for f, sc in enumerate(frames):
        assert torch.equal(batch[f], single.render_tile(sc)), f
    assert np.abs(batch[2].cpu().numpy() - golden_renders["ties_64x36_B2"]).max() <= ATOL


def test_render_frames_driver_batches(hip, tmp_path):
    """application.render_frames with a batching renderer: PNGs equal per-frame save_image output."""
    from PIL import Image

    from python_ray_tracer_amd.application import render_frames

    base = scenes.random_spec(16, 0, 80, 45)
    frames = [scenes.build_scene(scenes.with_camera(base, scenes.orbit_position(k, 6))) for k in range(6)]
    r = hip.HipRenderer(max_bounces=3)
    cols = render_frames(frames, r, tmp_path, batch=4)
    assert sorted(cols) == list(range(6))
    for k, sc in enumerate(frames):
        ref = tmp_path / f"ref_{k}.png"
        r.save_image(r.render(sc), sc.camera, ref)
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"frame_{k:04d}.png")), np.asarray(Image.open(ref)))


def test_explicit_rays_and_intersect(hip, golden_meta):
    """rtx_trace_rays (raytrace_scene on arbitrary rays) and rtx_sphere_intersect (shape.py:28-51)."""
    spec = scenes.readme_spec(64, 36)
    sc = O.scene_from_spec(spec)
    r = hip.HipRenderer(max_bounces=3)
    scene = scenes.build_scene(spec)
    d = O.ray_directions(sc.cam, 64, 36)
    # materialised get_ray_directions equals the oracle bit for bit
    dirs = r.get_ray_directions(scene.camera)
    assert np.array_equal(dirs.data.cpu().numpy(), np.stack(d))
    # explicit rays with a shared origin == the fused camera path
    got = r.raytrace_scene(scene.camera.position, hip.HipVector3D(*d), scene).data.cpu().numpy()
    assert np.abs(got - O.render(sc, 3)).max() <= ATOL
    # per-ray origins (a second-level batch: offset origins)
    rng = np.random.default_rng(1)
    o = [np.full(d[0].shape, v) + rng.uniform(-0.1, 0.1, d[0].shape) for v in sc.cam]
    got = r.raytrace_scene(hip.HipVector3D(*o), hip.HipVector3D(*d), scene).data.cpu().numpy()
    want = np.stack(O.trace(sc, tuple(o), d, 3))
    assert np.abs(got - want).max() <= ATOL
    # the same rays with no bounce cap (the reference default): explicit rays through the deep
    # deferral, the continuation pass and the general kernel
    got = hip.HipRenderer().raytrace_scene(hip.HipVector3D(*o), hip.HipVector3D(*d), scene).data.cpu().numpy()
    want = np.stack(O.trace(sc, tuple(o), d, None))
    assert np.abs(got - want).max() <= ATOL
    # intersect known answers
    for k in json.loads((GOLDEN / "intersect_kat.json").read_text()):
        s = hip.HipSphere(hip.HipVector3D(*k["center"]), k["radius"], None)
        t = s.intersect(hip.HipVector3D(*k["origin"]), hip.HipVector3D(*[np.array([v]) for v in k["dir"]]))
        assert float(t[0]) == k["t"], k["label"]


def test_fast_sqrt_div_bit_exact(hip):
    """The kernels' sqrt / division fast paths equal the compiler's full correctly-rounded
    expansions bit for bit, and both equal the CPU's IEEE sqrt and division."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    rng = np.random.default_rng(7)
    n = 1 << 20
    e = rng.uniform(-320, 320, n)
    a = rng.uniform(0.5, 1.0, n) * np.exp2(np.round(e))
    b = rng.uniform(0.5, 1.0, n) * np.exp2(np.round(rng.uniform(-320, 320, n))) * np.where(rng.random(n) < 0.5, -1, 1)
    specials = np.array([0.0, -0.0, 1.0, 4.0, 1e-8, 2.0 ** -767, 2.0 ** -768, 2.0 ** -300, 2.0 ** 300, 1e-310,
                         np.finfo(float).max, np.inf, 0.9999999999999999, 1.0000000000000002])
    a[:specials.size] = specials
    b[:specials.size] = specials[::-1]
    a[specials.size:2 * specials.size] = np.abs(rng.normal(size=specials.size)) * 1e-8
    # squared lengths of already-unit vectors: whole waves within 2^-30 of 1 (the closed form), the
    # range edges, and one wave with a single lane outside (the general path)
    m = 1 << 16
    near = 1.0 + np.round(rng.uniform(-2.0 ** 23, 2.0 ** 23, m)) * 2.0 ** -53
    near[near > 1.0] = 1.0 + np.floor((near[near > 1.0] - 1.0) * 2.0 ** 52) * 2.0 ** -52
    near[:6] = [1.0, 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51]
    near[64 + 17] = 1.5
    a[1 << 18:(1 << 18) + m] = near
    A = torch.from_numpy(a).cuda()
    Bt = torch.from_numpy(b).cuda()
    out = torch.empty(6 * n, dtype=torch.float64, device="cuda")
    L.check(L.load().rtx_selftest_math(A.data_ptr(), Bt.data_ptr(), n, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "rtx_selftest_math")
    o = out.cpu().numpy().reshape(6, n).view(np.uint64)
    assert np.array_equal(o[0], o[1]), "fast sqrt != full sqrt"
    assert np.array_equal(o[2], o[3]), "fast div != full div"
    pos = a >= 0
    assert np.array_equal(o[4][pos], o[5][pos]), "unit renormalisation != 1 / sqrt"
    with np.errstate(all="ignore"):
        want = 1.0 / np.where(a == 0, 1.0, np.sqrt(np.where(pos, a, 0.0)))
    assert np.array_equal(o[5][pos], want[pos].view(np.uint64))
    with np.errstate(all="ignore"):
        pos = a >= 0
        assert np.array_equal(o[1][pos], np.sqrt(a[pos]).view(np.uint64))
        q = a / b
        fin = np.isfinite(q)
        assert np.array_equal(o[3][fin], q[fin].view(np.uint64))


def test_quantize_matches_numpy(hip):
    r = hip.HipRenderer(max_bounces=1)
    vals = np.concatenate([np.linspace(-0.5, 1.5, 4001), [0, 1, 1 / 255, 2 / 255, 254.99999 / 255, np.inf, -np.inf]])
    n = vals.size
    c = np.stack([vals, vals[::-1], np.roll(vals, 7)])
    from python_ray_tracer_amd.domain import Camera

    cam = Camera(hip.HipVector3D(0, 0, -1), n, 1)
    got = r.quantize(hip.HipRGBColor.from_tensor(torch.from_numpy(c).cuda()), cam).cpu().numpy()
    assert np.array_equal(got, O.to_uint8(c, n, 1))


def test_unbounded_recursion_limit(hip):
    """Rays trapped inside a mirror sphere reflect forever (a negative radius flips the normal, so
    the nudged point stays inside): the reference hits Python's recursion limit; HipRenderer raises
    RecursionError past UNBOUNDED_LEVELS."""
    spec = scenes.readme_spec(8, 8)
    spec["spheres"] = [{"center": [0, 0.2, -2], "radius": -5.0,
                        "shader": {"reflection_gain": 1, "specular_gain": 1.0, "specular_roughness": 0.5,
                                   "iridescence_gain": 0, "diffuse_gain": 0.5,
                                   "texture": {"kind": "const", "color": [1, 1, 1]}}}]
    spec["lights"][0]["position"] = [0, 0.2, -2]
    r = hip.HipRenderer()
    scene = scenes.build_scene(spec)
    with pytest.raises(RecursionError):
        r.render(scene)


def test_unbounded_status_read_back_once_per_clean_render(hip, monkeypatch):
    """An uncapped render reads the kernel's status word back (a host round trip) to raise
    RecursionError at the call, as the reference does. The kernels are deterministic, so once a
    render of a (scene content, tile, cap) has come back clean, identical renders skip the read-back;
    a render that flagged something (trapped rays) is checked, and raises, every time."""
    r = hip.HipRenderer()  # unbounded, like the reference
    spec = scenes.readme_spec(64, 36)
    scene = scenes.build_scene(spec)
    first = r.render(scene).data.clone()
    assert len(r._clean) == 1
    calls = []
    orig = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append(1), orig(self))[1])
    again = r.render(scene).data
    monkeypatch.undo()
    assert not calls and torch.equal(first, again)
    assert np.abs(again.cpu().numpy() - O.render(O.scene_from_spec(spec), None)).max() <= ATOL
    trapped = scenes.readme_spec(8, 8)
    trapped["spheres"] = [{"center": [0, 0.2, -2], "radius": -5.0,
                           "shader": {"reflection_gain": 1, "specular_gain": 1.0, "specular_roughness": 0.5,
                                      "iridescence_gain": 0, "diffuse_gain": 0.5,
                                      "texture": {"kind": "const", "color": [1, 1, 1]}}}]
    trapped["lights"][0]["position"] = [0, 0.2, -2]
    for _ in range(2):
        with pytest.raises(RecursionError):
            r.render(scenes.build_scene(trapped))
    assert len(r._clean) == 1


@pytest.mark.parametrize("cap", [61, 80])
def test_deep_chains_resume_past_levels_30_and_60(hip, cap):
    """every chain deterministically outlives both resume records of the uncapped
    pipeline and then ends. Rays trapped in a negative-radius mirror sphere (camera and light at its
    centre: every hit lit, g = 1) reflect until the cap, so each pixel is deferred by the first DEEP
    pass with its 10-word record at level 30 (kFirstPassLevels), continued from rin[6..9] by the
    continuation pass to its level-60 record (kDeepLevel3), and finished by the general kernel
    resuming from that record (cap 80: levels 61-80; cap 61: the single level past the record).
    Colour, uint8 and the per-level ray/hit counters (levels 0-63) against the oracle."""
    spec = scenes.readme_spec(24, 16)
    spec["spheres"] = [{"center": [0, 0.2, -2], "radius": -5.0,
                        "shader": {"reflection_gain": 1, "specular_gain": 1.0, "specular_roughness": 0.5,
                                   "iridescence_gain": 0.05, "diffuse_gain": 0.5,
                                   "texture": {"kind": "const", "color": [0.9, 0.7, 0.4]}}}]
    spec["lights"][0]["position"] = [0, 0.2, -2]
    osc = O.scene_from_spec(spec)
    st = O.TraceStats()
    want = O.render(osc, cap, stats=st)
    assert len(st.rays) == cap + 1 and st.rays[31] == st.rays[61] == 24 * 16  # every chain passes 31 and 61
    r = hip.HipRenderer(max_bounces=cap, color_dtype=torch.float64)
    got = r.render(scenes.build_scene(spec)).data.cpu().numpy()
    assert np.abs(got - want).max() <= ATOL, (cap, np.abs(got - want).max())
    assert np.array_equal(O.to_uint8(got, 24, 16), O.to_uint8(want, 24, 16))
    rs = hip.HipRenderer(max_bounces=cap, collect_stats=True)
    rs.render(scenes.build_scene(spec))
    s = rs.stats()
    n = min(len(st.rays), hip._lib.S_LEVELS)
    assert s["rays"][:n] == st.rays[:n] and s["hits"][:n] == st.hits[:n]


@pytest.mark.parametrize("seed", range(14))
def test_fuzz_scenes_against_oracle(hip, seed):
    """Random scenes, cameras, sizes and bounce caps (both kernels; culled and linear sphere
    loops): colour within ATOL, identical uint8, per-level ray/hit counts equal the oracle's."""
    spec = _fuzz_spec(seed)
    B = [0, 1, 2, 3, 5, 8, 9][seed % 7]
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL, (seed, np.abs(got - want).max())
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    assert np.array_equal(O.to_uint8(got, W, H), O.to_uint8(want, W, H))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits, seed


@pytest.mark.parametrize("seed", [0, 3, 5])
def test_untamed_scene_takes_reference_expressions(hip, seed):
    """A fuzz scene with one sphere beyond 2^60 (RTX_H_TAME = 0): the fast kernel evaluates the
    reference's sphere-test expressions instead of the half-b form, and still equals the oracle;
    so does the explicit-ray path on the tamed original."""
    spec = _fuzz_spec(seed)
    far = spec["spheres"][0]
    far["center"] = [3e18, 2e18, 4e19]
    far["radius"] = 3e18
    B = 3
    r, got = _render(hip, spec, B, stats=True)
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P
    assert P.pack_scene(scenes.build_scene(spec))[P.L.H_TAME] == 0.0
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL, (seed, np.abs(got - want).max())
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    assert np.array_equal(O.to_uint8(got, W, H), O.to_uint8(want, W, H))
    assert r.stats()["rays"] == st.rays


def test_rays_at_right_angles_take_reference_expressions(hip):
    """A sphere centred exactly on the camera: every primary ray has h = D.(O - C) = 0, so every
    wave's half-b test falls back to the reference expressions (SphTest, |h| < 2^-350) at level 0,
    while the other spheres keep the half-b form; colour, uint8 and counters equal the oracle."""
    spec = scenes.readme_spec(64, 36)
    cam = spec["camera"]["position"]
    spec["spheres"].insert(0, dict(spec["spheres"][0], center=list(cam), radius=0.25))
    B = 3
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL, np.abs(got - want).max()
    assert np.array_equal(O.to_uint8(got, 64, 36), O.to_uint8(want, 64, 36))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits


@pytest.mark.parametrize("B", [3, 4])
def test_big_scene_register_level_kernel(hip, B):
    """65 spheres at caps 3 and 4, a big scene table in LDS beside a mid-size cap (the name dates from
    a choice between two kernels that launch_fast_b no longer makes: every cap has one capped
    kernel); colour, uint8 and counters."""
    spec = scenes.random_spec(64, 3, 96, 54)
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL, np.abs(got - want).max()
    assert np.array_equal(O.to_uint8(got, 96, 54), O.to_uint8(want, 96, 54))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("layout", sorted(HUGE_LAYOUTS))
def test_huge_tail_layouts(hip, layout, B):
    """Huge spheres ending the scene (RTX_H_NBEAM: the tile frustums' and reflected-ray beams'
    candidates without a test) before, at and after sphere 64, inside the scene, and absent; the
    persistent culled kernel against the oracle: colour, uint8 and counters."""
    spec = huge_tail_spec(layout, 80, 45)
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL, np.abs(got - want).max()
    assert np.array_equal(O.to_uint8(got, 80, 45), O.to_uint8(want, 80, 45))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits


def test_vector_algebra_on_device(hip):
    """HipVector3D with device tensors (the reference's NumpyVector3D algebra, base.py:28-79) equals
    the NumPy expressions bit for bit, norm's zero guard and sqrt included."""
    rng = np.random.default_rng(9)
    a = rng.normal(size=(3, 4097)) * rng.choice([1e-3, 1.0, 1e3], size=(1, 4097))
    a[:, 11] = 0.0
    v = hip.HipVector3D(*(torch.from_numpy(c).cuda() for c in a))
    mag = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    want = a * (1.0 / np.where(mag == 0, 1, mag))
    got = [c.cpu().numpy() for c in v.norm().components()]
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(abs(v).cpu().numpy(), (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


@pytest.mark.parametrize("B", [3, None])
def test_large_scene_without_lds_table(hip, B):
    """More than 128 spheres: the fast kernel reads materials from HBM instead of its LDS copy (the
    other instantiation), the culling tree has many levels; capped and unbounded (continuation and
    general kernel) against the oracle."""
    spec = scenes.random_spec(150, 4, 72, 40)
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL
    assert np.array_equal(O.to_uint8(got, 72, 40), O.to_uint8(want, 72, 40))
    assert r.stats()["rays"] == st.rays



@pytest.mark.parametrize("seed", range(14, 22))
def test_fuzz_scenes_deep_caps(hip, seed):
    """The fuzz scenes with no cap and caps beyond the fast kernels (the continuation passes, the
    DEEP kernel's LDS and register variants, the general kernel): colour, uint8 and counters."""
    spec = _fuzz_spec(seed)
    B = [None, 12, 20, None][seed % 4]
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    assert np.abs(got - want).max() <= ATOL, (seed, np.abs(got - want).max())
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    assert np.array_equal(O.to_uint8(got, W, H), O.to_uint8(want, W, H))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits, seed


def test_shader_create_matches_reference(hip):
    """HipShader.create (rtx_shade_hits) == the reference NumpyShader.create called directly
    (tests/golden/create_kat.*: rays that hit the shape, nearest or not; capped and unbounded),
    and == the oracle on a larger batch, through the scene's own shader and a foreign one."""
    z = np.load(GOLDEN / "create_kat.npz")
    meta = json.loads((GOLDEN / "create_kat.json").read_text())
    for name, c in meta["cases"].items():
        scene = scenes.build_scene(c["spec"])
        shape = scene.shapes[c["shape"]]
        shader = scene.shapes[c.get("shader_of", c["shape"])].shader  # the shape's own, or another's
        r = hip.HipRenderer(max_bounces=c["max_bounces"])
        col = shader.create(shape, scene, hip.HipVector3D(*c["origin"]), hip.HipVector3D(*z[name + "_dirs"]),
                            z[name + "_t"], r)
        assert np.abs(col.data.cpu().numpy() - z[name + "_rgb"]).max() <= ATOL, name
    # a bigger batch with per-ray origins against the oracle; and another shape's shader
    spec = scenes.random_spec(16, 3, 80, 45)
    scene = scenes.build_scene(spec)
    sc = O.scene_from_spec(spec)
    d = O.ray_directions(sc.cam, 80, 45)
    for si, B, foreign in ((16, 3, None), (4, None, None), (16, 2, 7)):
        t = O.intersect(sc.spheres[si], *sc.cam, *d)
        hit = t != O.FARAWAY
        dd = tuple(c[hit] for c in d)
        r = hip.HipRenderer(max_bounces=B)
        shader = scene.shapes[si].shader if foreign is None else scene.shapes[foreign].shader
        got = shader.create(scene.shapes[si], scene, hip.HipVector3D(*sc.cam), hip.HipVector3D(*dd), t[hit], r)
        mat = None if foreign is None else sc.spheres[foreign]  # level 0 only; reflections see the scene
        want = np.stack(O.create(sc, si, sc.cam, dd, t[hit], B, material=mat))
        assert np.abs(got.data.cpu().numpy() - want).max() <= ATOL, (si, B, foreign)
    with pytest.raises(ValueError):
        scene.shapes[0].shader.create(hip.HipSphere(hip.HipVector3D(0, 0, 0), 1.0, None), scene,
                                      hip.HipVector3D(*sc.cam), hip.HipVector3D(*dd), t[hit], r)


@pytest.mark.parametrize("B", [3, None])
def test_image_textured_spheres(hip, B):
    """ImageTexture / HipTexturedSphere (the per-point mapping of shape.py:66-79, pinned on the
    reference's own diffusecolor by tests/golden/texture_kat.json through the oracle): renders
    against the oracle. ROCm's atan2/asin and NumPy's may pick the neighbour texel for a point
    within an ulp of a texel edge (parity unpinned at that level): at most 1 pixel in 10^4 may differ,
    every other pixel within 1e-12. Also through reflections (the mirror-ish sphere) and create()."""
    spec = _textured_spec(160, 90)
    r, got = _render(hip, spec, B, stats=True)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), B, stats=st)
    bad = (np.abs(got - want) > ATOL).any(axis=0)
    assert bad.sum() <= max(1, got.shape[1] // 10000), bad.sum()
    assert r.stats()["rays"] == st.rays
    # HipTexturedSphere (the reference class's signature) == ImageTexture through HipShader
    from python_ray_tracer_amd.domain import Scene3D

    scene = scenes.build_scene(spec)
    img = spec["spheres"][0]["shader"]["texture"]["texels"]
    ts = hip.HipTexturedSphere(hip.HipVector3D(-0.9, 0.2, 2.0), 0.6, (img * 255).round().astype(np.uint8))
    scene2 = Scene3D([ts] + list(scene.shapes)[1:], scene.lights, scene.camera)
    r2 = hip.HipRenderer(max_bounces=B)
    got2 = r2.render(scene2).data.cpu().numpy()
    assert np.abs(got2 - got).max() <= ATOL


@pytest.mark.parametrize("B", [1, 3, 5])
def test_fast_kernel_texturing_build(hip, B):
    """RTX_F_IMAGES: the capped fast kernel's texturing build shades image-textured hits itself
    (HipRenderer(fast_textures=True), the default) — whole frames and row tiles bit-identical to
    the renders that defer those pixels to the general kernel, and fewer pixels deferred (the
    textured hits stay in the fast kernel)."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    for W, H, S in ((160, 90, None), (96, 64, 40)):  # 40 spheres: the persistent culled kernel
        spec = _textured_spec(W, H)
        if S:
            extra = scenes.random_spec(S, 3, W, H)
            spec = dict(spec, spheres=spec["spheres"] + extra["spheres"][:S - len(spec["spheres"])])
        scene = scenes.build_scene(spec)
        fast = hip.HipRenderer(max_bounces=B, color_dtype=torch.float32)
        slow = hip.HipRenderer(max_bounces=B, color_dtype=torch.float32, fast_textures=False)
        assert torch.equal(fast.render(scene).data, slow.render(scene).data), (B, S)
        # the texturing build against the oracle directly (not only against the general kernel):
        # float64 colour within 1e-12, up to 1 pixel in 10^4 on a texel edge (atan2 / asin, as in
        # test_image_textured_spheres); the first render learns the order, the second is the timed path
        f64 = hip.HipRenderer(max_bounces=B, color_dtype=torch.float64)
        want = O.render(O.scene_from_spec(spec), B)
        for _ in range(2):
            got = f64.render(scene).data.cpu().numpy()
            bad = (np.abs(got - want) > ATOL).any(axis=0)
            assert bad.sum() <= max(1, got.shape[1] // 10000), (B, S, int(bad.sum()))
        for P, part in ((3, 1), (4, 3)):
            assert torch.equal(fast.render_tile(scene, 8, P, part, out="u8"),
                               slow.render_tile(scene, 8, P, part, out="u8")), (B, S, P)
        blob, n = fast.scene_blob(scene)
        ws = fast.workspace(W * H)
        out = torch.empty((3, W * H), dtype=torch.float32, device=fast.device)
        word = torch.full((1,), 7, dtype=torch.int32, device=fast.device)
        deferred = []
        for flags in (L.F_IMAGES, 0):
            L.check(fast._lib.rtx_render_camera_ex(blob.data_ptr(), n, W, H, 1, 1, 0, H, B, out.data_ptr(),
                                                   L.OUT_F32_SOA, ws.data_ptr(), ws.numel(), None,
                                                   fast._stream(), flags, word.data_ptr()), "rtx_render_camera_ex")
            torch.cuda.synchronize()
            deferred.append(int(word.item()))
        assert deferred[0] < deferred[1], (B, S, deferred)  # the textured hits no longer deferred


@pytest.mark.parametrize("B", [3, None])
def test_textured_batch_matches_single_frames(hip, B):
    """A multi-frame launch (rtx_render_frames) of an orbit around the textured scene: the
    image-textured hits of every frame go to the general kernel with their frame index (its
    waterfall over frames), and each frame equals its single-frame render bit for bit."""
    base = _textured_spec(64, 36)
    frames = [scenes.build_scene(scenes.with_camera(base, scenes.orbit_position(k, 6))) for k in range(4)]
    r = hip.HipRenderer(max_bounces=B)
    batch = r.render_batch(frames)
    for f, sc in enumerate(frames):
        assert torch.equal(batch[f], r.render_tile(sc)), (B, f)


@pytest.mark.parametrize("B", [3, None])
def test_textured_row_tiles_reassemble(hip, B):
    """Row tiles of the textured scene (its image-textured hits deferred from each tile to the
    general kernel, which maps the tile's local pixel back to its frame row): reassembled they equal
    the whole frame bit for bit."""
    from python_ray_tracer_amd import tiling

    spec = _textured_spec(96, 61)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(max_bounces=B)
    full = r.render(scene).data
    for P, rb in ((3, 4), (4, 8)):
        n = tiling.part_len(61, 96, rb, P, full.element_size(), None)
        buf = torch.zeros((P, n), dtype=full.dtype, device=full.device)
        for p in range(P):
            shp = tiling.tile_shape(61, 96, rb, P, p, None)
            r.render_tile(scene, rb, P, p, into=buf[p, :int(np.prod(shp))].view(shp))
        assert torch.equal(r.assemble_rows(buf, 96, 61, rb, None), full), (B, P, rb)


@pytest.mark.parametrize("B", [3, 4, None])
def test_small_scene_with_a_tree_renders_without_it(hip, B):
    """Scenes below 8 spheres run the TP = 0 kernel, which compiles no culling-tree walk. A blob of
    such a scene that carries a tree anyway (packed with BVH_MIN_SPHERES lowered) must render what
    the linear loops render — the tree only culls — and equal the oracle."""
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P

    spec = scenes.random_spec(5, 7, 64, 40)  # 6 spheres with the ground
    old = P.BVH_MIN_SPHERES
    try:
        P.BVH_MIN_SPHERES = 2
        P._pack_static.cache_clear()
        r, got = _render(hip, spec, B)
        assert r.scene_blob(scenes.build_scene(spec))[0][P.L.H_NNODES].item() > 0  # the tree is there
    finally:
        P.BVH_MIN_SPHERES = old
        P._pack_static.cache_clear()
    want = O.render(O.scene_from_spec(spec), B)
    assert np.abs(got - want).max() <= ATOL
    _, plain = _render(hip, spec, B)
    assert np.array_equal(got, plain)


@pytest.mark.parametrize("cap", [2, None])
@pytest.mark.parametrize("n", range(9))
def test_sphere_loop_tails_one_to_nine_spheres(hip, n, cap):
    """1 to 9 spheres (n random ones and the ground): the odd and even tails of every sphere-pair
    scan, each compile-time sphere count of the small-scene kernels (1..7) and both sides of
    kTreeMinSpheres. The counting kernels against the oracle (colour, uint8, per-level rays and
    hits), then three renders on one timed renderer (the third runs with the learnt dispatch order
    and the decided general-kernel flag), bit-identical to each other and within ATOL of the
    oracle."""
    spec = scenes.random_spec(n, n, 32, 16)
    st = O.TraceStats()
    want = O.render(O.scene_from_spec(spec), cap, stats=st)
    r, got = _render(hip, spec, cap, stats=True)
    assert np.abs(got - want).max() <= ATOL, np.abs(got - want).max()
    assert np.array_equal(O.to_uint8(got, 32, 16), O.to_uint8(want, 32, 16))
    s = r.stats()
    assert s["rays"] == st.rays and s["hits"] == st.hits
    r2 = hip.HipRenderer(max_bounces=cap, color_dtype=torch.float64)
    scene = scenes.build_scene(spec)
    frames = [r2.render_tile(scene).cpu().numpy() for _ in range(3)]
    assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])
    timed = frames[2].reshape(want.shape)
    assert np.abs(timed - want).max() <= ATOL, np.abs(timed - want).max()
    assert np.array_equal(O.to_uint8(timed, 32, 16), O.to_uint8(want, 32, 16))


WORK_COUNTERS = ("sphere_tests", "node_tests", "sphere_tests_reflected", "node_tests_reflected", "box_tests",
                 "beam_tests", "beam_searches")
WORK_SCENES = {
    "rand2_32x16": lambda: scenes.random_spec(2, 0, 32, 16),            # no culling tree
    "rand15_48x27": lambda: scenes.random_spec(15, 1, 48, 27),          # a tree, one tile per block
    "rand39_64x36": lambda: scenes.random_spec(39, 2, 64, 36),          # persistent: beams, shadow grid
    "tail_below_64_80x45": lambda: huge_tail_spec("tail_below_64", 80, 45),
}


def work_counters(H, name, cap):
    r, _ = _render(H, WORK_SCENES[name](), cap, stats=True)
    s = r.stats()
    return {k: s[k] for k in WORK_COUNTERS}


@pytest.mark.parametrize("cap", [3, None])
@pytest.mark.parametrize("name", sorted(WORK_SCENES))
def test_executed_work_counters_are_pinned(hip, name, cap):
    """The executed-work counters under bench.py's FLOP model (sphere, node, box and beam tests, of
    all rays and of reflected rays) equal the values recorded in tests/golden/work_counters.json
    from the commit named there: where the searches count their work must not move."""
    golden = json.loads((GOLDEN / "work_counters.json").read_text())
    want = golden["cases"][f"{name}_B{cap}"]
    assert work_counters(hip, name, cap) == want
