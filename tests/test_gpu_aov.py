"""Primary-hit render passes on the GPU: HipRenderer.render_aovs / trace_aovs, rtx_primary_aovs.

Every pass is a decided value (id, hits, lit, the checker cell, the texel) or a correctly rounded
float64 expression in the reference's operation order (depth, position, normal), so every comparison
with the NumPy reference (tests/aov_ref.py, pinned to the oracle by tests/test_aov_cpu.py) is
np.array_equal: there is no tolerance. The frames are 50 x 22 (no multiple of a wave or of the
kernel's 256-ray blocks) unless the scene brings its own size.
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes, tiling
from tests import aov_ref, specs

pytestmark = pytest.mark.gpu

W, H = 50, 22
PASSES = aov_ref.PASSES


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _equal(got: dict, ref: dict, names=PASSES, sel=None, what=""):
    assert tuple(got) == tuple(names), (what, tuple(got))
    for k in names:
        g = got[k].cpu().numpy()
        want = ref[k] if sel is None else ref[k][..., sel]
        assert g.dtype == want.dtype and g.shape == want.shape, (what, k, g.dtype, g.shape, want.shape)
        bad = int((g != want).sum()) if g.shape == want.shape else -1
        assert np.array_equal(g, want), (what, k, f"{bad} of {want.size} values differ")


SCENES = {
    "readme": lambda: scenes.readme_spec(W, H),
    "main": lambda: scenes.main_spec(W, H),
    "rand16": lambda: scenes.random_spec(16, 0, W, H),  # a culling tree
    "rand64": lambda: scenes.random_spec(64, 0, W, H),  # a tree, a shadow grid, the persistent kernel's sphere count
    "rand150": lambda: scenes.random_spec(150, 0, W, H),  # above 128 spheres: the table is out of LDS in the render kernels
    "trapped": lambda: specs.trapped_spec(24, 16),  # a negative radius, inward normals, the camera inside
    "fuzz3": lambda: specs.fuzz_spec(3),  # every pixel lit (the camera inside a sphere)
    "fuzz10": lambda: specs.fuzz_spec(10),  # every pixel in shadow
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_passes_equal_the_reference(hip, name):
    spec = SCENES[name]()
    oscene, ref = aov_ref.frame(name, SCENES[name])
    hit = ref["id"] >= 0
    if name == "fuzz3":
        assert hit.all() and ref["lit"].all()
    if name == "fuzz10":
        assert hit.all() and not ref["lit"].any()
    if name == "trapped":
        assert oscene.spheres[0].radius < 0 and hit.all()
    scene = scenes.build_scene(spec)
    got = hip.HipRenderer(3).render_aovs(scene)
    n = oscene.width * oscene.height
    assert got["depth"].shape == (n,) and got["position"].shape == (3, n) and got["lit"].dtype == torch.uint8
    _equal(got, ref, what=name)


def test_ties_take_the_first_shape_in_scene_order(hip, golden_meta):
    spec = golden_meta["cases"]["ties_64x36_B2"]["spec"]
    oscene, ref = aov_ref.frame("ties", lambda: spec)
    tie = ref["hits"] > 1
    assert int(tie.sum()) == 226
    got = hip.HipRenderer(2).render_aovs(scenes.build_scene(spec))
    _equal(got, ref, what="ties")
    # id is the first of the tied shapes: no shape before it is at the nearest distance
    origin, dirs = aov_ref.frame_rays(oscene)
    ident = got["id"].cpu().numpy()
    for si, sp in enumerate(oscene.spheres):
        d = O.intersect(sp, *origin, *dirs)
        assert not (tie & (d == ref["depth"]) & (ident > si)).any(), si


def test_image_textures_are_exact(hip):
    oscene, ref = aov_ref.frame("textured", lambda: specs.textured_spec(W, H))
    assert int(np.isin(ref["id"], [0, 1]).sum()) == 241
    got = hip.HipRenderer(3).render_aovs(scenes.build_scene(specs.textured_spec(W, H)))
    _equal(got, ref, what="textured")


def test_pass_subsets_equal_the_all_pass_call(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(3)
    full = r.render_aovs(scene)
    assert tuple(full) == PASSES
    rays = r.get_ray_directions(scene.camera).data
    for names in (("depth",), ("id", "hits"), ("lit",), ("albedo", "normal"), PASSES):
        order = tuple(k for k in PASSES if k in names)
        for got in (r.render_aovs(scene, passes=names), r.trace_aovs(scene.camera.position, rays, scene, passes=names)):
            assert tuple(got) == order, names
            for k in order:
                assert torch.equal(got[k], full[k]), (names, k)


def test_row_tiles_equal_the_rows_of_the_whole_frame(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    _, ref = aov_ref.frame("readme", lambda: scenes.readme_spec(W, H))
    r = hip.HipRenderer(3)
    full = r.render_aovs(scene)
    rb = 4
    layouts = [(3, [(p, 1) for p in range(3)])]  # a 3-way interleave
    layouts.append(tiling.runs(3, 1, 2))  # and runs (root_run, run) = (1, 2) over 3 ranks
    for P, tiles in layouts:
        seen = []
        for first, run in tiles:
            rows = tiling.tile_rows(H, rb, P, first, run)
            seen += list(rows)
            pix = (np.asarray(rows)[:, None] * W + np.arange(W)[None, :]).reshape(-1)
            got = r.render_aovs(scene, row_block=rb, n_parts=P, part=first, part_run=run)
            _equal(got, ref, sel=pix, what=(P, first, run))
            dev = torch.as_tensor(pix, device=got["id"].device)
            for k in PASSES:
                assert torch.equal(got[k], full[k][..., dev]), (P, first, run, k)
        assert sorted(seen) == list(range(H))


def test_explicit_rays(hip):
    spec = scenes.readme_spec(W, H)
    scene = scenes.build_scene(spec)
    oscene, ref = aov_ref.frame("readme", lambda: scenes.readme_spec(W, H))
    r = hip.HipRenderer(3)
    full = r.render_aovs(scene)
    D = r.get_ray_directions(scene.camera).data  # the frame's materialised directions
    n = W * H
    cam = [float(c) for c in oscene.cam]
    per_ray = torch.tensor(cam, dtype=torch.float64, device=D.device)[:, None].expand(3, n).contiguous()
    for origin in (per_ray, scene.camera.position):  # stride n and stride 0
        got = r.trace_aovs(origin, D, scene)
        for k in PASSES:
            assert torch.equal(got[k], full[k]), k
    # level-1 rays: the nudged origins and reflected directions of every level-0 hit (O._shade)
    origin, dirs = aov_ref.frame_rays(oscene)
    qs, rs = [], []
    for si, sp in enumerate(oscene.spheres):
        m = ref["id"] == si
        _, _, _, _, q, refl = O._shade(oscene, si, sp, *origin, *(c[m] for c in dirs), ref["depth"][m])
        qs.append(np.stack(q))
        rs.append(np.stack(refl))
    q, refl = np.concatenate(qs, axis=1), np.concatenate(rs, axis=1)
    assert q.shape == refl.shape == (3, 745)
    want = aov_ref.aovs(oscene, tuple(q), tuple(refl))
    assert (want["id"] >= 0).any() and (want["id"] < 0).any() and len(np.unique(want["id"])) == 4
    got = r.trace_aovs(hip.HipVector3D(*q), hip.HipVector3D(*refl), scene)
    _equal(got, want, what="level 1")
    # a single ray, and an empty tile
    one = r.trace_aovs(scene.camera.position, hip.HipVector3D(*(c[:1] for c in refl)), scene, passes=("id", "depth"))
    assert one["id"].shape == (1,) and one["depth"].shape == (1,)
    empty = r.render_aovs(scene, row_block=8, n_parts=4, part=3)  # rows 24..31 of 22
    assert all(t.shape[-1] == 0 for t in empty.values()) and tuple(empty) == PASSES


def test_ops_equal_the_renderer_methods(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    L = hip._lib
    scene = scenes.build_scene(scenes.random_spec(16, 0, W, H))
    r = hip.HipRenderer(3)
    blob, S = r.scene_blob(scene)
    assert S == 17
    full = r.render_aovs(scene)
    got = torch.ops.rt.primary_aovs(blob, S, W, H, 1, 1, 0, 1, L.AOV_ALL)
    assert len(got) == 7
    for t, k in zip(got, PASSES):
        assert t.dtype == full[k].dtype and torch.equal(t, full[k]), k
    tile = torch.ops.rt.primary_aovs(blob, S, W, H, 4, 3, 1, 2, L.AOV_ID | L.AOV_LIT, False)
    want = r.render_aovs(scene, ("id", "lit"), row_block=4, n_parts=3, part=1, part_run=2)
    assert len(tile) == 2 and torch.equal(tile[0], want["id"]) and torch.equal(tile[1], want["lit"])
    D = r.get_ray_directions(scene.camera).data
    cam = torch.tensor([float(c) for c in scene.camera.position.components()], dtype=torch.float64, device=D.device)
    rays = torch.ops.rt.primary_aovs_rays(blob, S, cam, D, L.AOV_ALL)
    for t, k in zip(rays, PASSES):
        assert torch.equal(t, full[k]), k
    sub = torch.ops.rt.primary_aovs_rays(blob, S, cam[:, None].expand(3, W * H).contiguous(), D,
                                         L.AOV_DEPTH | L.AOV_NORMAL)
    assert len(sub) == 2 and torch.equal(sub[0], full["depth"]) and torch.equal(sub[1], full["normal"])
    with pytest.raises(RuntimeError, match="n_spheres"):  # the header check of the render ops
        torch.ops.rt.primary_aovs(blob, S - 1, W, H, 1, 1, 0, 1, L.AOV_ALL)


def test_passes_drive_the_shader_plugin(hip):
    """depth and id are what Shader.create needs: shading every shape's pixels from them gives the
    render's colour (the project's 1e-12 bar; the frame has no tie), and a miss is black."""
    B = 3
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(B)
    a = r.render_aovs(scene, ("depth", "id"))
    color = r.render(scene).data
    D = r.get_ray_directions(scene.camera).data
    assert not color[:, a["id"] < 0].any() and int((a["id"] < 0).sum()) == 355
    for si, shape in enumerate(scene.shapes):
        m = a["id"] == si
        assert m.any()
        got = r.shade_hits(shape, scene, scene.camera.position, D[:, m].contiguous(), a["depth"][m])
        err = float((got - color[:, m]).abs().max())
        print(f"shape {si}: max|shade_hits - render| = {err:.3e}")
        assert err <= 1e-12, (si, err)


def test_refusals(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r2 = hip.HipRenderer(3, samples=2)
    rays = hip.HipRenderer(3).get_ray_directions(scene.camera).data
    with pytest.raises(ValueError, match="samples=2"):
        r2.render_aovs(scene)
    with pytest.raises(ValueError, match="samples=2"):
        r2.trace_aovs(scene.camera.position, rays, scene)
    r = hip.HipRenderer(3)
    for bad in (("depth", "colour"), ("Depth",), ()):
        with pytest.raises(ValueError, match="passes"):
            r.render_aovs(scene, passes=bad)
        with pytest.raises(ValueError, match="passes"):
            r.trace_aovs(scene.camera.position, rays, scene, passes=bad)
