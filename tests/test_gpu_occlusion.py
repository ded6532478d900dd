"""Occlusion passes on the GPU: HipRenderer.render_occlusion / trace_occlusion, rtx_occlusion.

Every sample of a bundle is decided by the reference's own sphere tests in float64, and a pass is a
count of samples divided once, so every comparison with the NumPy restatement (tests/occlusion_ref.py,
fed with the GPU's own id, position and normal passes, which tests/test_gpu_aov.py pins to the
reference) is np.array_equal on the float32 outputs: there is no tolerance, a mismatch is a bug. The
floors keep equality from passing trivially; tests/test_occlusion_cpu.py holds the measured counts.
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import occlusion, scenes, tiling
from python_ray_tracer_amd.domain import Vector3D
from tests import occlusion_ref as R
from tests.test_occlusion_cpu import MAIN_SOFT, PINHOLE, SCENES, partial

pytestmark = pytest.mark.gpu

W, H = 50, 22
INPUTS = ("id", "position", "normal")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _check(hip, spec, what="", **kw):
    """render_occlusion of ``spec`` against the restatement on the GPU's own primary hits; returns the
    passes as NumPy arrays (and the hits' ``id``)."""
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    got = r.render_occlusion(scene, **kw)
    a = {k: v.cpu().numpy() for k, v in r.render_aovs(scene, INPUTS).items()}
    names = occlusion.pass_names(kw.get("passes", R.PASSES))
    ref = R.occlusion(O.scene_from_spec(spec), a["id"], a["position"], a["normal"],
                      **{**{k: v for k, v in kw.items() if k in ("side", "max_distance", "light_radius")},
                         "passes": names})
    assert tuple(got) == names, (what, tuple(got))
    out = {"id": a["id"]}
    for k in names:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == a["id"].shape, (what, k, g.dtype, g.shape)
        bad = int((g != ref[k]).sum())
        print(f"{what} {k}: {bad} of {g.size} differ, {partial(g)} partial")
        assert np.array_equal(g, ref[k]), (what, k, f"{bad} of {g.size} values differ")
        out[k] = g
    miss = a["id"] < 0
    if "ao" in out:
        assert (out["ao"][miss] == 1).all()
    if "soft_lit" in out:
        assert not out["soft_lit"][miss].any()
    return out


@pytest.mark.parametrize("side", [1, 2, 3, 8])
def test_ambient_occlusion_of_the_readme_scene(hip, side):
    o = _check(hip, scenes.readme_spec(W, H), f"readme side {side}", side=side, passes=("ao",))
    assert int((o["id"] >= 0).sum()) == 745
    if side >= 2:
        assert partial(o["ao"]) >= 300
    else:
        assert set(np.unique(o["ao"]).tolist()) == {0.0, 1.0}


def test_max_distance_limits_the_occluders(hip):
    near = _check(hip, scenes.readme_spec(W, H), "readme 0.5", side=3, max_distance=0.5, passes=("ao",))
    far = _check(hip, scenes.readme_spec(W, H), "readme", side=3, passes=("ao",))
    assert partial(near["ao"]) >= 100 and int((near["ao"] != far["ao"]).sum()) >= 100
    assert (near["ao"] >= far["ao"]).all()  # a nearer limit only removes occluders


@pytest.mark.parametrize("radius", sorted(MAIN_SOFT))
def test_soft_shadows_of_the_main_scene(hip, radius):
    o = _check(hip, scenes.main_spec(W, H), f"main radius {radius}", side=3, light_radius=radius, passes=("soft_lit",))
    assert partial(o["soft_lit"]) >= MAIN_SOFT[radius][1]


@pytest.mark.parametrize("key", sorted(SCENES))
def test_scenes_with_and_without_a_culling_tree(hip, key):
    make, side, radius, ao_floor, soft_floor = SCENES[key]
    o = _check(hip, make(), key, side=side, light_radius=radius)
    assert partial(o["ao"]) >= ao_floor and partial(o["soft_lit"]) >= soft_floor
    if key == "fuzz3":
        assert (o["id"] >= 0).all() and o["id"].size == 468


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (67, 5)])
def test_frames_that_end_inside_a_wave(hip, size):
    o = _check(hip, scenes.readme_spec(*size), f"readme {size}", side=2, light_radius=1.0)
    if size == (1, 1):
        assert o["id"].tolist() == [-1] and o["ao"].tolist() == [1.0] and o["soft_lit"].tolist() == [0.0]
    if size == (67, 5):
        assert partial(o["ao"]) >= 150


def test_row_tiles_equal_the_rows_of_the_whole_frame(hip):
    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(3)
    kw = dict(side=2, light_radius=1.0)
    full = r.render_occlusion(scene, **kw)
    assert partial(full["ao"].cpu().numpy()) >= 300
    rb = 4
    layouts = [(3, [(p, 1) for p in range(3)])]  # a 3-way interleave
    layouts.append(tiling.runs(3, 1, 2))  # and runs (root_run, run) = (1, 2) over 3 ranks
    for P, tiles in layouts:
        seen = []
        for first, run in tiles:
            rows = tiling.tile_rows(H, rb, P, first, run)
            seen += list(rows)
            pix = torch.as_tensor((np.asarray(rows)[:, None] * W + np.arange(W)[None, :]).reshape(-1), device="cuda")
            got = r.render_occlusion(scene, row_block=rb, n_parts=P, part=first, part_run=run, **kw)
            for k in R.PASSES:
                assert torch.equal(got[k], full[k][pix]), (P, first, run, k)
        assert sorted(seen) == list(range(H))


def test_explicit_rays(hip):
    spec = scenes.readme_spec(W, H)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    kw = dict(side=2, light_radius=1.0)
    full = r.render_occlusion(scene, **kw)
    D = r.get_ray_directions(scene.camera).data
    n = W * H
    cam = [float(c) for c in spec["camera"]["position"]]
    per_ray = torch.tensor(cam, dtype=torch.float64, device=D.device)[:, None].expand(3, n).contiguous()
    for origin in (per_ray, scene.camera.position):  # stride n and stride 0
        got = r.trace_occlusion(origin, D, scene, **kw)
        assert tuple(got) == R.PASSES
        for k in R.PASSES:
            assert torch.equal(got[k], full[k]), k
    # per-ray origins that differ: every ray starts a little off the camera, towards its pixel
    moved = per_ray + D * 0.125
    got = r.trace_occlusion(moved, D, scene, **kw)
    a = {k: v.cpu().numpy() for k, v in r.trace_aovs(moved, D, scene, INPUTS).items()}
    ref = R.occlusion(O.scene_from_spec(spec), a["id"], a["position"], a["normal"], **kw)
    for k in R.PASSES:
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    assert partial(ref["ao"]) >= 300


def test_a_pinhole_perspective_camera(hip):
    o = _check(hip, PINHOLE(), "pinhole", side=2, light_radius=2.0)  # (629 hits, 153 and 283 on the restatement)
    assert int((o["id"] >= 0).sum()) >= 600 and partial(o["ao"]) >= 100 and partial(o["soft_lit"]) >= 200


def test_one_pass_alone_equals_it_among_both(hip):
    spec = scenes.main_spec(W, H)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    kw = dict(side=3, light_radius=1.0)
    both = r.render_occlusion(scene, **kw)
    assert tuple(both) == R.PASSES
    for name in R.PASSES:
        for passes in (name, (name,), [name]):
            got = r.render_occlusion(scene, passes=passes, **kw)
            assert tuple(got) == (name,) and torch.equal(got[name], both[name]), name
    assert tuple(r.render_occlusion(scene, passes=("soft_lit", "ao"), **kw)) == R.PASSES
    # through the entry point: the buffer of the pass not requested is untouched
    lib, L = hip._lib.load(), hip._lib
    blob, S = r.scene_blob(scene)
    a = r.render_aovs(scene, INPUTS)
    n = W * H
    table = torch.from_numpy(occlusion.hemisphere_table(3)).cuda()
    rot = torch.from_numpy(occlusion.rotation_table()).cuda()
    for name in R.PASSES:
        bufs = {k: torch.full((n,), -7.0, dtype=torch.float32, device="cuda") for k in R.PASSES}
        ptr = {k: bufs[k].data_ptr() if k == name else None for k in R.PASSES}
        L.check(lib.rtx_occlusion(blob.data_ptr(), S, a["id"].data_ptr(), a["position"].data_ptr(),
                                  a["normal"].data_ptr(), n, table.data_ptr(), 3, rot.data_ptr(), 1e39, 1.0,
                                  ptr["ao"], ptr["soft_lit"], L.stream_handle()), "rtx_occlusion")
        torch.cuda.synchronize()
        other = R.PASSES[1 - R.PASSES.index(name)]
        assert torch.equal(bufs[name], both[name]) and bool((bufs[other] == -7.0).all()), name


@pytest.mark.parametrize("key", ["readme", "main", "rand16", "fuzz15"])
def test_a_point_light_gives_the_lit_pass(hip, key):
    make = {"readme": lambda: scenes.readme_spec(W, H), "main": lambda: scenes.main_spec(W, H)}.get(key) or SCENES[key][0]
    scene = scenes.build_scene(make())
    r = hip.HipRenderer(3)
    soft = r.render_occlusion(scene, passes="soft_lit", side=2, light_radius=0.0)["soft_lit"]
    lit = r.render_aovs(scene, "lit")["lit"]
    assert torch.equal(soft, lit.to(torch.float32))
    assert 0 < int(lit.sum()) and set(np.unique(soft.cpu().numpy()).tolist()) <= {0.0, 1.0}


def test_the_op_equals_the_renderer_and_foreign_ids_miss(hip):
    import python_ray_tracer_amd.ops  # noqa: F401

    L = hip._lib
    spec = scenes.main_spec(W, H)
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(3)
    blob, S = r.scene_blob(scene)
    a = r.render_aovs(scene, INPUTS)
    table = torch.from_numpy(occlusion.hemisphere_table(3)).cuda()
    rot = torch.from_numpy(occlusion.rotation_table()).cuda()
    want = r.render_occlusion(scene, side=3, max_distance=2.0, light_radius=1.0)
    for mask, names in ((3, R.PASSES), (1, ("ao",)), (2, ("soft_lit",))):
        got = torch.ops.rt.occlusion(blob, S, a["id"], a["position"], a["normal"], table, rot, 2.0, 1.0, mask)
        assert len(got) == len(names)
        for t, k in zip(got, names):
            assert torch.equal(t, want[k]), (mask, k)
    # a caller-made id: S, S + 7 and -5 are misses, whatever position and normal hold
    ident = a["id"].clone()
    hit = torch.nonzero(ident >= 0).view(-1)
    assert hit.numel() >= 300
    for j, v in enumerate((S, S + 7, -5)):
        ident[hit[j::3]] = v
    assert not bool(((ident >= 0) & (ident < S)).any())
    ao, soft = torch.ops.rt.occlusion(blob, S, ident, a["position"], a["normal"], table, rot, 1e39, 1.0, L.OCC_ALL)
    assert bool((ao == 1).all()) and not bool(soft.any())
    # a blob whose sphere count disagrees with n_spheres: every ray a miss (check=False: no host check)
    ao, soft = torch.ops.rt.occlusion(blob, S + 1 if S < 3 else S - 1, a["id"], a["position"], a["normal"], table, rot,
                                      1e39, 1.0, L.OCC_ALL, False)
    assert bool((ao == 1).all()) and not bool(soft.any())
    with pytest.raises(RuntimeError, match="n_spheres"):
        torch.ops.rt.occlusion(blob, S - 1, a["id"], a["position"], a["normal"], table, rot, 1e39, 1.0, L.OCC_ALL)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.rt.occlusion(blob, S, a["id"], a["position"].t().contiguous().t(), a["normal"], table, rot, 1e39, 1.0, 3)


def test_refusals(hip):
    from python_ray_tracer_amd.domain import PerspectiveCamera, Scene3D

    scene = scenes.build_scene(scenes.readme_spec(W, H))
    r = hip.HipRenderer(3)
    D = r.get_ray_directions(scene.camera).data
    for call in (lambda **kw: r.render_occlusion(scene, **kw),
                 lambda **kw: r.trace_occlusion(scene.camera.position, D, scene, **kw)):
        for bad in (("ao", "lit"), (), "shadow"):
            with pytest.raises(ValueError, match="passes"):
                call(passes=bad)
        for bad in (0, 9, 2.5, None):
            with pytest.raises(ValueError, match="side"):
                call(side=bad)
        for bad in (0.0, -1.0, 2e39, float("nan")):
            with pytest.raises(ValueError, match="max_distance"):
                call(max_distance=bad)
        for bad in (-0.5, float("inf"), float("nan"), None):
            with pytest.raises(ValueError, match="light_radius"):
                call(light_radius=bad)
    k2 = hip.HipRenderer(3, samples=2)
    with pytest.raises(ValueError, match="samples=2"):
        k2.render_occlusion(scene)
    with pytest.raises(ValueError, match="samples=2"):
        k2.trace_occlusion(scene.camera.position, D, scene)
    cam = PerspectiveCamera(Vector3D(2.5, 1.5, -1.5), W, H, Vector3D(0, 0.3, 3), lens_radius=0.05)
    with pytest.raises(ValueError, match="lens_radius"):
        r.render_occlusion(Scene3D(scene.shapes, scene.lights, cam))
