"""GPU parity of the counter-free kernel builds, checked by the launch record.

k_render_fast is one function compiled into a family of kernels (template arguments B 0..6, LDS,
DEEP 0/1/2, STATS, TP 0/1/2, IMG, NSPH 0..7, WAVES 0/6), each with its own launch bounds, register
allocation and spills. The builds the README's numbers and bench.py time are the counter-free ones
(STATS = false), but a fresh HipRenderer's first render of a key is a recording launch, which runs
the STATS build (launch_fast_b: a stats buffer or a tile_cost record), as does every
collect_stats=True render. Every case here therefore renders five frames — a counting render, a
plain one (learn_tile_order=False: counter-free from the first launch) and three on a default
renderer (recording, then counter-free with the learnt order and the decided general-kernel flag) —
asks the library which instantiation each launch ran (rtx_last_launches), compares the plain frame
with the oracle (colour within 1e-12, uint8 identical, every pixel) and requires all five to be
bit-identical: the counting and counter-free builds share their source and are built with
-ffp-contract=off. After every render the workspace's counter prefix must be zero again
(rtx_hip.h: no per-call memset; the persistent launch's last user of a fetch counter resets it).

The module ends with the dispatch-coverage test: every counter-free instantiation launch_fast_b,
launch_fast_lds and rtx_launch_small can select for a scene without image textures must have been
rendered, and compared, by the cases above.
"""

import ctypes

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from tests.specs import HUGE_LAYOUTS, fuzz_cap, fuzz_spec, huge_tail_spec, trapped_spec

pytestmark = pytest.mark.gpu

ATOL = 1e-12

# counter-free, texture-free k_render_fast records of renders that passed their comparison:
# (B, LDS, DEEP, TP, NSPH > 0, WAVES), and the small unit's (B, DEEP, NSPH)
SEEN: set = set()
SEEN_SMALL: set = set()
RAN: set = set()  # the case groups that ran (the coverage test needs all of them)
GROUPS = ("tp0", "tp1", "tp2_lds", "tp2_global", "deep_resume", "six_waves")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H

    return H


def _L():
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    return L


def _note(recs):
    for k in recs:
        if not k.STATS and not k.IMG:
            SEEN.add((k.B, k.LDS, k.DEEP, k.TP, k.NSPH > 0, k.WAVES))
            if k.TP == 0:
                SEEN_SMALL.add((k.B, k.DEEP, k.NSPH))


def _clean(ws, label, status=0):
    """The workspace's counter prefix after a call: all zero but the sticky status word."""
    L = _L()
    words = ws[:L.WS_COUNTER_BYTES].view(torch.int32).cpu().numpy()
    assert int(words[1]) == status, (label, int(words[1]))
    words[1] = 0
    assert not words.any(), (label, np.flatnonzero(words).tolist())


def _render(r, scene, label):
    """One whole-frame render: (frame on the host, launch records, general kernel launched)."""
    L = _L()
    frame = r.render_tile(scene)
    recs, general = L.last_launches()  # host state of this thread's latest render call
    torch.cuda.synchronize()
    _clean(r._ws, label)
    assert recs and general in (0, 1), (label, recs, general)
    return frame.cpu().numpy(), recs, general


class Builds:
    """What check_builds saw: the oracle's counters, the counting renderer, and per render the launch
    records and whether the general kernel ran (counting, plain, default x 3)."""


def check_builds(H, spec, cap, edit=None):
    """The five renders of ``spec`` at bounce cap ``cap`` described in the module docstring.
    ``edit(scene)`` changes the built scene first (the oracle then reads the objects)."""
    L = _L()
    scene = scenes.build_scene(spec)
    if edit is None:
        osc = O.scene_from_spec(spec)
    else:
        edit(scene)
        osc = O.scene_from_objects(scene)
    W, Hh = int(scene.camera.width), int(scene.camera.height)
    res = Builds()
    res.scene, res.st = scene, O.TraceStats()
    want = O.render(osc, cap, stats=res.st)
    assert np.isfinite(want).all()
    label = (len(scene.shapes), W, Hh, cap)

    res.counting = H.HipRenderer(cap, collect_stats=True)
    f_count, res.recs_counting, _ = _render(res.counting, scene, label)
    assert all(k.STATS == 1 for k in res.recs_counting), res.recs_counting

    plain = H.HipRenderer(cap, learn_tile_order=False)
    f_plain, res.recs_plain, res.general_plain = _render(plain, scene, label)
    for k in res.recs_plain:
        assert k.STATS == 0 and k.tile_order == 0, (label, k)
    err = float(np.abs(f_plain - want).max())
    assert err <= ATOL, (label, err)
    assert np.array_equal(O.to_uint8(f_plain, W, Hh), O.to_uint8(want, W, Hh)), label

    units = ctypes.c_int64()
    L.check(L.load().rtx_sched_tiles(W, Hh, len(scene.shapes), ctypes.byref(units)), "rtx_sched_tiles")
    many = units.value > 1  # the first render of a key records unit costs (a STATS build) and learns the order
    r = H.HipRenderer(cap)
    runs = [_render(r, scene, label) for _ in range(3)]  # (_render synchronises: probe and order have landed)
    res.recs_default = [recs for _, recs, _ in runs]
    first, third = runs[0][1][0], runs[2][1][0]
    assert first.STATS == int(many), (label, units.value, first)
    assert third.STATS == 0 and third.tile_order == int(many), (label, units.value, third)
    assert all(k.STATS == 0 for k in runs[2][1]), runs[2][1]
    (state,) = r._defers.values()  # True: the first render deferred nothing
    assert isinstance(state, bool), state
    res.general_third = runs[2][2]
    assert (res.general_third == 0) == state, (label, res.general_third, state)

    for k, f in enumerate((f_plain, runs[0][0], runs[1][0], runs[2][0])):
        assert np.array_equal(f, f_count), (label, "frame", k, float(np.abs(f - f_count).max()))
    _note(res.recs_plain)
    _note(runs[1][1])
    _note(runs[2][1])
    return res


def _one(recs, **want):
    """The single record of a render call, with the given fields."""
    assert len(recs) == 1, recs
    for name, v in want.items():
        assert getattr(recs[0], name) == v, (name, v, recs[0])
    return recs[0]


# ---------------------------------------------------------------------------------------------
# the capped and uncapped builds of each launch path
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4, 5, 6, 9, None])
@pytest.mark.parametrize("n", range(7))
def test_small_unit_every_sphere_count_and_cap(hip, n, cap):
    """TP 0 (rtx_small.hip): 1..7 spheres, each a build of its own (NSPH), at every cap."""
    RAN.add("tp0")
    res = check_builds(hip, scenes.random_spec(n, n, 37, 19), cap)
    for k in res.recs_plain:
        assert (k.TP, k.LDS, k.NSPH, k.WAVES, k.n_fetch) == (0, 1, n + 1, 0, 0), k
    if cap is not None and cap <= 6:
        _one(res.recs_plain, B=cap, DEEP=0)
    else:  # the uncapped pipeline: first pass, continuation pass
        assert [(k.B, k.DEEP) for k in res.recs_plain] == [(5, 1), (5, 2)], res.recs_plain


@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4, 5, 6, 7, 12, None])
def test_culled_one_tile_builds(hip, cap):
    """TP 1: 17 spheres, a culling tree, one block tile per block."""
    RAN.add("tp1")
    res = check_builds(hip, scenes.random_spec(16, 3, 75, 41), cap)
    for k in res.recs_plain:
        assert (k.TP, k.LDS, k.NSPH, k.WAVES, k.n_fetch) == (1, 1, 0, 0, 0), k
    if cap is not None and cap <= 6:
        _one(res.recs_plain, B=cap, DEEP=0)
    else:
        assert [(k.B, k.DEEP) for k in res.recs_plain] == [(5, 1), (5, 2)], res.recs_plain


@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4, 5, 6, 7, None])
def test_persistent_builds_lds(hip, cap):
    """TP 2 with the table in LDS: 41 spheres, persistent waves fetching wave tiles (the
    continuation pass of an uncapped render is never persistent: its TP 1, DEEP 2 build)."""
    RAN.add("tp2_lds")
    res = check_builds(hip, scenes.random_spec(40, 7, 75, 41), cap)
    k = res.recs_plain[0]
    assert (k.TP, k.LDS, k.NSPH, k.WAVES) == (2, 1, 0, 0) and k.n_fetch > 0, k
    if cap is not None and cap <= 6:
        _one(res.recs_plain, B=cap, DEEP=0)
    else:
        assert [(k.B, k.DEEP, k.TP, k.n_fetch > 0) for k in res.recs_plain] == [(5, 1, 2, True), (5, 2, 1, False)]


# (the issue's caps are 0, 3, 6 and None; 1, 2, 4 and 5 are added so that the coverage test's list
# holds every capped LDS = false build)
@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4, 5, 6, None])
def test_persistent_builds_table_in_global_memory(hip, cap):
    """TP 2 with LDS = false: 151 spheres, more than the LDS table holds."""
    RAN.add("tp2_global")
    res = check_builds(hip, scenes.random_spec(150, 7, 56, 32), cap)
    for k in res.recs_plain:
        assert (k.TP, k.LDS, k.NSPH, k.WAVES, k.lds_bytes) == (2, 0, 0, 0, 0), k
    if cap is not None:
        _one(res.recs_plain, B=cap, DEEP=0)
    else:
        assert [(k.B, k.DEEP, k.n_fetch > 0) for k in res.recs_plain] == [(5, 1, True), (5, 2, False)]


# ---------------------------------------------------------------------------------------------
# scene features that only the counting builds had rendered
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(22))
def test_fuzz_scenes(hip, seed):
    """The fuzz scenes of test_gpu_parity (camera inside a sphere, 0-2 domes, huge spheres), each at
    the cap it is rendered with there."""
    check_builds(hip, fuzz_spec(seed), fuzz_cap(seed))


@pytest.mark.parametrize("seed", [0, 3, 5])
def test_untamed_scenes(hip, seed):
    """RTX_H_TAME = 0 (a sphere beyond 2^60): the reference's sphere-test expressions everywhere."""
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P

    spec = fuzz_spec(seed)
    spec["spheres"][0]["center"] = [3e18, 2e18, 4e19]
    spec["spheres"][0]["radius"] = 3e18
    assert P.pack_scene(scenes.build_scene(spec))[P.L.H_TAME] == 0.0
    check_builds(hip, spec, 3)


def test_right_angle_fallback(hip):
    """A sphere centred on the camera: every wave's half-b test falls back at level 0."""
    spec = scenes.readme_spec(64, 36)
    spec["spheres"].insert(0, dict(spec["spheres"][0], center=list(spec["camera"]["position"]), radius=0.25))
    check_builds(hip, spec, 3)


@pytest.mark.parametrize("cap", [3, 5])
@pytest.mark.parametrize("layout", sorted(HUGE_LAYOUTS))
def test_huge_tail_layouts(hip, layout, cap):
    """RTX_H_NBEAM: huge spheres ending the scene, before, at and after sphere 64."""
    check_builds(hip, huge_tail_spec(layout, 80, 45), cap)


@pytest.mark.parametrize("cap", [2, None])
def test_ties(hip, golden_meta, cap):
    """Ties go to the general kernel: it runs on every render of this scene, the third included."""
    res = check_builds(hip, golden_meta["cases"]["ties_64x36_B2"]["spec"], cap)
    assert res.general_plain == 1 and res.general_third == 1
    assert res.counting.stats()["ties"] > 100


SINRED_SCENES = {
    "readme": lambda: scenes.readme_spec(64, 36),
    "rand16": lambda: scenes.random_spec(16, 3, 75, 41),
    "rand40": lambda: scenes.random_spec(40, 7, 75, 41),
}


@pytest.mark.parametrize("cap", [3, None])
@pytest.mark.parametrize("name", sorted(SINRED_SCENES))
def test_thin_film_phases_beyond_the_sine_reduction_range(hip, name, cap):
    """RTX_H_SINRED = 0: two materials whose thin-film phases (|phase| <= 10 pi |thickness|) fall on
    both sides of 2^20, so sin_ref's per-wave ballot sends some waves through the kernel sine's own
    reduction and others through the sin(x) fallback. Held to ATOL like every other scene (device
    sin and NumPy's are each about 1 ulp)."""
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P

    def edit(scene):
        scene.shapes[0].shader.thin_film_thickness = 4e4
        scene.shapes[1].shader.thin_film_thickness = -1e5

    probe = scenes.build_scene(SINRED_SCENES[name]())
    assert P.pack_scene(probe)[P.L.H_SINRED] == 1.0
    edit(probe)
    assert P.pack_scene(probe)[P.L.H_SINRED] == 0.0
    check_builds(hip, SINRED_SCENES[name](), cap, edit=edit)


@pytest.mark.parametrize("cap", [61, 80])
@pytest.mark.parametrize("n_outside", [9, 40, 150])
def test_deep_resumes_with_a_tree_and_without_the_lds_table(hip, n_outside, cap):
    """The trapped-ray scene (every chain runs to the cap: deferred by the first pass at level 30,
    continued to the level-60 record, finished by the general kernel) with spheres outside the trap
    that are never hit but give the scene a culling tree (10 spheres: TP 1; 41: the persistent first
    pass; 151: the table in global memory and the general kernel's tree walk, kGeneralTreeMin = 32,
    resuming a record)."""
    RAN.add("deep_resume")
    L = _L()
    spec = trapped_spec(24, 16, n_outside)
    st = O.TraceStats()
    O.render(O.scene_from_spec(spec), cap, stats=st)
    assert len(st.rays) == cap + 1 and st.rays[31] == st.rays[61] == 24 * 16  # the oracle alone
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P

    assert P.pack_scene(scenes.build_scene(spec))[P.L.H_NNODES] > 0  # a culling tree
    res = check_builds(hip, spec, cap)
    s = res.counting.stats()
    n = min(len(st.rays), L.S_LEVELS)
    assert s["rays"][:n] == st.rays[:n] and s["hits"][:n] == st.hits[:n]
    for recs, general in ((res.recs_plain, res.general_plain), (res.recs_default[2], res.general_third)):
        assert [(k.B, k.DEEP) for k in recs] == [(5, 1), (5, 2)] and general == 1, (recs, general)
        lds = 0 if n_outside + 1 > 128 else 1
        assert all(k.LDS == lds for k in recs), recs
        assert recs[0].TP == (1 if n_outside + 1 < 32 else 2), recs


# ---------------------------------------------------------------------------------------------
# the 6-wave build at its threshold
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def orbit8():
    base = scenes.random_spec(16, 0, 1024, 512)
    specs = [scenes.with_camera(base, scenes.orbit_position(k, 8)) for k in range(8)]
    return specs, [scenes.build_scene(sp) for sp in specs]


@pytest.mark.parametrize("cap", range(7))
def test_six_wave_build_at_its_threshold(hip, orbit8, cap):
    """Launches of kWavesLargeMinPixels (4 Mi) pixels and more of the one-tile culled kernel run its
    build for 6 waves/SIMD (kFwdWavesLarge; it spills). Eight 1024x512 frames in one launch are
    exactly 4 Mi pixels, seven are below: every frame of both batches equals its single-frame render
    (the 5-wave build) bit for bit, and frame 3 the oracle."""
    RAN.add("six_waves")
    L = _L()
    specs, frames = orbit8
    assert 8 * 1024 * 512 == 4 << 20
    r = hip.HipRenderer(cap)
    b8 = r.render_batch(frames)
    rec8 = _one(L.last_launches()[0], B=cap, WAVES=6, TP=1, STATS=0, DEEP=0, LDS=1, grid_z=8)
    b7 = r.render_batch(frames[:7])
    rec7 = _one(L.last_launches()[0], B=cap, WAVES=0, TP=1, STATS=0, DEEP=0, LDS=1, grid_z=7)
    torch.cuda.synchronize()
    _clean(r._ws, ("batch", cap))
    single = hip.HipRenderer(cap, learn_tile_order=False)
    for f, sc in enumerate(frames):
        one = single.render_tile(sc)
        rec1 = _one(L.last_launches()[0], B=cap, WAVES=0, TP=1, STATS=0, tile_order=0)
        assert torch.equal(b8[f], one), (cap, f)
        assert f == 7 or torch.equal(b7[f], one), (cap, f)
    torch.cuda.synchronize()
    _clean(single._ws, ("single", cap))
    want = O.render(O.scene_from_spec(specs[3]), cap)
    got = b8[3].cpu().numpy()
    assert float(np.abs(got - want).max()) <= ATOL, (cap, float(np.abs(got - want).max()))
    assert np.array_equal(O.to_uint8(got, 1024, 512), O.to_uint8(want, 1024, 512))
    _note([rec8, rec7, rec1])


# ---------------------------------------------------------------------------------------------
# persistent fetch counters under a small grid
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(8, 8), (24, 24), (256, 8), (264, 8), (75, 41)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("reserve", [4095, 0])
def test_fetch_counters_reset_under_a_small_grid(hip, reserve, size):
    """The persistent launch hands out wave tiles from counters that their last user resets (no
    per-call memset). RTX_F_RESERVE(4095) shrinks the grid to 8 blocks (32 waves), so frames of 1, 9,
    32, 33 and 60 wave tiles have fewer tiles than waves, exactly as many, one more, and about twice
    as many. Three launches on one zero-initialised workspace (default order, the units reversed,
    default again): each equals the counting render bit for bit and leaves the counters zero."""
    L = _L()
    lib = L.load()
    W, Hh = size
    scene = scenes.build_scene(scenes.random_spec(40, 7, W, Hh))
    rs = hip.HipRenderer(3, collect_stats=True)
    ref = rs.render_tile(scene)
    assert all(k.STATS == 1 for k in L.last_launches()[0])
    blob, S = rs.scene_blob(scene)
    nbytes = int(lib.rtx_workspace_bytes(W * Hh, 3))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=rs.device)
    units = ctypes.c_int64()
    L.check(lib.rtx_sched_tiles(W, Hh, S, ctypes.byref(units)), "rtx_sched_tiles")
    tiles = ((W + 7) // 8) * ((Hh + 7) // 8)
    assert units.value == tiles
    reverse = torch.arange(tiles - 1, -1, -1, dtype=torch.int32, device=rs.device)  # a permutation of the units
    flags = (reserve & 0xFFF) << L.F_RESERVE_SHIFT
    for k, order in enumerate((None, reverse, None)):
        out = torch.full((3, W * Hh), -7.25, dtype=torch.float64, device=rs.device)
        L.check(lib.rtx_render_camera_sched(blob.data_ptr(), S, W, Hh, 1, 1, 0, 1, Hh, 3, out.data_ptr(), L.OUT_F64_SOA,
                                            ws.data_ptr(), nbytes, None, L.stream_handle(), flags, None,
                                            None if order is None else order.data_ptr(), None),
                "rtx_render_camera_sched")
        rec = _one(L.last_launches()[0], B=3, TP=2, LDS=1, STATS=0, DEEP=0, tile_order=int(order is not None))
        torch.cuda.synchronize()
        print(f"{W}x{Hh} reserve {reserve} launch {k}: {tiles} tiles, grid_x {rec.grid_x}, n_fetch {rec.n_fetch}")
        assert torch.equal(out, ref), (size, reserve, k)
        _clean(ws, (size, reserve, k))
        assert 1 <= rec.n_fetch <= 32 and (rec.grid_x * 4) % rec.n_fetch == 0, rec
        if reserve:
            assert rec.grid_x <= 8, rec
            if tiles == 60:
                assert rec.grid_x * 4 < tiles, rec  # the dynamic fetch really ran
        _note([rec])


def test_fetch_counters_of_a_full_grid(hip):
    """An unreserved persistent launch with more wave tiles than the device holds waves (640x480:
    4,800 tiles): the dynamic fetch on a full grid."""
    res = check_builds(hip, scenes.random_spec(40, 7, 640, 480), 5)
    rec = _one(res.recs_plain, B=5, TP=2, LDS=1)
    print(f"640x480: 4800 tiles, grid_x {rec.grid_x}, n_fetch {rec.n_fetch}")
    assert rec.grid_x * 4 < 4800, rec


# ---------------------------------------------------------------------------------------------
# RTX_F_NO_GENERAL on a render that does defer
# ---------------------------------------------------------------------------------------------

SENTINEL = -7.25  # no colour is negative


def _camera_ex(L, blob, S, W, Hh, cap, ws, flags, count=None):
    out = torch.full((3, W * Hh), SENTINEL, dtype=torch.float64, device=ws.device)
    rc = L.load().rtx_render_camera_ex(blob.data_ptr(), S, W, Hh, 1, 1, 0, Hh, cap, out.data_ptr(), L.OUT_F64_SOA,
                                       ws.data_ptr(), ws.numel(), None, L.stream_handle(), flags,
                                       None if count is None else count.data_ptr())
    recs, general = L.last_launches()
    torch.cuda.synchronize()
    return rc, out, recs, general


def _status(ws):
    return int(ws[:8].view(torch.int32)[1].item())


@pytest.mark.parametrize("case", ["ties_B2", "trapped_uncapped"])
def test_no_general_on_a_deferring_render(hip, golden_meta, case):
    """RTX_F_NO_GENERAL for a render that does defer rays (rtx_hip.h): the call succeeds, the deferred
    pixels stay unwritten, the sticky RTX_ST_UNRENDERED flag is raised and the workspace counters stay
    clean, so the same call without the flag on the same workspace renders the frame."""
    L = _L()
    if case == "ties_B2":
        spec, cap = golden_meta["cases"]["ties_64x36_B2"]["spec"], 2
    else:  # every chain outlives the first pass's level-30 record: every pixel is deferred
        spec, cap = trapped_spec(12, 8), L.UNBOUNDED
    W, Hh = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(2)  # (for the device blob only)
    blob, S = r.scene_blob(scene)
    nbytes = int(L.load().rtx_workspace_bytes(W * Hh, cap))
    # the normal render, on a workspace of its own
    ws0 = torch.zeros(nbytes, dtype=torch.uint8, device=r.device)
    count = torch.full((1,), -1, dtype=torch.int32, device=r.device)
    rc, normal, recs, general = _camera_ex(L, blob, S, W, Hh, cap, ws0, 0, count)
    assert rc == 0 and general == 1, (rc, general)
    status0 = _status(ws0)
    _clean(ws0, case, status0)
    if case == "ties_B2":
        assert status0 == 0
        want = O.render(O.scene_from_spec(spec), cap)
        assert float(np.abs(normal.cpu().numpy() - want).max()) <= ATOL
        deferred = int(count.item())
        assert 100 < deferred < W * Hh
    else:  # (the reference would hit Python's recursion limit; the library flags the overflow)
        assert status0 == L.ST_STACK_OVERFLOW
        deferred = W * Hh
    # the same render with the flag
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=r.device)
    rc, out, recs, general = _camera_ex(L, blob, S, W, Hh, cap, ws, L.F_NO_GENERAL)
    assert rc == 0
    assert len(recs) == 1 and general == 0, (recs, general)
    assert recs[0].STATS == 0 and recs[0].DEEP == (0 if cap >= 0 else 1), recs
    assert _status(ws) == L.ST_UNRENDERED
    _clean(ws, case, L.ST_UNRENDERED)  # every other byte of the counter prefix is zero
    unwritten = (out == SENTINEL).all(dim=0)
    assert ((out == SENTINEL).any(dim=0) == unwritten).all()  # a pixel is written whole or not at all
    assert int(unwritten.sum()) == deferred, (int(unwritten.sum()), deferred)  # the sentinel survives there
    assert torch.equal(out[:, ~unwritten], normal[:, ~unwritten])
    # after clearing the sticky flag, the same workspace renders the frame
    ws[4:8].zero_()
    rc, again, recs, general = _camera_ex(L, blob, S, W, Hh, cap, ws, 0)
    assert rc == 0 and general == 1
    assert torch.equal(again, normal)
    assert _status(ws) == status0
    _clean(ws, case, status0)


def test_renderer_raises_on_the_unrendered_flag(hip):
    """HipRenderer._check_status names RTX_ST_UNRENDERED: a renderer wrongly convinced that the
    trapped-ray scene defers nothing (its plan forced) must not return a frame of unwritten pixels."""
    from python_ray_tracer_amd.infrastructure.hip.scene_pack import scene_key

    scene = scenes.build_scene(trapped_spec(12, 8))
    r = hip.HipRenderer()
    r._defers[(scene_key(scene), 1, 1, 0, 1, None)] = True
    with pytest.raises(RuntimeError, match="RTX_ST_UNRENDERED"):
        r.render(scene)
    L = _L()
    recs, general = L.last_launches()
    assert len(recs) == 1 and recs[0].DEEP == 1 and general == 0  # the forced plan was the one used
    assert _status(r._ws) == 0  # read and cleared


# ---------------------------------------------------------------------------------------------
# dispatch coverage
# ---------------------------------------------------------------------------------------------

def test_every_counter_free_build_was_rendered():
    """Every counter-free k_render_fast instantiation the dispatch can select for a scene without
    image textures, as (B, LDS, DEEP, TP, NSPH > 0, WAVES), from the rules in rtx_hip.h and DESIGN.md:
    * below 8 spheres (rtx_launch_small): TP 0, the table in LDS, the sphere count compiled in
      (NSPH 1..7); caps 0..6 are DEEP 0 with B = cap, larger or no caps B = 5 with DEEP 1 (first
      pass) and DEEP 2 (continuation pass);
    * 8..128 spheres (launch_fast_lds): the table in LDS. One tile per block (TP 1) below 32
      spheres, for a launch of several frames, for explicit rays and for every continuation pass;
      its capped build for 6 waves/SIMD (WAVES 6) from 4 Mi pixels per launch on. Persistent
      (TP 2) for one camera frame of 32 spheres and more: capped and the first pass;
    * above 128 spheres (launch_fast_b): LDS = false, always the TP 2 build, all three DEEP modes.
    The cases of this module must have rendered all of them through records that say STATS == 0."""
    if not RAN:
        pytest.skip("collects the launch records of this module's other tests: run the whole module")
    missing_groups = [g for g in GROUPS if g not in RAN]
    if missing_groups:
        pytest.skip(f"needs this module's {missing_groups} cases in the same run")
    caps = range(7)
    want = (
        [(B, 1, 0, 0, True, 0) for B in caps] + [(5, 1, 1, 0, True, 0), (5, 1, 2, 0, True, 0)]
        + [(B, 1, 0, 1, False, 0) for B in caps] + [(B, 1, 0, 1, False, 6) for B in caps]
        + [(5, 1, 1, 1, False, 0), (5, 1, 2, 1, False, 0)]
        + [(B, 1, 0, 2, False, 0) for B in caps] + [(5, 1, 1, 2, False, 0)]
        + [(B, 0, 0, 2, False, 0) for B in caps] + [(5, 0, 1, 2, False, 0), (5, 0, 2, 2, False, 0)]
    )
    literal = [
        (0, 1, 0, 0, True, 0), (1, 1, 0, 0, True, 0), (2, 1, 0, 0, True, 0), (3, 1, 0, 0, True, 0),
        (4, 1, 0, 0, True, 0), (5, 1, 0, 0, True, 0), (6, 1, 0, 0, True, 0), (5, 1, 1, 0, True, 0),
        (5, 1, 2, 0, True, 0),
        (0, 1, 0, 1, False, 0), (1, 1, 0, 1, False, 0), (2, 1, 0, 1, False, 0), (3, 1, 0, 1, False, 0),
        (4, 1, 0, 1, False, 0), (5, 1, 0, 1, False, 0), (6, 1, 0, 1, False, 0),
        (0, 1, 0, 1, False, 6), (1, 1, 0, 1, False, 6), (2, 1, 0, 1, False, 6), (3, 1, 0, 1, False, 6),
        (4, 1, 0, 1, False, 6), (5, 1, 0, 1, False, 6), (6, 1, 0, 1, False, 6),
        (5, 1, 1, 1, False, 0), (5, 1, 2, 1, False, 0),
        (0, 1, 0, 2, False, 0), (1, 1, 0, 2, False, 0), (2, 1, 0, 2, False, 0), (3, 1, 0, 2, False, 0),
        (4, 1, 0, 2, False, 0), (5, 1, 0, 2, False, 0), (6, 1, 0, 2, False, 0), (5, 1, 1, 2, False, 0),
        (0, 0, 0, 2, False, 0), (1, 0, 0, 2, False, 0), (2, 0, 0, 2, False, 0), (3, 0, 0, 2, False, 0),
        (4, 0, 0, 2, False, 0), (5, 0, 0, 2, False, 0), (6, 0, 0, 2, False, 0), (5, 0, 1, 2, False, 0),
        (5, 0, 2, 2, False, 0),
    ]
    assert sorted(want) == sorted(literal) and len(set(literal)) == 42
    missing = sorted(set(literal) - SEEN)
    assert not missing, missing
    # nothing outside the list either: a build the rules above do not name would be one this test misses
    assert not sorted(SEEN - set(literal)), sorted(SEEN - set(literal))
    # and the small unit's builds one by one: every sphere count at every cap and in both DEEP passes
    small = {(B, 0, n) for B in caps for n in range(1, 8)} | {(5, d, n) for d in (1, 2) for n in range(1, 8)}
    assert not sorted(small - SEEN_SMALL), sorted(small - SEEN_SMALL)
