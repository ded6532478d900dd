"""The small-scene kernels' optimistic body, guard verdict and start-up (rtx_device.h: small_wave).

The counter-free capped builds of scenes below 8 spheres render a camera tile of a tame scene through
range-checked helpers that take their exact fast core unconditionally and only flag a lane outside
the core's range; a wave with a flagged lane renders its tile again through the guarded helpers.
Every TP 0 wave also holds its share of the sphere table in registers until its level-0 search has
found a hit. Neither may change a bit of a frame, so every case renders its scene five ways — a
``learn_tile_order=False`` renderer (counter-free, optimistic), a ``collect_stats=True`` one (the
STATS build: guarded only) and three renders of a default renderer (recording, then counter-free
with the learnt order) — requires the five frames bit-identical, and the plain one within 1e-12 of
the oracle with identical uint8.

Which guard a case trips is established on the CPU, from the oracle's own rays (``guard_trips``):
the level-0 operands of every guard that became a sticky flag. The guards and their cases:

* ``sph_test``, |h| >= 2^-350: test_guard_trips_in_a_camera_frame (h = 0 in the centre column).
* ``inv_mag`` in ``camera_dir``, |v|^2 in [2^-600, 2^600]: test_camera_in_the_image_plane (v = 0).
* ``inv_mag`` in ``shade`` (the light vector): test_light_at_a_hit_point (L = 0).
* ``inv_mag_unit`` in ``reflect_dir`` and ``specular``, | |v|^2 - 1 | <= 2^-30:
  test_far_sphere_reflection_is_not_unit (a sphere a million radii away: its hit point, hence its
  normal, carries the rounding of t, and the "reflected" direction is far from unit).
* ``sin_ref``, |phase| <= 2^20 unless the host bounded every phase: test_thin_film_phase_out_of_range.
* ``sqrt_cr`` and ``div_cr`` carry ballots too, but the optimistic body never calls them: they serve
  the guarded expansions of the helpers above (isect_sol's full-b form, inv_mag's fallback) only.
"""

import copy

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from tests.specs import fuzz_spec

pytestmark = pytest.mark.gpu

ATOL = 1e-12
TW, TH = 16, 4  # the small kernels' wave tile (kWaveWSmall x 64 / kWaveWSmall)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H

    return H


def c1_spec(width, height, position=(0, 0.2, -2)):
    spec, _ = scenes.CONFIGS["C1"]()
    return scenes.with_camera(spec, position=list(position), width=width, height=height)


def level0(osc):
    """The oracle's camera rays and their nearest hits: directions, hit sphere (-1: none), distance."""
    d = O.ray_directions(osc.cam, osc.width, osc.height)
    ts = np.stack([O.intersect(sp, *osc.cam, *d) for sp in osc.spheres])
    t = ts.min(axis=0)
    return d, np.where(t < O.FARAWAY, ts.argmin(axis=0), -1), t


def guard_trips(osc, thickness=None):
    """Pixels whose level-0 operands leave a fast core's exact range, per guard (the expressions of
    rtx_device.h's camera_dir, isect_disc_cam, shade, reflect_dir and hit_color, from oracle rays)."""
    W, H = osc.width, osc.height
    cam = osc.cam
    aspect = float(W) / H
    x = np.tile(np.linspace(-1, 1, W), H) - cam[0]
    y = np.repeat(np.linspace(1 / aspect + 0.25, -1 / aspect + 0.25, H), W) - cam[1]
    vz = 0 - cam[2]
    v2 = ((x * x) + (y * y)) + vz * vz
    d, hit, t = level0(osc)
    half = np.zeros(W * H, dtype=bool)
    for sp in osc.spheres:
        half |= np.abs(O._dot(*d, cam[0] - sp.cx, cam[1] - sp.cy, cam[2] - sp.cz)) < 2.0**-350
    light = np.zeros(W * H, dtype=bool)
    unit = np.zeros(W * H, dtype=bool)
    phase = np.zeros(W * H, dtype=bool)
    p = [cam[k] + d[k] * t for k in range(3)]
    for si, sp in enumerate(osc.spheres):
        m = hit == si
        l2 = sum((osc.light_pos[k] - p[k]) ** 2 for k in range(3))
        light |= m & ~((l2 >= 2.0**-600) & (l2 <= 2.0**600))
        inv_r = 1.0 / sp.radius
        n = [(p[0] - sp.cx) * inv_r, (p[1] - sp.cy) * inv_r, (p[2] - sp.cz) * inv_r]
        dn = O._dot(*d, *n)
        r = [d[k] - (n[k] * 2.0) * dn for k in range(3)]
        unit |= m & ~(np.abs(O._dot(*r, *r) - 1.0) <= 2.0**-30)
        if thickness is not None and si in thickness:
            va = np.clip(-O._dot(*d, *n), 0, 1)  # V = -D at level 0
            phase |= m & (np.abs(((np.abs(va - 0.5) * 2.0) * np.pi) * thickness[si] * 10.0) > 2.0**20)
    return {"camera": int((~((v2 >= 2.0**-600) & (v2 <= 2.0**600))).sum()), "half": int(half.sum()),
            "light": int(light.sum()), "unit": int(unit.sum()), "phase": int(phase.sum())}


def five_ways(H, spec, cap, edit=None):
    """The module docstring's five renders of ``spec`` at bounce cap ``cap``: the plain frame and the
    oracle's. ``edit(scene)`` changes the built scene first (the oracle then reads the objects)."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    scene = scenes.build_scene(spec)
    if edit is None:
        osc = O.scene_from_spec(spec)
    else:
        edit(scene)
        osc = O.scene_from_objects(scene)
    W, Hh, S = osc.width, osc.height, len(osc.spheres)
    want = O.render(osc, cap)
    label = (S, W, Hh, cap)

    plain = H.HipRenderer(cap, learn_tile_order=False)
    f_plain = plain.render_tile(scene).cpu().numpy()
    recs, _ = L.last_launches()
    # the build under test: counter-free, capped, no culling tree, the sphere count compiled in
    assert [(k.TP, k.STATS, k.IMG, k.DEEP, k.B, k.NSPH, k.tile_order) for k in recs] == [(0, 0, 0, 0, cap, S, 0)], recs
    counting = H.HipRenderer(cap, collect_stats=True)
    f_count = counting.render_tile(scene).cpu().numpy()
    assert all(k.STATS == 1 and k.TP == 0 for k in L.last_launches()[0])
    r = H.HipRenderer(cap)
    thrice = [r.render_tile(scene).cpu().numpy() for _ in range(3)]
    for k, f in enumerate([f_count, *thrice]):
        assert np.array_equal(f, f_plain), (label, "frame", k, float(np.abs(f - f_plain).max()))
    err = float(np.abs(f_plain - want).max())
    assert err <= ATOL, (label, err)
    assert np.array_equal(O.to_uint8(f_plain, W, Hh), O.to_uint8(want, W, Hh)), label
    return f_plain, want


# ---------------------------------------------------------------------------------------------
# 1. a guard that trips in a camera frame
# ---------------------------------------------------------------------------------------------

def right_angle_spec(width, height):
    """C1 with a unit sphere whose centre lies in the plane through the camera at right angles to the
    centre column of an odd-width frame: D.(O - C) = 0 exactly in that column."""
    spec = c1_spec(width, height)
    spec["spheres"].insert(0, dict(copy.deepcopy(spec["spheres"][0]), center=[3.0, 0.2, -2.0], radius=1.0))
    return spec


@pytest.mark.parametrize("cap", [0, 3])
def test_guard_trips_in_a_camera_frame(hip, cap):
    """49 x 13 (no multiple of the 16 x 4 wave tile either way: edge tiles with inactive lanes): the
    13 pixels of the centre column have |h| < 2^-350 for the added sphere, so the four waves holding
    them discard their optimistic pass and render again, guarded."""
    spec = right_angle_spec(49, 13)
    trips = guard_trips(O.scene_from_spec(spec))
    assert trips["half"] == 13 and trips["camera"] == trips["light"] == 0, trips
    assert guard_trips(O.scene_from_spec(right_angle_spec(17, 5)))["half"] == 5
    five_ways(hip, spec, cap)


# ---------------------------------------------------------------------------------------------
# 2. no guard trips; every sphere count's staging code
# ---------------------------------------------------------------------------------------------

def cut_spec(n, width, height):
    """C1's scene (n = 3), or n of seven spheres: C1's two, four small ones, and the ground last
    (n = 1: the first sphere alone)."""
    spec = c1_spec(width, height)
    if n == 3:
        return spec
    proto, ground = spec["spheres"][1], spec["spheres"][-1]
    extra = [dict(copy.deepcopy(proto), center=c, radius=r) for c, r in
             (([-1.2, 0.0, 2.0], 0.5), ([1.4, -0.2, 1.2], 0.3), ([0.2, 0.9, 2.2], 0.35), ([-0.3, -0.3, 0.2], 0.2))]
    small = spec["spheres"][:2] + extra
    spec["spheres"] = small[:1] if n == 1 else small[:n - 1] + [ground]
    return spec


@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("n", [3, 1, 2, 5, 7])
def test_no_guard_trips(hip, n, cap):
    """50 x 14, the scene as it is and cut to 1, 2, 5 and 7 spheres (every NSPH copy of the table's
    staging: one to four words a lane, the last partly filled for odd counts)."""
    spec = cut_spec(n, 50, 14)
    assert len(spec["spheres"]) == n
    trips = guard_trips(O.scene_from_spec(spec))
    assert not any(trips.values()), trips
    five_ways(hip, spec, cap)


# ---------------------------------------------------------------------------------------------
# 3. sky
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 3])
def test_sky_tiles(hip, cap):
    """The camera moved (down: the rays through the upper rows of the image plane then rise above the
    spheres) so that whole wave tiles hit nothing (they end without touching the sphere table)
    while others are part sky, part hit (they stage it). All-sky tiles are exactly 0.0."""
    W, Hh = 50, 22
    spec = c1_spec(W, Hh, (0, 0.0, -2))
    osc = O.scene_from_spec(spec)
    _, hit, _ = level0(osc)
    hm = (hit >= 0).reshape(Hh, W)
    tiles = [(ty, tx, hm[ty:ty + TH, tx:tx + TW]) for ty in range(0, Hh, TH) for tx in range(0, W, TW)]
    sky = [(ty, tx) for ty, tx, b in tiles if not b.any()]
    part = [(ty, tx) for ty, tx, b in tiles if b.any() and not b.all()]
    assert len(sky) >= 3 and len(part) >= 3, (sky, part)
    assert not any(guard_trips(osc).values())
    got, want = five_ways(hip, spec, cap)
    got = got.reshape(3, Hh, W)
    for ty, tx in sky:
        assert not got[:, ty:ty + TH, tx:tx + TW].any(), (ty, tx)
    assert not want.reshape(3, Hh, W)[:, ~hm].any()


# ---------------------------------------------------------------------------------------------
# 4. what the guarded body still serves
# ---------------------------------------------------------------------------------------------

def test_untamed_scene_goes_straight_to_the_guarded_body(hip):
    """RTX_H_TAME = 0 (a sphere beyond 2^60) in a scene of six spheres: no optimistic pass."""
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P

    spec = fuzz_spec(0)
    assert len(spec["spheres"]) == 6
    spec["spheres"][0]["center"] = [3e18, 2e18, 4e19]
    spec["spheres"][0]["radius"] = 3e18
    assert P.pack_scene(scenes.build_scene(spec))[P.L.H_TAME] == 0.0
    five_ways(hip, spec, 3)


def test_explicit_rays_go_straight_to_the_guarded_body(hip):
    """raytrace_scene with hand-made per-ray origins (mode 1) on the right-angle scene's rays."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    spec = right_angle_spec(49, 13)
    osc = O.scene_from_spec(spec)
    scene = scenes.build_scene(spec)
    d = O.ray_directions(osc.cam, 49, 13)
    rng = np.random.default_rng(4)
    o = [np.full(d[0].shape, float(v)) + rng.uniform(-0.1, 0.1, d[0].shape) for v in osc.cam]
    o[0][::7] = osc.cam[0]  # some rays from the camera itself: h = 0 again in the centre column
    o[1][::7] = osc.cam[1]
    o[2][::7] = osc.cam[2]
    r = hip.HipRenderer(3)
    got = r.raytrace_scene(hip.HipVector3D(*o), hip.HipVector3D(*d), scene).data.cpu().numpy()
    recs, _ = L.last_launches()
    assert recs and recs[0].TP == 0 and recs[0].DEEP == 0, recs
    want = np.stack(O.trace(osc, tuple(o), d, 3))
    assert float(np.abs(got - want).max()) <= ATOL


# ---------------------------------------------------------------------------------------------
# 5. each remaining guard
# ---------------------------------------------------------------------------------------------

def test_camera_in_the_image_plane(hip):
    """camera_dir's inv_mag: a camera at z = 0 on the centre pixel of a 5 x 5 frame (linspace(-1, 1, 5)
    and linspace(1.25, -0.75, 5) are exact) has v = (0, 0, 0) there; the reference's zero guard makes
    that direction (0, 0, 0)."""
    spec = c1_spec(5, 5, (0, 0.25, 0.0))
    trips = guard_trips(O.scene_from_spec(spec))
    assert trips["camera"] == 1, trips
    five_ways(hip, spec, 3)


def test_light_at_a_hit_point(hip):
    """shade's inv_mag: the light placed on a camera ray's hit point, bit for bit (the hit point does
    not depend on the light), so that pixel's light vector is (0, 0, 0)."""
    spec = c1_spec(49, 13)
    osc = O.scene_from_spec(spec)
    d, hit, t = level0(osc)
    pix = int(np.flatnonzero(hit == 1)[0])
    spec["lights"][0]["position"] = [float(osc.cam[k] + d[k][pix] * t[pix]) for k in range(3)]
    trips = guard_trips(O.scene_from_spec(spec))
    assert trips["light"] == 1 and trips["half"] == trips["camera"] == 0, trips
    five_ways(hip, spec, 3)


def test_far_sphere_reflection_is_not_unit(hip):
    """reflect_dir's inv_mag_unit: a sphere of radius 0.5 a million units down the centre pixel's
    ray, a little off it. The root's rounding (an ulp of 10^6) is a large part of the radius, so the
    normal (P - C) / r is not unit and neither is D - 2 (D.N) N; the reference normalises it all the
    same."""
    W, Hh = 17, 5
    spec = c1_spec(W, Hh)
    cam = spec["camera"]["position"]
    d = O.ray_directions(tuple(cam), W, Hh)
    c = (Hh // 2) * W + W // 2
    far = dict(copy.deepcopy(spec["spheres"][0]), radius=0.5,
               center=[float(cam[0] + d[0][c] * 1e6 + 0.3), float(cam[1] + d[1][c] * 1e6 + 0.2), float(cam[2] + d[2][c] * 1e6)])
    spec["spheres"] = [far, spec["spheres"][-1]]
    trips = guard_trips(O.scene_from_spec(spec))
    assert trips["unit"] >= 1 and trips["half"] == trips["camera"] == trips["light"] == 0, trips
    five_ways(hip, spec, 3)


def test_thin_film_phase_out_of_range(hip):
    """sin_ref: thin-film thicknesses whose phases pass 2^20 (RTX_H_SINRED = 0)."""
    from python_ray_tracer_amd.infrastructure.hip import scene_pack as P

    thickness = {0: 4e4, 1: -1e5}

    def edit(scene):
        for si, v in thickness.items():
            scene.shapes[si].shader.thin_film_thickness = v

    spec = c1_spec(50, 14)
    probe = scenes.build_scene(spec)
    edit(probe)
    assert P.pack_scene(probe)[P.L.H_SINRED] == 0.0
    trips = guard_trips(O.scene_from_objects(probe), thickness)
    assert trips["phase"] > 0, trips
    five_ways(hip, spec, 3, edit=edit)
