"""The limits of the lights and mesh kernels without a GPU: the cases of tests/test_gpu_mesh_limits.py and
tests/test_gpu_lights_limits.py, what each exercises, and that the restatement is a sound reference for it
(DESIGN.md §15, §17).

* ``pending_need`` of tests/mesh_ref.py and tests/lights_ref.py (the high-water mark of a lane's stack of
  pending rays) against the kernel's walk taken literally, ray by ray.
* Frames larger than the pool of workers (taken from the library, never from a constant): which rows are
  second items and what their rays do there.
* A stack of 2B + 2 entries filled to its last entry, and one over.
* Incoherent rays through a scene placed near and far from the origin, large and small; deep trees; rays
  aimed at vertices and edges; a box met from six sides with exact arithmetic.

For every case the tree's emulated pruning (mesh_ref.Pruner at leaves 1 and 4) gives the brute-force result
bit for bit, so every triangle tried for every ray is a fair reference, and no colour of a compared uint8
frame sits near a quantisation step.
"""

import copy

import numpy as np
import pytest

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes, tiling
from python_ray_tracer_amd.infrastructure.hip import _lib as L
from tests import lights_ref as LR
from tests import mesh_ref as R
from tests import meshuv_ref as U
from tests.test_glass_cpu import coincident_spec
from tests.test_lights_cpu import colored, step_distance
from tests.test_lights_cpu import pool as lights_pool
from tests.test_mesh_cpu import exact_spec, shader
from tests.test_meshuv_cpu import image, image_shader

RTOL = 1e-12  # the project's bar: |GPU - restatement| <= RTOL * max(1, |colour|)


def mesh_pool(cap):
    """The largest pool of workers rtx_trace_mesh launches at ``cap``, from the library's own workspace
    size: the workspace of a huge ray count holds one stack of 2 cap + 2 rays of 80 bytes per worker."""
    return (int(L.load().rtx_mesh_workspace_bytes(1 << 40, cap)) - L.WS_HDR_BYTES) // ((2 * cap + 2) * 80)


def table_of(spec, max_leaf=4):
    return M.mesh_table(scenes.build_scene(spec).shapes, max_leaf)


def trace_spec(spec, o, d, cap, counts=None, leaf=None, uv=False):
    """The restatement's colours float64 [3, n] of explicit rays (origins three scalars or [3, n], directions
    [3, n]) through ``spec``: tests/mesh_ref.py, or tests/meshuv_ref.py (``uv``); ``leaf``: with the pruning of
    the device table of that leaf size emulated."""
    scene = O.scene_from_spec(spec)
    prune = None if leaf is None else R.Pruner(table_of(spec, leaf))
    ref, g = (U, U.group_of(spec)) if uv else (R, R.group_of(spec))
    return np.stack(ref.trace(scene, g, R.table_of(spec), tuple(o), tuple(d), cap, counts, 0, prune))


def need_spec(spec, o, d, cap):
    """R.pending_need of explicit rays through ``spec``."""
    return R.pending_need(O.scene_from_spec(spec), R.group_of(spec), R.table_of(spec), tuple(o), tuple(d), cap)


def frame_rays(spec, rows=None):
    """(the eye, the directions [3, n]) of ``spec``'s frame, or of its rows ``rows``."""
    osc = O.scene_from_spec(spec)
    d = O.ray_directions(osc.cam, osc.width, osc.height) if rows is None else \
        O.ray_directions_rows(osc.cam, osc.width, osc.height, rows)
    return tuple(float(c) for c in osc.cam), np.stack(d)


# ---- frames larger than the pool of workers --------------------------------------------------------------------

# key -> (spec, restatement module, cap, the pool, rows compared with the restatement)
LAPS = {
    "mesh": (lambda: scenes.mesh_spec(640, 360, 1), R, 3, mesh_pool, [0, 100, 200, 300, 310, 330, 345, 359]),
    "mesh_uv": (lambda: scenes.textured_mesh_spec(640, 360, 1, scenes.uv_grid_texels(8, 8)), U, 3, mesh_pool,
                [0, 100, 200, 300, 310, 330, 345, 359]),
    "lights": (lambda: scenes.lights_spec(640, 360), LR, 3, lights_pool, [0, 100, 200, 300, 310, 330, 345, 359]),
    # the pool of the 256 MiB budget, the only stride of the stack other than 196,608; with its small sphere
    # twice (a tie on every ray that meets it) entries above the first are addressed at that stride
    "mesh_B16": (lambda: _twice(scenes.mesh_spec(448, 252, 1)), R, 16, mesh_pool, [0, 110, 219, 221, 236, 251]),
}
_laps: dict = {}


def _twice(spec):
    spec["spheres"].insert(2, copy.deepcopy(spec["spheres"][1]))
    return spec


def lap_case(key):
    """(spec, cap, the pool, the rows, the restatement's rows float64 [3, len(rows) * W]) of a frame that ends
    in the workers' second lap; computed once. Fails, never skips, when the pool was retuned."""
    if key not in _laps:
        make, ref, cap, pool_of, rows = LAPS[key]
        spec = make()
        n, p = spec["camera"]["width"] * spec["camera"]["height"], pool_of(cap)
        assert p < n < 2 * p, f"{key}: {n} rays for a pool of {p} workers: the pool was retuned: pick another frame"
        _laps[key] = (spec, cap, p, rows, ref.render(spec, cap, rows=rows))
    return _laps[key]


def second_lap_rows(key):
    """The compared rows all of whose rays are second items."""
    spec, _, p, rows, _ = lap_case(key)
    return [r for r in rows if r * spec["camera"]["width"] >= p]


_origins: dict = {}


def origins_case():
    """The "mesh" lap frame's rays with one origin per ray, moved back along the ray by linspace(0, 0.5, n):
    (spec, cap, pool, origins [3, n], directions [3, n], the indices of three blocks of 2,048 rays (the first,
    those that straddle the pool, the last), the restatement's colours of those indices); computed once."""
    if not _origins:
        spec, cap, p = lap_case("mesh")[:3]
        cam, d = frame_rays(spec)
        n = d.shape[1]
        back = np.linspace(0.0, 0.5, n)
        o = np.stack([cam[c] - d[c] * back for c in range(3)])
        idx = np.concatenate([np.arange(2048), np.arange(p - 1024, p + 1024), np.arange(n - 2048, n)])
        _origins["case"] = (spec, cap, p, o, d, idx, trace_spec(spec, o[:, idx], d[:, idx], cap))
    return _origins["case"]


# ---- the stack filled to its last entry, and one over ----------------------------------------------------------

TIE_W = TIE_H = 17  # a square frame of dyadic pixel steps: its centre ray is (0, 0, 1) exactly
TIE_PIXEL = (TIE_H // 2) * TIE_W + TIE_W // 2  # lane 16 of the third wave
TIE_LANES = (0, 31, 63, 101)  # where the explicit ray sets carry the tie ray as well: two waves, both ends of one


def tie_spec(k, uv=False):
    """The exact "tie" case of tests/test_mesh_cpu.py::exact_cases as a 17 x 17 frame, raised by 0.25 so that
    the frame's centre ray is the tie ray: ``k`` coincident copies of its sphere and its triangle at t = 4
    exactly, so that ray's k + 1 hits push one ray each at B = 1 into a stack of 4. A sphere behind the eye
    stands where the reflected rays of those hits go: a dropped one changes the colour."""
    sph = [{"center": [0, 0.25, 3], "radius": 1.0, "shader": shader((1.0 - 0.2 * j, 0.5, 0.25 + 0.2 * j))} for j in range(k)]
    sph.append({"center": [0, 0.25, -6], "radius": 1.0, "shader": shader((0.3, 0.9, 0.4))})
    tri = {"kind": "triangles", "vertices": [[-1, -0.75, 2], [1, -0.75, 2], [0, 1.25, 2]], "faces": [[0, 1, 2]],
           "shader": shader((0.5, 0.25, 1.0))}
    if uv:
        tri["uvs"] = [[[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]]]
        tri["shader"] = image_shader(image(4, 4))
    spec = exact_spec([tri], sph)
    spec["camera"] = {"position": [0.0, 0.25, -2.0], "width": TIE_W, "height": TIE_H}
    return spec


_ties: dict = {}


def tie_case(k, uv=False):
    """(spec, the restatement's frame at B = 1, pending_need per pixel, the explicit rays' directions [3, n]
    (the frame's, with the tie ray at TIE_LANES too), their colours, their pending_need); computed once."""
    if (k, uv) not in _ties:
        spec = tie_spec(k, uv)
        cam, d = frame_rays(spec)
        e = d.copy()
        e[:, list(TIE_LANES)] = d[:, [TIE_PIXEL]]
        _ties[k, uv] = (spec, trace_spec(spec, cam, d, 1, uv=uv), need_spec(spec, cam, d, 1), e,
                        trace_spec(spec, cam, e, 1, uv=uv), need_spec(spec, cam, e, 1))
    return _ties[k, uv]


_light_stacks: dict = {}


def lights_stack_case(k):
    """(spec, the restatement's frame at B = 1, pending_need per pixel) of tests/test_glass_cpu.py's
    coincident_spec(k) (k coincident spheres, 32 x 18) without transmission under one ColoredPointLight."""
    if k not in _light_stacks:
        spec = colored(coincident_spec(k))
        osc = O.scene_from_spec(spec)
        cam, d = frame_rays(spec)
        _light_stacks[k] = (spec, LR.render(spec, 1), LR.pending_need(osc, LR.table_of(spec), cam, tuple(d), 1))
    return _light_stacks[k]


# ---- incoherent rays, scale and distance, deep trees, edges ----------------------------------------------------

PLACEMENTS = {  # name -> (centre c, scale s)
    "near": ((0.0, 0.0, 0.0), 1.0),
    "far1e3": ((1000.0, -2000.0, 3000.0), 1.0),
    "far1e4": ((1e4, 2e4, -3e4), 1.0),
    "big": ((0.0, 0.0, 0.0), 1e3),
    "tiny": ((0.0, 0.0, 0.0), 1e-3),
    "far_tiny": ((1000.0, -2000.0, 3000.0), 1e-2),
}
EDGE_PLACEMENTS = {**{k: PLACEMENTS[k] for k in ("far1e4", "big", "tiny")}, "near": ((0.013, 0.027, 0.0091), 1.0)}


def bar(c, s):
    """The bar of a placement. A coordinate's float64 spacing is eps |c| against a scene of size s: the
    project's known reassociations, pinned below the bar in scenes of size about |c|, are amplified by |c| / s
    (DESIGN.md §17). Derived, not measured."""
    return RTOL * max(1.0, float(np.sqrt(np.sum(np.square(c)))) / s)


def spec_of(level, c, s, smooth=True, textured=False):
    """A (smooth) icosphere of ``level`` scaled 0.5 s at c, a 16 x 8 torus scaled s beside it (``textured``:
    under a 4 x 4 image), a sphere of radius 0.35 s on the other side, a point light and a dome light."""
    c = np.asarray(c, dtype=np.float64)
    at = lambda *v: (c + np.array(v) * s).tolist()  # noqa: E731
    torus = {"kind": "torus", "R": 0.45, "r": 0.16, "nu": 16, "nv": 8, "scale": s, "translation": at(-0.9, 0.0, 0.1),
             "shader": shader((1.0, 0.6, 0.1))}
    if textured:
        torus["uv"] = True
        torus["shader"] = image_shader(image(4, 4))
    return {"spheres": [{"center": at(0.9, 0.1, 0.2), "radius": 0.35 * s, "shader": shader((1.0, 0.5, 0.25))}],
            "meshes": [{"kind": "icosphere", "level": level, "smooth": smooth, "scale": 0.5 * s, "translation": c.tolist(),
                        "shader": shader()}, torus],
            "lights": [{"kind": "point", "position": at(-2.0, 4.0, -1.0)},
                       {"kind": "dome", "intensity": 0.125, "color": [1, 1, 1]}],
            "camera": {"position": at(0.0, 0.0, -3.0), "width": 2, "height": 2}}


def _directions(rng, n):
    u = rng.normal(size=(3, n))
    return u / np.sqrt((u * u).sum(axis=0))


def random_rays(c, s, n, seed):
    """Incoherent rays: origins on random directions from c at distance s U(0.05, 4) (some inside the shapes),
    aimed at c + U(-1.2, 1.2)^3 o (1, 0.5, 0.5) s. (origins [3, n], directions [3, n])."""
    rng = np.random.default_rng(seed)
    c = np.asarray(c, dtype=np.float64).reshape(3, 1)
    o = c + _directions(rng, n) * (s * rng.uniform(0.05, 4.0, n))
    target = c + rng.uniform(-1.2, 1.2, (3, n)) * np.array([[1.0], [0.5], [0.5]]) * s
    return o, np.stack(O._norm(*(target - o)))


def edge_rays(spec, c, s, seed):
    """16 rays at every vertex of ``spec``'s first mesh and at one random point of each of its edges, from
    random origins at distance s U(1, 4) of c."""
    rng = np.random.default_rng(seed)
    v, f, _ = scenes.mesh_arrays(spec["meshes"][0])
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    lam = rng.uniform(0.0, 1.0, (e.shape[0], 1))
    target = np.repeat(np.concatenate([v, v[e[:, 0]] * (1.0 - lam) + v[e[:, 1]] * lam]), 16, axis=0).T
    n = target.shape[1]
    o = np.asarray(c, dtype=np.float64).reshape(3, 1) + _directions(rng, n) * (s * rng.uniform(1.0, 4.0, n))
    return o, np.stack(O._norm(*(target - o)))


# name -> (kind, placement, level, smooth, textured, rays, cap, seed)
RAYS = {
    **{f"random_{k}": ("random", PLACEMENTS[k], 2, True, False, 2048, 2, 11) for k in PLACEMENTS},
    "random_near_uv": ("random", PLACEMENTS["near"], 2, True, True, 2048, 2, 11),
    "deep5": ("random", PLACEMENTS["near"], 5, True, False, 512, 1, 12),
    # the benchmark's largest table (scenes.mesh_spec at level 6: 82,946 triangles), rays about its icosphere
    "deep6": ("bench", ((-1.5, -0.05, 1.75), 0.9), 6, True, False, 256, 1, 13),
    **{f"edges_{k}": ("edges", EDGE_PLACEMENTS[k], 2, False, False, 642 * 16, 1, 14) for k in EDGE_PLACEMENTS},
}
_rays: dict = {}


def ray_case(name):
    """(spec, origins [3, n], directions [3, n], cap, the restatement's colours, its counts, the bar, whether
    through meshuv_ref); computed once."""
    if name not in _rays:
        kind, (c, s), level, smooth, textured, n, cap, seed = RAYS[name]
        spec = scenes.mesh_spec(2, 2, level) if kind == "bench" else spec_of(level, c, s, smooth, textured)
        o, d = edge_rays(spec, c, s, seed) if kind == "edges" else random_rays(c, s, n, seed)
        assert d.shape == (3, n)
        counts = U.Counts() if textured else R.Counts()
        atol = RTOL if kind == "bench" else bar(c, s)  # (the benchmark's scene stands where it always stood)
        _rays[name] = (spec, o, d, cap, trace_spec(spec, o, d, cap, counts, uv=textured), counts, atol, textured)
    return _rays[name]


def box_case():
    """A box of dyadic corners met by axis-parallel rays from all six sides, every quantity exact:
    (spec, origins [3, n], directions [3, n], the group's t per ray). Every leaf box of its table is flat on
    one axis, so slab_inv's 1e-200 nudge of a zero direction component decides every slab test."""
    spec = exact_spec([{"kind": "box", "lo": [-1, -1, 1], "hi": [1, 1, 3], "shader": shader((0.5, 0.25, 1.0))}])
    F = M.FARAWAY
    rays = [  # origin, direction, t
        # through the interior of each face, from outside
        ([0.25, 0.5, -2], [-0.0, 0.0, 1.0], 3), ([0.25, -0.5, 6], [0.0, -0.0, -1.0], 3),
        ([-3, 0.25, 2.5], [1.0, 0.0, -0.0], 2), ([4, -0.25, 1.5], [-1.0, -0.0, 0.0], 3),
        ([0.5, -5, 1.5], [0.0, 1.0, 0.0], 4), ([-0.5, 2, 2.25], [-0.0, -1.0, -0.0], 1),
        # along the plane of a face (det == 0 for its triangles): the perpendicular face is met on its edge
        ([0.25, 1, -2], [0.0, 0.0, 1.0], 3), ([-1, 0.5, 6], [0.0, 0.0, -1.0], 3),
        ([-3, 0.25, 1], [1.0, 0.0, 0.0], 2), ([0.5, -5, 3], [0.0, 1.0, -0.0], 4),
        # along an edge of the box: met at its corner
        ([1, 1, -2], [0.0, 0.0, 1.0], 3), ([-1, -1, 6], [-0.0, -0.0, -1.0], 3), ([-3, 1, 3], [1.0, 0.0, 0.0], 2),
        ([1, 4, 1], [0.0, -1.0, 0.0], 3),
        # through the diagonal that splits a face (u + v == 1, or u or v == 0, on both of its triangles)
        ([0, 0, -2], [0.0, 0.0, 1.0], 3), ([-3, 0, 2], [1.0, -0.0, 0.0], 2), ([0, 5, 2], [0.0, -1.0, 0.0], 4),
        # from inside
        ([0, 0, 2], [0.0, 0.0, 1.0], 1), ([0.5, 0.25, 2], [-1.0, 0.0, 0.0], 1.5), ([0.5, 0.25, 2.5], [0.0, -1.0, -0.0], 1.25),
        ([0.25, 0.5, 1.5], [-0.0, 0.0, -1.0], 0.5),
        # past the box, and away from it
        ([2, 0, -2], [0.0, 0.0, 1.0], F), ([0, 0, 4], [0.0, 0.0, 1.0], F), ([0, -1.0000000000000002, 2], [1.0, 0.0, 0.0], F),
        # one ulp past the face x = 1: O - v0 rounds to the face (2 + 2^-52 -> 2), a hit on the triangle's edge
        ([1.0000000000000002, 0, -2], [0.0, 0.0, 1.0], 3),
    ]
    o = np.array([r[0] for r in rays], dtype=np.float64).T
    d = np.array([r[1] for r in rays], dtype=np.float64).T
    return spec, o, d, [float(r[2]) for r in rays]


# ---- pending_need ----------------------------------------------------------------------------------------------

def _walked(push_of, o, d, cap, entries=None):
    """pending_need of one ray by the kernel's walk taken literally: a stack of (origin, direction, level), pop
    one, push the rays of its hits one by one, and the high-water mark of the stack. ``entries``: a stack that
    holds so many, guarded like the kernel's (a push at sp < entries is kept, another is dropped); then
    (the high-water mark, the dropped pushes as (level of the hit, its place among the ray's pushes))."""
    one = (lambda v: np.array([v], dtype=np.float64))  # noqa: E731
    stack = [(tuple(one(c) for c in o), tuple(one(c) for c in d), 0)]
    high, dropped = 1, []
    while stack:
        oo, dd, level = stack.pop()
        if level >= cap:
            continue
        for j, (_, o2, d2) in enumerate(push_of(oo, dd)):
            if entries is not None and not len(stack) < entries:
                dropped.append((level, j))
                continue
            stack.append((o2, d2, level + 1))
            high = max(high, len(stack))
    return high if entries is None else (high, dropped)


def test_the_guarded_walk_holds_the_last_entry_and_drops_the_one_over():
    """The kernel's guard, sp < 2B + 2, in the literal walk: the tie ray of three coincident spheres fills
    the 4 entries of B = 1 and drops nothing; with four spheres exactly one push is dropped, the fifth of the
    camera ray's, which is the triangle's (the group shades after the spheres). The same for the lights
    kernel's five coincident spheres: the fifth sphere's."""
    for k, want in ((3, (4, [])), (4, (4, [(0, 4)]))):
        spec = tie_spec(k)
        osc, g, table = O.scene_from_spec(spec), R.group_of(spec), R.table_of(spec)
        cam, d = frame_rays(spec)
        assert _walked(lambda o, dr: R.pushes(osc, g, table, o, dr), cam, d[:, TIE_PIXEL], 1, 2 * 1 + 2) == want
    for k, want in ((4, (4, [])), (5, (4, [(0, 4)]))):
        spec, _, need = lights_stack_case(k)
        osc, table = O.scene_from_spec(spec), LR.table_of(spec)
        cam, d = frame_rays(spec)
        i = int(np.argmax(need))
        assert _walked(lambda o, dr: LR.pushes(osc, table, o, dr), cam, d[:, i], 1, 2 * 1 + 2) == want


def test_pending_need_is_the_walk_taken_literally():
    """The vectorised recursions against a scalar stack machine, ray by ray: the tie frames (four coincident
    spheres and a triangle, at B = 1 and 2) and every fifth ray of a mesh frame at B = 3; five coincident
    spheres under the lights kernel at B = 1 and 2."""
    for spec, cap, step in ((tie_spec(4), 1, 1), (tie_spec(2), 2, 3), (scenes.mesh_spec(32, 18, 1), 3, 5)):
        osc, g, table = O.scene_from_spec(spec), R.group_of(spec), R.table_of(spec)
        cam, d = frame_rays(spec)
        d = d[:, ::step]
        need = R.pending_need(osc, g, table, cam, tuple(d), cap)
        walked = [_walked(lambda o, dr: R.pushes(osc, g, table, o, dr), cam, d[:, i], cap) for i in range(d.shape[1])]
        assert need.tolist() == walked and max(walked) == {1: 5, 2: 3, 3: 1}[cap]  # (no tie in the mesh frame: 1)
    for cap in (1, 2):
        spec = colored(coincident_spec(5))
        osc, table = O.scene_from_spec(spec), LR.table_of(spec)
        cam, d = frame_rays(spec)
        need = LR.pending_need(osc, table, cam, tuple(d), cap)
        walked = [_walked(lambda o, dr: LR.pushes(osc, table, o, dr), cam, d[:, i], cap) for i in range(d.shape[1])]
        assert need.tolist() == walked and max(walked) == 5  # (the five-way tie of the camera rays)


def test_the_pushes_are_the_rays_the_restatement_traces():
    """``pushes`` restates the decisions of ``trace`` without the colours: level by level it sends exactly the
    rays ``trace`` counts, for the mesh and for the lights restatement."""
    def total(push_of, o, d, cap, level=0):
        n = np.asarray(d[0]).shape[0]
        if level >= cap or n == 0:
            return n
        return n + sum(total(push_of, o2, d2, cap, level + 1) for _, o2, d2 in push_of(o, d))

    for spec, cap in ((scenes.mesh_spec(32, 18, 1), 3), (tie_spec(4), 1), (spec_of(1, (0, 0, 0), 1.0), 2)):
        osc, g, table = O.scene_from_spec(spec), R.group_of(spec), R.table_of(spec)
        cam, d = frame_rays(spec) if spec["camera"]["width"] > 2 else random_rays((0, 0, 0), 1.0, 300, 5)
        c = R.Counts()
        R.trace(osc, g, table, tuple(cam), tuple(d), cap, c)
        assert total(lambda o, dr: R.pushes(osc, g, table, o, dr), tuple(cam), tuple(d), cap) == c.rays > d.shape[1]
    spec = scenes.lights_spec(32, 18)
    osc, table = O.scene_from_spec(spec), LR.table_of(spec)
    cam, d = frame_rays(spec)
    c = LR.Counts()
    LR.trace(osc, table, cam, tuple(d), 3, c)
    assert total(lambda o, dr: LR.pushes(osc, table, o, dr), cam, tuple(d), 3) == c.rays > d.shape[1]


def test_pending_need_with_k_plus_one_shapes_at_every_level_is_bk_plus_one():
    """Two and three shapes at the tie ray's nearest distance at level 0 only: k + 1 at B = 1; the stack of
    2B + 2 entries holds three ties' worth."""
    for k in (1, 2, 3, 4):
        spec = tie_spec(k)
        cam, d = frame_rays(spec)
        assert need_spec(spec, cam, d[:, [TIE_PIXEL]], 1).tolist() == [k + 1]
    assert need_spec(tie_spec(3), *frame_rays(tie_spec(3)), 0).max() == 1  # at cap 0 nothing is pushed


# ---- laps ------------------------------------------------------------------------------------------------------

def test_the_pools_come_from_the_library():
    assert mesh_pool(0) == mesh_pool(3) and mesh_pool(16) < mesh_pool(3) and mesh_pool(16) % 64 == 0
    for cap in (0, 3, 16):
        assert mesh_pool(cap) * (2 * cap + 2) * 80 + L.WS_HDR_BYTES == L.load().rtx_mesh_workspace_bytes(1 << 40, cap)


@pytest.mark.parametrize("key", sorted(LAPS))
def test_preconditions_of_the_second_lap(key):
    """Rows of both laps are compared; the second-lap rows trace reflected rays (pushed and popped by a
    worker on its second item), on triangles where the kernel has any; no colour sits near a quantisation step."""
    spec, cap, p, rows, want = lap_case(key)
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    lap2 = second_lap_rows(key)
    assert len(lap2) >= 2 and sum(r * W + W <= p for r in rows) >= 2 and W * H - p > 64 * 3 + 17
    assert want.shape == (3, len(rows) * W) and np.isfinite(want).all() and step_distance(want) > 1e-9
    assert all(W * len(tiling.tile_rows(H, 8, 4, part)) < p for part in range(4))  # the GPU test's row tiles: one lap
    ref = LAPS[key][1]
    counts = {R: R.Counts, U: U.Counts, LR: LR.Counts}[ref]()
    again = ref.render(spec, cap, rows=lap2, counts=counts)
    assert np.array_equal(again, want[:, -len(lap2) * W:]) and rows[-len(lap2):] == lap2
    print(f"{key}: pool {p}, rows {lap2} of the second lap: {counts}")
    assert counts.rays > len(lap2) * W  # reflected rays
    cam, d = frame_rays(spec, lap2)
    if ref is LR:
        need = LR.pending_need(O.scene_from_spec(spec), LR.table_of(spec), cam, tuple(d), cap)
    else:
        need = need_spec(spec, cam, d, cap)
        assert counts.tri_primary > 1000 and counts.sphere_to_tri > 0 and counts.tri_to_sphere > 0
    print(f"{key}: the walk holds up to {need.max()} pending rays of {2 * cap + 2}")
    assert (need.max() >= 3 if key == "mesh_B16" else need.max() >= 1) and need.max() <= 2 * cap + 2
    if ref is U:
        assert counts.tex_primary > 1000 and counts.tex_reflected > 0 and counts.wrapped_x + counts.wrapped_y > 0
    if key == "mesh_B16":
        assert counts.rays > 2 * len(lap2) * W  # (deep trees of reflections: levels beyond 3)


@pytest.mark.parametrize("key", ["mesh", "mesh_uv", "mesh_B16"])
def test_pruning_changes_no_row_of_the_second_lap(key):
    spec, cap, p, rows, want = lap_case(key)
    W = spec["camera"]["width"]
    some = second_lap_rows(key)[::2]
    ref = LAPS[key][1]
    for leaf in (1, 4):
        got = ref.render(spec, cap, rows=some, prune=R.Pruner(table_of(spec, leaf)))
        for k, row in enumerate(some):
            at = rows.index(row)
            assert np.array_equal(got[:, k * W:(k + 1) * W], want[:, at * W:(at + 1) * W]), (leaf, row)


def test_preconditions_of_the_per_ray_origins():
    spec, cap, p, o, d, idx, want = origins_case()
    n = d.shape[1]
    assert idx.shape == (3 * 2048,) and (idx < p).sum() == 3072 and (idx >= p).sum() == 3072 and idx.max() == n - 1
    assert np.isfinite(want).all() and step_distance(want) > 1e-9
    c = R.Counts()
    lap2 = idx[idx >= p]
    assert np.array_equal(trace_spec(spec, o[:, lap2], d[:, lap2], cap, c), want[:, idx >= p])
    print(f"per-ray origins, the {lap2.size} second items compared: {c}")
    assert c.tri_primary > 1000 and c.rays > lap2.size
    some = idx[1500::3]  # rays of every block
    for leaf in (1, 4):
        assert np.array_equal(trace_spec(spec, o[:, some], d[:, some], cap, leaf=leaf), want[:, 1500::3]), leaf


# ---- the stack -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("uv", [False, True])
def test_preconditions_of_the_mesh_stack_at_capacity(uv):
    """Three coincident spheres and the triangle fill the 4 entries of B = 1 exactly on the tie ray; a fourth
    sphere needs one more. The dropped push is the triangle's (the last hit shaded), and its ray meets the
    sphere behind the eye: without it the colour is another."""
    for k in (3, 4):
        spec, want, need, e, want_e, need_e = tie_case(k, uv)
        assert np.isfinite(want).all() and np.isfinite(want_e).all()
        assert need[TIE_PIXEL] == k + 1 == need.max() and (need == k + 1).sum() == 1 and 2 * 1 + 2 == 4
        tied = np.nonzero(need_e == k + 1)[0].tolist()
        assert tied == sorted(TIE_LANES + (TIE_PIXEL,)) and need_e.max() == k + 1
        assert len({i // 64 for i in tied}) == 3 and (need_e[:128] <= 2).sum() >= 100  # lanes that fit among them
        for i in TIE_LANES:
            assert np.array_equal(want_e[:, i], want[:, TIE_PIXEL])
        cam, d = frame_rays(spec)
        c = U.Counts() if uv else R.Counts()
        one = trace_spec(spec, cam, d[:, [TIE_PIXEL]], 1, c, uv=uv)
        print(f"k = {k}, uv = {uv}: the tie ray traces {c.rays} rays, colour {one[:, 0].tolist()}")
        assert c.rays == k + 2 and c.ties == 1 and np.array_equal(one[:, 0], want[:, TIE_PIXEL])
        if uv:
            assert c.tex_primary == 1
        assert step_distance(want) > 1e-9
        for leaf in (1, 4):
            assert np.array_equal(trace_spec(spec, cam, d, 1, leaf=leaf, uv=uv), want), leaf
        # what the overflowed lane loses: the colour without the triangle's reflected ray differs by far more than the bar
        blind = copy.deepcopy(spec)
        blind["spheres"].pop()
        lost = trace_spec(blind, cam, d[:, [TIE_PIXEL]], 1, uv=uv)
        assert np.abs(lost[:, 0] - want[:, TIE_PIXEL]).max() > 1e-3


def test_preconditions_of_the_lights_stack_at_capacity():
    for k in (4, 5):
        spec, want, need = lights_stack_case(k)
        assert len(spec["lights"]) == 2 and spec["lights"][0]["intensity"] == 1.0
        assert not any("transmission_gain" in s["shader"] for s in spec["spheres"])
        assert np.isfinite(want).all() and need.max() == k and step_distance(want) > 1e-9
        print(f"{k} coincident spheres: need {np.bincount(need).tolist()}")
    assert np.array_equal(lights_stack_case(4)[2] == 4, lights_stack_case(5)[2] == 5)
    assert (lights_stack_case(5)[2] == 5).sum() > 20 and 2 * 1 + 2 == 4
    # the clean frames rendered after an overflow
    assert step_distance(R.render(scenes.mesh_spec(32, 18, 1), 1)) > 1e-9
    assert step_distance(LR.render(scenes.lights_spec(32, 18), 1)) > 1e-9


# ---- incoherent rays, deep trees, edges ------------------------------------------------------------------------

def _prune_rays(name):
    """The rays of a case whose pruning is emulated (a table's nodes times the rays must fit in memory)."""
    n = ray_case(name)[1].shape[1]
    return np.arange(n) if RAYS[name][2] < 5 else np.arange(0, n, 4 if RAYS[name][2] == 5 else 8)


@pytest.mark.parametrize("name", sorted(RAYS))
def test_preconditions_of_the_ray_cases(name):
    spec, o, d, cap, want, c, atol, uv = ray_case(name)
    kind, (centre, s), level = RAYS[name][:3]
    n = d.shape[1]
    g = R.group_of(spec)
    print(f"{name}: {g.v0.shape[0]} triangles, bar {atol:.2e}, {c}")
    assert np.isfinite(want).all() and g.v0.shape[0] == 20 * 4 ** level + (2 + 1024 if kind == "bench" else 256)
    assert step_distance(want) > max(1e-9, 10 * atol if atol > RTOL else 0.0)
    sel = _prune_rays(name)
    for leaf in (1, 4):
        if level == 6 and leaf == 1:  # (165,891 nodes: the leaf-4 table is the benchmark's)
            continue
        assert np.array_equal(trace_spec(spec, o[:, sel], d[:, sel], cap, leaf=leaf, uv=uv), want[:, sel]), leaf
    if kind != "edges":
        assert c.tri_primary > n // 3 and c.smooth_hits > n // 8 and c.self_shadow > 0 and c.rays > n
    if kind == "random":
        assert level >= 5 or (c.sphere_to_tri > 0 and c.tri_to_sphere > 0)
        rel = (o - np.asarray(centre).reshape(3, 1)) / s
        assert (np.sqrt((rel * rel).sum(axis=0)) < 0.5 * 0.9).sum() > 0  # origins inside the icosphere
        assert (d[0] > 0.5).sum() > n // 8 and (d[0] < -0.5).sum() > n // 8  # opposite directions among a wave's rays
        if uv:
            assert c.tex_primary > 100 and c.tex_reflected > 0
    if level >= 5:  # deep trees: 14 and 16 levels of nodes at least
        nodes = int(table_of(spec)[M.MH_NNODES])
        print(f"{name}: {nodes} nodes at leaf 4")
        assert nodes == {5: 16383, 6: 65535}[level]
    if kind == "edges":
        ico = R.group_of({"meshes": spec["meshes"][:1]})
        t, num, u, v, share = R.nearest_triangle(ico, *o, *d)
        hit = t != O.FARAWAY
        on_edge = hit & ((np.abs(u) < 1e-9) | (np.abs(v) < 1e-9) | (np.abs((1.0 - u) - v) < 1e-9))
        print(f"{name}: {int(on_edge.sum())} hits within 1e-9 of an edge, {int((hit & (share > 1)).sum())} rays with two "
              f"triangles at one t, {int((~hit).sum())} rays slip between the triangles")
        assert on_edge.sum() > 1000 and (hit & (share > 1)).sum() > 50 and (~hit).sum() > 50 and c.tri_ties > 50


def test_the_placements_differ_in_nothing_but_place_and_scale():
    """The same seed gives the same rays up to the placement: the near, big and tiny cases hit the same
    shapes (powers of ten are not exact scalings, so a few decisions on edges may differ)."""
    a, b = ray_case("random_near")[5], ray_case("random_far1e3")[5]
    assert abs(a.tri_primary - b.tri_primary) <= 8
    assert bar(*PLACEMENTS["near"]) == bar(*PLACEMENTS["big"]) == bar(*PLACEMENTS["tiny"]) == RTOL
    assert [round(bar(*PLACEMENTS[k]) / RTOL) for k in ("far1e3", "far1e4", "far_tiny")] == [3742, 37417, 374166]


def test_the_box_from_six_sides_exactly():
    spec, o, d, want_t = box_case()
    g = R.group_of(spec)
    t, num, u, v, share = R.nearest_triangle(g, *o, *d)
    assert t.tolist() == want_t, t.tolist()
    assert np.signbit(d).sum() > 10 and (np.signbit(d) & (d == 0)).sum() >= 10  # -0.0 components
    assert ((d == 0).sum(axis=0) == 2).all()
    hit = t != O.FARAWAY
    assert (hit & ((u == 0) | (v == 0) | (u + v == 1))).sum() >= 10  # edges, corners and the faces' diagonals
    assert (hit & (share > 1)).sum() >= 6  # two triangles at one t: the lowest number decides
    c = R.Counts()
    col = trace_spec(spec, o, d, 3, c)
    assert np.isfinite(col).all() and np.array_equal(col.any(axis=0), hit) and c.self_shadow > 0
    for leaf in (1, 4):
        assert np.array_equal(trace_spec(spec, o, d, 3, leaf=leaf), col), leaf
    # every leaf box of the table is flat on one axis
    table = np.asarray(table_of(spec, 1))
    N = int(table[M.MH_NNODES])
    nodes = table[int(table[M.MH_NODES]):][:N * L.NODE_WORDS].reshape(N, L.NODE_WORDS)
    leaves = nodes[nodes[:, L.N_COUNT] > 0]
    flat = (leaves[:, L.N_LOX:L.N_LOZ + 1] == leaves[:, L.N_HIX:L.N_HIZ + 1]).sum(axis=1)
    assert leaves.shape[0] == 12 and (flat == 1).all()
