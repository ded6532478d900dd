"""NumPy restatement of the environment map (rtx_trace_lights_env / rtx_trace_glass_env).

The reference's ``raytrace_scene`` starts from black and adds nothing on a miss (base.py:100-121), so
there is no reference output to pin to. ``sample`` is the contract's formula of include/rtx_hip.h in
NumPy, float64 in that order. ``trace`` is ``lights_ref.trace`` (with ``glass``: ``glass_ref.trace``)
with the one new term,

    raytrace_scene(O, D):  col[c][miss] = sample(D[miss])[c]      miss: nearest == FARAWAY

at every level of the recursion. It is not a third copy of the walk: for the time of a call the
restatement's module-level ``trace`` is replaced by itself plus that term, so that its own recursive
calls (which look the name up in the module) pass through it at every level; the miss of a ray is
taken from the oracle's ``O.intersect`` like the restatement takes it. Built from the oracle's pieces
only.
"""

import copy
import inspect
from dataclasses import dataclass, field
from functools import reduce

import numpy as np

from oracle import numpy_oracle as O
from tests import glass_ref, lights_ref


@dataclass
class Env:
    """An environment as the tests state it: float32 texels (H, W, 3), gain per channel (intensity *
    colour) and the rotation in degrees."""

    texels: np.ndarray
    gain: tuple = (1.0, 1.0, 1.0)
    rotation: float = 0.0


@dataclass
class Counts:
    misses: list = field(default_factory=list)  # rays that meet no shape, by level
    transmitted_misses: int = 0  # of them, rays that left a glass ball

    def add(self, level, n):
        while len(self.misses) <= level:
            self.misses.append(0)
        self.misses[level] += n


def default_env():
    """The environment of the tests: a 16 x 8 image of uniform noise in [0, 2], gain (1, 0.9, 0.8),
    turned by 45 degrees."""
    return Env(np.random.default_rng(0).uniform(0, 2, (8, 16, 3)).astype(np.float32), (1.0, 0.9, 0.8), 45.0)




def sample(env, dirs):
    """env(D) of include/rtx_hip.h for the directions ``dirs`` (three arrays): [r, g, b] float64."""
    t = np.asarray(env.texels)[:, :, :3].astype(np.float64)  # float32 -> float64 is exact
    H, W = t.shape[:2]
    turn = env.rotation / 360.0
    dx, dy, dz = (np.atleast_1d(np.asarray(d, dtype=np.float64)) for d in dirs)
    with np.errstate(invalid="ignore"):
        u = 0.5 + np.arctan2(dz, dx) / (2 * np.pi) + turn
        u = u - np.floor(u)
        v = 0.5 - np.arcsin(np.minimum(np.maximum(dy, -1), 1)) / np.pi
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x = u * W - 0.5
    i0 = np.floor(x)
    fx = x - i0
    i1 = ((i0 + 1) % W).astype(np.int64)
    i0 = (i0 % W).astype(np.int64)
    y = v * H - 0.5
    j0 = np.floor(y)
    fy = y - j0
    j1 = np.clip(j0 + 1, 0, H - 1).astype(np.int64)
    j0 = np.clip(j0, 0, H - 1).astype(np.int64)
    out = []
    for c in range(3):
        top = t[j0, i0, c] * (1 - fx) + t[j0, i1, c] * fx
        bot = t[j1, i0, c] * (1 - fx) + t[j1, i1, c] * fx
        out.append(np.where(ok, (top * (1 - fy) + bot * fy) * float(env.gain[c]), 0.0))
    return out


def _with_miss_term(module, env, counts, state):
    """``module.trace`` plus the miss term (and the counts of the rays that miss)."""
    inner = module.trace
    sig = inspect.signature(inner)

    def trace(*args, **kw):
        a = sig.bind(*args, **kw)
        a.apply_defaults()
        transmitted, state["transmitted"] = state["transmitted"], False
        col = inner(*args, **kw)
        scene, (ox, oy, oz) = a.arguments["scene"], a.arguments["origin"]
        dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in a.arguments["dirs"])
        nearest = reduce(np.minimum, [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres])  # base.py:97-98
        miss = np.broadcast_to(nearest == O.FARAWAY, dx.shape)
        if miss.any():
            e = sample(env, (dx[miss], dy[miss], dz[miss]))
            for c in range(3):
                col[c][miss] = e[c]
        if counts is not None:
            counts.add(a.arguments["level"], int(miss.sum()))
            if transmitted:
                counts.transmitted_misses += int(miss.sum())
        return col

    return trace


def trace(scene, table, origin, dirs, max_bounces, env, counts=None, glass=None):
    """raytrace_scene under the environment ``env`` for a batch of rays. Without ``glass``:
    ``lights_ref.trace`` under the lights of ``table``. With ``glass`` = (gains, iors):
    ``glass_ref.trace`` (``table`` is not read: the glass kernel lights with ``scene.light_pos``).
    Returns [r, g, b] float64 arrays."""
    module = lights_ref if glass is None else glass_ref
    state = {"transmitted": False}
    saved = module.trace, glass_ref.through_ball
    module.trace = _with_miss_term(module, env, counts, state)
    if glass is not None:
        def through_ball(*args, **kw):  # the next ray traced after a passage is the one that leaves the ball
            c, o2, d2 = saved[1](*args, **kw)
            state["transmitted"] = bool((c < 0).any())
            return c, o2, d2
        glass_ref.through_ball = through_ball
    try:
        if glass is None:
            return module.trace(scene, table, origin, dirs, max_bounces)
        return module.trace(scene, glass[0], glass[1], origin, dirs, max_bounces)
    finally:
        module.trace, glass_ref.through_ball = saved


def plain(spec):
    """``spec`` without its environment entries: what the oracle and the other restatements read."""
    out = copy.deepcopy(spec)
    out["lights"] = [li for li in out["lights"] if li["kind"] != "environment"]
    return out


def with_env(spec, env):
    """A copy of ``spec`` with ``env`` appended to its lights as build_scene takes it."""
    out = plain(spec)
    out["lights"].append({"kind": "environment", "texels": np.asarray(env.texels), "intensity": 1.0,
                          "color": [float(g) for g in env.gain], "rotation": float(env.rotation)})
    return out


def unit_table(spec):
    """The one row (lights[0], 1, 1, 1) of a scene without a ColoredPointLight, else the spec's table."""
    pts = [li for li in spec["lights"] if li["kind"] == "point"]
    if any("intensity" in li or "color" in li for li in pts):
        return lights_ref.table_of(plain(spec))
    return np.asarray([[float(x) for x in pts[0]["position"]] + [1.0, 1.0, 1.0]], dtype=np.float64)


def render(spec, env, max_bounces=3, rows=None, counts=None, glass=None):
    """The frame of ``spec`` (or its rows ``rows``) under ``env``: float64 [3, n]. ``glass``: per-sphere
    gains (then through glass_ref, indices of refraction 1.5)."""
    spec = plain(spec)
    if glass is None:
        scene, g = O.scene_from_spec(spec), None
    else:
        scene, gains, iors = glass_ref.scene_of(spec, glass)
        g = (gains, iors)
    if rows is None:
        d = O.ray_directions(scene.cam, scene.width, scene.height)
    else:
        d = O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)
    return np.stack(trace(scene, unit_table(spec), tuple(float(c) for c in scene.cam), d, max_bounces, env, counts, g))
