"""NumPy reference of the primary-hit render passes (HipRenderer.render_aovs, rtx_primary_aovs).

Composed only of the oracle's public pieces (``O.intersect``, ``O.ray_directions_rows``,
``O._norm``, ``O._checker_mask``, ``O.image_texels``), in the reference's expressions and operation
order: the nearest distance and hit shapes of ``raytrace_scene`` (base.py:97-103), P, the normal and
``is_in_light`` of ``NumpyShader.create`` (shader.py:73-84, 126-128) and ``get_color``. Vectorised
per shape, as the reference loops over ``scene.shapes``; origins may be scalars (the camera, as at
the reference's level 0) or arrays. tests/test_aov_cpu.py pins it to ``O._shade``, ``O.create`` and
``O.render``.
"""

from functools import reduce

import numpy as np

from oracle import numpy_oracle as O

PASSES = ("depth", "id", "hits", "position", "normal", "albedo", "lit")


def aovs(scene: O.OScene, origin, dirs) -> dict:
    """The seven passes of rays (origin, dirs) plus ``nudged`` (the shadow ray's origin, shader.py:77):
    depth float64 [n], id / hits int32 [n], position / normal / albedo / nudged float64 [3, n],
    lit uint8 [n]. Misses: depth FARAWAY, id -1, hits 0, everything else 0."""
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    n = dx.shape[0]
    ox, oy, oz = origin
    dist = [np.broadcast_to(O.intersect(sp, ox, oy, oz, dx, dy, dz), (n,)) for sp in scene.spheres]  # base.py:97
    nearest = reduce(np.minimum, dist)  # base.py:98
    ident = np.full(n, -1, dtype=np.int32)
    hits = np.zeros(n, dtype=np.int32)
    for si, d in enumerate(dist):
        hit = (nearest != O.FARAWAY) & (d == nearest)  # base.py:102-103
        hits += hit
        ident[hit & (ident < 0)] = si
    out = {"depth": np.array(nearest, dtype=np.float64), "id": ident, "hits": hits,
           "position": np.zeros((3, n)), "normal": np.zeros((3, n)), "albedo": np.zeros((3, n)),
           "nudged": np.zeros((3, n)), "lit": np.zeros(n, dtype=np.uint8)}
    lpx, lpy, lpz = scene.light_pos
    for si, sp in enumerate(scene.spheres):
        idx = np.nonzero(ident == si)[0]
        if idx.size == 0:
            continue
        sub = (lambda a: a if np.ndim(a) == 0 else np.asarray(a)[idx])  # noqa: E731 - extract, base.py:15-25
        t = nearest[idx]
        px, py, pz = sub(ox) + dx[idx] * t, sub(oy) + dy[idx] * t, sub(oz) + dz[idx] * t  # shader.py:73
        inv_r = 1.0 / sp.radius
        nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r  # :74
        lx, ly, lz = O._norm(lpx - px, lpy - py, lpz - pz)  # :75
        qx, qy, qz = px + nx * 0.0001, py + ny * 0.0001, pz + nz * 0.0001  # :77
        light_d = [O.intersect(o, qx, qy, qz, lx, ly, lz) for o in scene.spheres]  # :126
        lit = light_d[si] == reduce(np.minimum, light_d)  # :127-128
        if sp.checker:
            m = O._checker_mask(px, pz)  # shader.py:30-32
            tex = (1 * m, 1 * m, 1 * m)
        elif sp.image is not None:
            tex = O.image_texels(sp, px, py, pz)  # shape.py:66-79
        else:
            tex = sp.tex  # shader.py:17-19
        for c, (p_, n_, q_) in enumerate(((px, nx, qx), (py, ny, qy), (pz, nz, qz))):
            out["position"][c, idx] = p_
            out["normal"][c, idx] = n_
            out["nudged"][c, idx] = q_
            out["albedo"][c, idx] = tex[c]
        out["lit"][idx] = lit
    for v in out.values():
        v.setflags(write=False)
    return out


def frame_rays(scene: O.OScene, rows=None):
    """(origin, dirs) of the camera rays of the frame rows ``rows`` (default: all, top to bottom)."""
    rows = np.arange(scene.height) if rows is None else rows
    return tuple(float(c) for c in scene.cam), O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)


_FRAMES: dict = {}


def frame(key, spec_fn) -> tuple:
    """(OScene, aovs of its whole frame) of ``spec_fn()``, computed once per ``key`` and read-only."""
    if key not in _FRAMES:
        scene = O.scene_from_spec(spec_fn())
        _FRAMES[key] = (scene, aovs(scene, *frame_rays(scene)))
    return _FRAMES[key]
