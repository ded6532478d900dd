"""NumPy restatement of transmission (glass spheres; rtx_trace_glass).

The reference has no transmission (shader.py:143, "TODO: VOIR TRANSMISSION"), so there is no reference
output to pin to. This is the reference's recursion with the one term the feature adds, built only
from the oracle's own pieces (``O.intersect``, ``O._shade``, ``O._norm``, ``O._dot``) and the
arithmetic of include/rtx_hip.h, in float64 and in that order:

    raytrace_scene(O, D):                                      base.py:91-121
      for every shape at the nearest distance, in scene order:
        color += create(shape, O, D, t)
    create:                                                    shader.py:63-112
      color = ((A + (spec + reflection*0.5)*g*lit) + irid)     reflection: raytrace_scene one level deeper
      color += transmission * transmission_gain                transmission: likewise, through the ball

recursive like the reference, vectorised over the rays of a call. With every gain 0 it is ``O.trace``
bit for bit (tests/test_glass_cpu.py).
"""

from dataclasses import dataclass
from functools import reduce

import numpy as np

from oracle import numpy_oracle as O


@dataclass
class Counts:
    rays: int = 0  # rays traced, every level
    transmitted: int = 0  # of them, rays that left a glass ball
    inside: int = 0  # shaded hits of a glass sphere from inside (D.n >= 0) below the cap: no transmitted ray
    clamps: int = 0  # exits whose 1 - ior^2 (1 - ce^2) was negative (clamped to 0)
    deepest: int = 0  # the deepest level a ray was traced at
    ties: int = 0  # rays with more than one shape at the nearest distance, every level
    ties0: int = 0  # of them, level-0 rays


def through_ball(sp, ior, ox, oy, oz, dx, dy, dz, t, counts=None):
    """The ray leaving the solid ball ``sp`` for rays (O, D) that hit it at distance ``t``: (c, O', D')
    with c = D.n; only rays with c < 0 are transmitted (the others' O', D' are meaningless)."""
    px, py, pz = ox + dx * t, oy + dy * t, oz + dz * t  # shader.py:73
    inv_r = 1.0 / sp.radius
    nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r  # shader.py:74
    c = O._dot(dx, dy, dz, nx, ny, nz)
    eta = 1.0 / ior
    ci = -c
    k = 1.0 - (eta * eta) * (1.0 - ci * ci)
    with np.errstate(invalid="ignore"):
        f = eta * ci - np.sqrt(k)
    tx, ty, tz = O._norm(dx * eta + nx * f, dy * eta + ny * f, dz * eta + nz * f)
    mx, my, mz = px - sp.cx, py - sp.cy, pz - sp.cz
    b = O._dot(tx, ty, tz, mx, my, mz)
    ex, ey, ez = px - tx * (2 * b), py - ty * (2 * b), pz - tz * (2 * b)
    ux, uy, uz = (ex - sp.cx) * inv_r, (ey - sp.cy) * inv_r, (ez - sp.cz) * inv_r
    ce = O._dot(tx, ty, tz, ux, uy, uz)
    raw = 1.0 - (ior * ior) * (1.0 - ce * ce)
    if counts is not None:
        counts.clamps += int(((raw < 0) & (c < 0)).sum())
    ke = np.maximum(raw, 0.0)
    g = np.sqrt(ke) - ior * ce
    o2 = (ex + ux * 0.0001, ey + uy * 0.0001, ez + uz * 0.0001)
    d2 = O._norm(tx * ior + ux * g, ty * ior + uy * g, tz * ior + uz * g)
    return c, o2, d2


def trace(scene, gains, iors, origin, dirs, max_bounces, counts=None, level=0):
    """raytrace_scene with transmission for a batch of rays: ``origin`` a 3-tuple of scalars or of
    arrays, ``dirs`` three arrays; ``gains`` / ``iors`` per sphere. Levels 0..max_bounces are shaded.
    Returns [r, g, b] float64 arrays."""
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    n = dx.shape[0]
    if counts is not None:
        counts.rays += n
        counts.deepest = max(counts.deepest, level)
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]  # base.py:97
    nearest = reduce(np.minimum, dist)  # base.py:98
    col = [np.zeros(n), np.zeros(n), np.zeros(n)]  # base.py:100
    if counts is not None:
        tied = int((sum(((nearest != O.FARAWAY) & (d == nearest)).astype(np.int64) for d in dist) > 1).sum())
        counts.ties += tied
        if level == 0:
            counts.ties0 += tied
    bounded = level < max_bounces
    for si, (sp, d) in enumerate(zip(scene.spheres, dist)):
        hit = (nearest != O.FARAWAY) & (d == nearest)  # base.py:103
        if not np.any(hit):  # base.py:105
            continue
        idx = np.nonzero(hit)[0]
        sub = (lambda a: a if np.ndim(a) == 0 else a[idx])  # noqa: E731
        hx, hy, hz, hdx, hdy, hdz, ht = sub(ox), sub(oy), sub(oz), dx[idx], dy[idx], dz[idx], d[idx]
        A, spec, lit, irid, q, r = O._shade(scene, si, sp, hx, hy, hz, hdx, hdy, hdz, ht)
        m = idx.shape[0]
        R = [np.zeros(m) for _ in range(3)]
        need = lit & (sp.specular_gain != 0) if bounded else np.zeros(m, dtype=bool)
        if need.any():  # (a reflection that is multiplied by zero is not traced: O.trace's rule)
            child = trace(scene, gains, iors, tuple(np.broadcast_to(c, (m,))[need] for c in q),
                          tuple(c[need] for c in r), max_bounces, counts, level + 1)
            for c in range(3):
                R[c][need] = child[c]
        color = [(A[c] + (spec + R[c] * 0.5) * sp.specular_gain * lit) + irid[c] for c in range(3)]  # shader.py:106-110
        tg = gains[si]
        if tg != 0:
            T = [np.zeros(m) for _ in range(3)]
            if bounded:
                cdn, o2, d2 = through_ball(sp, iors[si], hx, hy, hz, hdx, hdy, hdz, ht, counts)
                go = cdn < 0
                if counts is not None:
                    counts.inside += int((~go).sum())
                    counts.transmitted += int(go.sum())
                if go.any():
                    child = trace(scene, gains, iors, tuple(c[go] for c in o2), tuple(c[go] for c in d2), max_bounces,
                                  counts, level + 1)
                    for c in range(3):
                        T[c][go] = child[c]
            color = [color[c] + T[c] * tg for c in range(3)]
        for c in range(3):
            col[c][idx] = col[c][idx] + color[c]  # base.py:119 (scene order)
    return col


def pending_need(scene, gains, iors, origin, dirs, max_bounces, level=0):
    """Per ray, the largest number of pending rays that k_trace_glass's depth-first walk would hold with
    an unbounded stack (the kernel's holds 4 * max_bounces + 4; a lane that needs more drops rays and
    reports RTX_ST_STACK_OVERFLOW). Arguments as ``trace``; an int64 array, at least 1: the ray itself.

    The walk pops a ray and, for every shape at the nearest distance in scene order, when level <
    max_bounces, pushes the reflected ray (``lit and specular_gain != 0``) and then the transmitted one
    (``gain != 0 and c < 0``); it pops the last pushed first and finishes that ray's whole tree before the
    next. So the j-th ray a node pushed (from 0) is popped with j siblings still below it, and a node
    needs max(1, max_j (j + need of its j-th child)) entries, itself included: the recursion below,
    vectorised over the rays of a call like ``trace`` and built from the same pieces."""
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    n = dx.shape[0]
    need = np.ones(n, dtype=np.int64)
    if level >= max_bounces or n == 0:  # the next level is black: nothing is pushed
        return need
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]
    nearest = reduce(np.minimum, dist)
    pushed = np.zeros(n, dtype=np.int64)

    def push(rays, o2, d2):  # the child rays of the rays ``rays`` (indices into this call's)
        child = pending_need(scene, gains, iors, o2, d2, max_bounces, level + 1)
        need[rays] = np.maximum(need[rays], pushed[rays] + child)
        pushed[rays] += 1

    for si, (sp, d) in enumerate(zip(scene.spheres, dist)):
        hit = (nearest != O.FARAWAY) & (d == nearest)
        if not np.any(hit):
            continue
        idx = np.nonzero(hit)[0]
        sub = (lambda a: a if np.ndim(a) == 0 else a[idx])  # noqa: E731
        hx, hy, hz, hdx, hdy, hdz, ht = sub(ox), sub(oy), sub(oz), dx[idx], dy[idx], dz[idx], d[idx]
        m = idx.shape[0]
        _, _, lit, _, q, r = O._shade(scene, si, sp, hx, hy, hz, hdx, hdy, hdz, ht)
        refl = np.broadcast_to(lit & (sp.specular_gain != 0), (m,))
        if refl.any():
            push(idx[refl], tuple(np.broadcast_to(c, (m,))[refl] for c in q), tuple(c[refl] for c in r))
        if gains[si] != 0:
            cdn, o2, d2 = through_ball(sp, iors[si], hx, hy, hz, hdx, hdy, hdz, ht)
            go = cdn < 0
            if go.any():
                push(idx[go], tuple(c[go] for c in o2), tuple(c[go] for c in d2))
    return need


def scene_of(spec, gains, iors=None):
    """(the oracle's scene of ``spec``, gains, iors) as ``trace`` takes them: ``iors`` default to 1.5
    each (shader.py:51) and are the shaders' specular_ior (the specular's F0 reads it too, shader.py:290)."""
    scene = O.scene_from_spec(spec)
    S = len(scene.spheres)
    gains = [float(g) for g in gains]
    iors = [1.5] * S if iors is None else [float(v) for v in iors]
    assert len(gains) == S and len(iors) == S
    for sp, ior in zip(scene.spheres, iors):
        sp.specular_ior = ior
    return scene, gains, iors


def render(spec, gains, iors=None, max_bounces=3, rows=None, counts=None):
    """The frame of ``spec`` (or its rows ``rows``, global indices in the given order) with per-sphere
    ``gains`` and ``iors``: float64 [3, n]."""
    scene, gains, iors = scene_of(spec, gains, iors)
    if rows is None:
        d = O.ray_directions(scene.cam, scene.width, scene.height)
    else:
        d = O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)
    return np.stack(trace(scene, gains, iors, tuple(float(c) for c in scene.cam), d, max_bounces, counts))


def with_gains(spec, gains, iors=None):
    """A copy of ``spec`` whose shaders carry ``transmission_gain`` (and ``specular_ior``) per sphere."""
    import copy

    out = copy.deepcopy(spec)
    for i, sp in enumerate(out["spheres"]):
        sp["shader"]["transmission_gain"] = gains[i]
        if iors is not None:
            sp["shader"]["specular_ior"] = iors[i]
    return out
