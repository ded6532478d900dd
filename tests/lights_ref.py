"""NumPy restatement of several point lights (rtx_trace_lights).

The reference lights with ``scene.lights[0]`` alone (main.py: "TODO: use multiple lights"; domain.py:
"class PointLight:  # TODO: add intensity"), so there is no reference output to pin to beyond one unit
light. This is the reference's recursion with its light-dependent terms summed over a table of
lights, built only from the oracle's own pieces (``O.intersect``, ``O._norm``, ``O._dot``,
``O._specular``, ``O._iridescence``, ``O._checker_mask``, ``O.image_texels``) and the arithmetic of
include/rtx_hip.h, in float64 and in that order:

    raytrace_scene(O, D):                                      base.py:91-121
      for every shape at the nearest distance, in scene order:
        color += create(shape, O, D, t)
    create, per channel c:                                     shader.py:63-112
      diffuse = sum_i (((tex*dli_i)*lit_i)*dg)*e_i
      glossy  = sum_i (((spec_i + R*0.5)*g)*lit_i)*e_i        R: raytrace_scene one level deeper
      color   = (((0.004 + diffuse) + dome) + glossy) + irid

recursive like the reference, vectorised over the rays of a call. With the one-row table
``(lights[0], 1, 1, 1)`` it is ``O.trace`` bit for bit (tests/test_lights_cpu.py).
"""

from dataclasses import dataclass
from functools import reduce

import numpy as np

from oracle import numpy_oracle as O


@dataclass
class Counts:
    """What the level-0 hits and the traced reflections of a frame cover."""

    first_only: int = 0  # level-0 hits lit by the first light and by no other
    other_only: int = 0  # ... by one or more of the other lights, not by the first
    several: int = 0  # ... by more than one light (the first among them or not)
    none: int = 0  # ... by no light
    rays: int = 0  # rays traced, every level
    reflected_by_others: int = 0  # reflected rays traced although the first light does not reach the hit
    ties: int = 0  # rays with more than one shape at the nearest distance, every level


def trace(scene, table, origin, dirs, max_bounces, counts=None, level=0):
    """raytrace_scene under the lights of ``table`` (float64 [L, 6]: position, e = intensity * colour)
    for a batch of rays: ``origin`` a 3-tuple of scalars or of arrays, ``dirs`` three arrays. Levels
    0..max_bounces are shaded. ``scene.light_pos`` is not read. Returns [r, g, b] float64 arrays."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    n = dx.shape[0]
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]  # base.py:97
    nearest = reduce(np.minimum, dist)  # base.py:98
    col = [np.zeros(n), np.zeros(n), np.zeros(n)]  # base.py:100
    if counts is not None:
        counts.rays += n
        counts.ties += int((sum(((nearest != O.FARAWAY) & (d == nearest)).astype(np.int64) for d in dist) > 1).sum())
    bounded = level < max_bounces
    cpx, cpy, cpz = scene.cam
    for si, (sp, d) in enumerate(zip(scene.spheres, dist)):
        hit = (nearest != O.FARAWAY) & (d == nearest)  # base.py:103
        if not np.any(hit):  # base.py:105
            continue
        idx = np.nonzero(hit)[0]
        sub = (lambda a: a if np.ndim(a) == 0 else a[idx])  # noqa: E731
        hx, hy, hz, hdx, hdy, hdz, t = sub(ox), sub(oy), sub(oz), dx[idx], dy[idx], dz[idx], d[idx]
        m = idx.shape[0]
        px, py, pz = hx + hdx * t, hy + hdy * t, hz + hdz * t  # shader.py:73
        inv_r = 1.0 / sp.radius
        nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r  # :74
        vx, vy, vz = O._norm(cpx - px, cpy - py, cpz - pz)  # :76
        qx, qy, qz = px + nx * 0.0001, py + ny * 0.0001, pz + nz * 0.0001  # :77
        if sp.checker:
            mask = O._checker_mask(px, pz)
            tex = (1 * mask, 1 * mask, 1 * mask)
        elif sp.image is not None:
            tex = O.image_texels(sp, px, py, pz)
        else:
            tex = sp.tex
        g, dg = sp.specular_gain, sp.diffuse_gain
        lits, specs = [], []
        diffuse = [np.zeros(m) for _ in range(3)]
        reach = [np.zeros(m) for _ in range(3)]  # sum_i lit_i * e_i
        for row in table:
            lx, ly, lz = O._norm(row[0] - px, row[1] - py, row[2] - pz)  # :75
            light_d = [O.intersect(o, qx, qy, qz, lx, ly, lz) for o in scene.spheres]  # :126
            lit = light_d[si] == reduce(np.minimum, light_d)  # :127-128
            dli = np.maximum(O._dot(nx, ny, nz, lx, ly, lz), 0)  # :138
            lits.append(lit)
            specs.append(O._specular(sp, nx, ny, nz, lx, ly, lz, vx, vy, vz))
            for c in range(3):
                diffuse[c] = diffuse[c] + (((tex[c] * dli) * lit) * dg) * row[3 + c]
                reach[c] = reach[c] + lit * row[3 + c]
        # dome, shader.py:234-244 (light_direction = (0, 1, 0))
        dome_i = 0.0
        dome_c = (1.0, 1.0, 1.0)
        for inten, dcol in scene.domes:
            dome_c = dcol
            dome_i += inten * np.maximum(O._dot(nx, ny, nz, 0, 1, 0), 0)
        irid = O._iridescence(sp, nx, ny, nz, vx, vy, vz)
        # the reflected colour (shader.py:143-161): not traced where it is multiplied by zero
        R = [np.zeros(m) for _ in range(3)]
        need = np.zeros(m, dtype=bool)
        if bounded and g != 0:
            need = (reach[0] != 0) | (reach[1] != 0) | (reach[2] != 0)
        if counts is not None:
            others = reduce(np.logical_or, lits[1:], np.zeros(m, dtype=bool))
            counts.reflected_by_others += int((need & ~lits[0]).sum())
            if level == 0:
                nlit = sum(li.astype(np.int64) for li in lits)
                counts.first_only += int((lits[0] & ~others).sum())
                counts.other_only += int((~lits[0] & others).sum())
                counts.several += int((nlit > 1).sum())
                counts.none += int((nlit == 0).sum())
        if need.any():
            dn = O._dot(hdx, hdy, hdz, nx, ny, nz)
            rx, ry, rz = O._norm(hdx - (nx * 2) * dn, hdy - (ny * 2) * dn, hdz - (nz * 2) * dn)  # :151
            child = trace(scene, table, (qx[need], qy[need], qz[need]), (rx[need], ry[need], rz[need]), max_bounces,
                          counts, level + 1)
            for c in range(3):
                R[c][need] = child[c]
        for c in range(3):
            glossy = np.zeros(m)
            for row, lit, spec in zip(table, lits, specs):
                glossy = glossy + (((spec + R[c] * 0.5) * g) * lit) * row[3 + c]
            color = (((0.004 + diffuse[c]) + dome_c[c] * dome_i) + glossy) + irid[c]
            col[c][idx] = col[c][idx] + color  # base.py:119 (scene order)
    return col


def pushes(scene, table, origin, dirs):
    """The reflected rays that the hits of a batch of rays send, in the order k_trace_lights pushes them
    (the shapes at the nearest distance in scene order): a list of (indices into the batch, origins,
    directions). ``trace``'s decisions (``specular_gain != 0`` and a light that reaches the hit) restated
    without the colours; the bounce cap is the caller's."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]
    nearest = reduce(np.minimum, dist)
    out = []
    for si, (sp, d) in enumerate(zip(scene.spheres, dist)):
        idx = np.nonzero((nearest != O.FARAWAY) & (d == nearest))[0]
        if idx.size == 0 or sp.specular_gain == 0:
            continue
        sub = (lambda a: a if np.ndim(a) == 0 else a[idx])  # noqa: E731
        hx, hy, hz, hdx, hdy, hdz, t = sub(ox), sub(oy), sub(oz), dx[idx], dy[idx], dz[idx], d[idx]
        px, py, pz = hx + hdx * t, hy + hdy * t, hz + hdz * t
        inv_r = 1.0 / sp.radius
        nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r
        qx, qy, qz = px + nx * 0.0001, py + ny * 0.0001, pz + nz * 0.0001
        reach = [np.zeros(idx.size) for _ in range(3)]
        for row in table:
            lx, ly, lz = O._norm(row[0] - px, row[1] - py, row[2] - pz)
            light_d = [O.intersect(o, qx, qy, qz, lx, ly, lz) for o in scene.spheres]
            lit = light_d[si] == reduce(np.minimum, light_d)
            for c in range(3):
                reach[c] = reach[c] + lit * row[3 + c]
        need = (reach[0] != 0) | (reach[1] != 0) | (reach[2] != 0)
        if need.any():
            dn = O._dot(hdx, hdy, hdz, nx, ny, nz)
            rx, ry, rz = O._norm(hdx - (nx * 2) * dn, hdy - (ny * 2) * dn, hdz - (nz * 2) * dn)
            out.append((idx[need], (qx[need], qy[need], qz[need]), (rx[need], ry[need], rz[need])))
    return out


def pending_need(scene, table, origin, dirs, max_bounces, level=0):
    """Per ray, the largest number of pending rays that k_trace_lights's depth-first walk would hold with an
    unbounded stack (the kernel's holds 2 * max_bounces + 2; a lane that needs more drops rays and reports
    RTX_ST_STACK_OVERFLOW): tests/mesh_ref.py's recursion over ``pushes``. An int64 array, at least 1."""
    n = np.asarray(dirs[0]).shape[0]
    need = np.ones(n, dtype=np.int64)
    if level >= max_bounces or n == 0:  # the next level is black: nothing is pushed
        return need
    pushed = np.zeros(n, dtype=np.int64)
    for rays, o2, d2 in pushes(scene, table, origin, dirs):
        child = pending_need(scene, table, o2, d2, max_bounces, level + 1)
        need[rays] = np.maximum(need[rays], pushed[rays] + child)
        pushed[rays] += 1
    return need


def table_of(spec):
    """The lights table of ``spec`` as lights.lights_table builds it from the scene: every point entry
    in list order, e = intensity * colour (defaults 1 and white)."""
    rows = []
    for li in spec["lights"]:
        if li["kind"] != "point":
            continue
        inten = float(li.get("intensity", 1.0))
        rows.append([float(x) for x in li["position"]] + [inten * float(c) for c in li.get("color", (1.0, 1.0, 1.0))])
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 6)


def render(spec, max_bounces=3, rows=None, counts=None, table=None):
    """The frame of ``spec`` (or its rows ``rows``, global indices in the given order) under all its
    point lights (or ``table``): float64 [3, n]."""
    scene = O.scene_from_spec(spec)
    table = table_of(spec) if table is None else table
    if rows is None:
        d = O.ray_directions(scene.cam, scene.width, scene.height)
    else:
        d = O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)
    return np.stack(trace(scene, table, tuple(float(c) for c in scene.cam), d, max_bounces, counts))
