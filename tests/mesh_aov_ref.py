"""NumPy restatement of the primary-hit render passes of a mesh scene (rtx_mesh_aovs).

Composed of pieces that exist: the triangle group, its nearest hit and its shadow distances from
tests/mesh_ref.py (``group_of``, ``nearest_triangle``, ``_min_by_mesh``, ``Pruner``), the image lookup of
tests/meshuv_ref.py, the lights table of tests/mesh_ref.py (tests/lights_ref.py's) and the oracle's
``O.intersect``, ``O._norm``, ``O._dot``, ``O._checker_mask`` and ``O.image_texels``. Every triangle is tried
for every ray, with no tree, in the arithmetic and the order of include/rtx_hip.h: tests/mesh_ref.py's
``trace`` up to the call of ``_shade``, with the values written out instead of shaded.

The first hit of a ray is the first sphere in scene order at the nearest distance, else the group's
triangle. tests/test_mesh_aov_cpu.py pins the passes to tests/aov_ref.py where no triangle is in sight and
to ``mesh_ref.render`` through ``mesh_ref._shade``.
"""

from functools import reduce

import numpy as np

from oracle import numpy_oracle as O
from tests import mesh_ref as R
from tests import meshuv_ref as U

PASSES = ("depth", "id", "hits", "position", "normal", "geometric_normal", "albedo", "lit", "triangle", "bary")


def aovs(scene: O.OScene, ug: U.UvGroup, table, origin, dirs, shape_ids=None, prune=None) -> dict:
    """The ten passes of rays (origin, dirs) through the spheres of ``scene`` and the group ``ug`` under the
    lights table ``table`` [L, 6]: depth float64 [n], id / hits / triangle int32 [n], position / normal /
    geometric_normal / albedo float64 [3, n], lit uint8 [n] (bit i: row i), bary float64 [2, n].
    ``shape_ids``: what ``id`` reports for the spheres, then for the meshes (None: their position in that
    order). ``prune``: a mesh_ref.Pruner whose tree's pruning is emulated, as mesh_ref.trace emulates it."""
    g = ug.g
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    n = dx.shape[0]
    ox, oy, oz = (np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)) for a in origin)
    S = len(scene.spheres)
    ids = np.arange(S + len(g.mats)) if shape_ids is None else np.asarray(shape_ids)
    dist = [np.broadcast_to(O.intersect(sp, ox, oy, oz, dx, dy, dz), (n,)) for sp in scene.spheres]  # base.py:97
    near_s = reduce(np.minimum, dist, np.full(n, O.FARAWAY))
    vis = None if prune is None else prune.visible(ox, oy, oz, dx, dy, dz, near_s)
    tt, num, tu, tv, _ = R.nearest_triangle(g, ox, oy, oz, dx, dy, dz, vis)
    if prune is not None:  # ... and with the tightest limit of a walk: the group's own nearest distance
        vis = prune.visible(ox, oy, oz, dx, dy, dz, np.minimum(near_s, tt))
        tt, num, tu, tv, _ = R.nearest_triangle(g, ox, oy, oz, dx, dy, dz, vis)
    nearest = np.minimum(near_s, tt)  # base.py:98
    some = nearest != O.FARAWAY
    first = np.full(n, -1)
    hits = np.zeros(n, dtype=np.int32)
    for si, d in enumerate(dist):
        hit = some & (d == nearest)  # base.py:102-103
        hits += hit
        first[hit & (first < 0)] = si
    tie_tri = some & (tt == nearest)
    hits += tie_tri
    on_tri = tie_tri & (first < 0)
    out = {"depth": np.array(nearest, dtype=np.float64), "id": np.full(n, -1, dtype=np.int32), "hits": hits,
           "position": np.zeros((3, n)), "normal": np.zeros((3, n)), "geometric_normal": np.zeros((3, n)),
           "albedo": np.zeros((3, n)), "lit": np.zeros(n, dtype=np.uint8),
           "triangle": np.where(on_tri, num, -1).astype(np.int32), "bary": np.zeros((2, n))}

    def lit_bits(si, px, py, pz, qx, qy, qz):
        m = px.shape[0]
        bits = np.zeros(m, dtype=np.uint8)
        for li, row in enumerate(table):
            lx, ly, lz = O._norm(row[0] - px, row[1] - py, row[2] - pz)  # shader.py:75
            light_d = [O.intersect(o, qx, qy, qz, lx, ly, lz) for o in scene.spheres]  # :126
            tself = light_d[si] if si >= 0 else np.full(m, O.FARAWAY)
            v = None if prune is None else prune.visible(qx, qy, qz, lx, ly, lz, tself)
            tri_d, _ = R._min_by_mesh(g, qx, qy, qz, lx, ly, lz, v)
            sph_d = reduce(np.minimum, light_d, np.full(m, O.FARAWAY))
            lit = tself == np.minimum(sph_d, tri_d)  # :127-128 with the triangles taking part
            bits |= (lit.astype(np.uint8) << li).astype(np.uint8)
        return bits

    def write(idx, P, N, G, tex, bits):
        for c in range(3):
            out["position"][c, idx] = P[c]
            out["normal"][c, idx] = N[c]
            out["geometric_normal"][c, idx] = G[c]
            out["albedo"][c, idx] = tex[c]
        out["lit"][idx] = bits

    for si, sp in enumerate(scene.spheres):
        idx = np.nonzero(first == si)[0]
        if idx.size == 0:
            continue
        t = nearest[idx]
        px, py, pz = ox[idx] + dx[idx] * t, oy[idx] + dy[idx] * t, oz[idx] + dz[idx] * t  # shader.py:73
        inv_r = 1.0 / sp.radius
        nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r  # :74
        qx, qy, qz = px + nx * 0.0001, py + ny * 0.0001, pz + nz * 0.0001  # :77
        if sp.checker:
            m = O._checker_mask(px, pz)  # shader.py:30-32
            tex = (1 * m, 1 * m, 1 * m)
        elif sp.image is not None:
            tex = O.image_texels(sp, px, py, pz)  # shape.py:66-79
        else:
            tex = sp.tex  # shader.py:17-19
        out["id"][idx] = ids[si]
        write(idx, (px, py, pz), (nx, ny, nz), (nx, ny, nz), tex, lit_bits(si, px, py, pz, qx, qy, qz))

    idx = np.nonzero(on_tri)[0]
    if idx.size:
        t, r, u, v = nearest[idx], num[idx], tu[idx], tv[idx]
        hdx, hdy, hdz = dx[idx], dy[idx], dz[idx]
        px, py, pz = ox[idx] + hdx * t, oy[idx] + hdy * t, oz[idx] + hdz * t
        flip = np.where(O._dot(g.ng[r, 0], g.ng[r, 1], g.ng[r, 2], hdx, hdy, hdz) > 0, -1.0, 1.0)
        gx, gy, gz = g.ng[r, 0] * flip, g.ng[r, 1] * flip, g.ng[r, 2] * flip
        w0 = (1.0 - u) - v
        sx, sy, sz = ((w0 * g.n0[r, c] + u * g.n1[r, c]) + v * g.n2[r, c] for c in range(3))
        with np.errstate(all="ignore"):  # (the rows without vertex normals: 0 / 0, not taken)
            sx, sy, sz = O._norm(sx, sy, sz)
        back = np.where(O._dot(sx, sy, sz, gx, gy, gz) < 0, -1.0, 1.0)
        smooth = g.smooth[r]
        nx, ny, nz = (np.where(smooth, s * back, f) for s, f in ((sx, gx), (sy, gy), (sz, gz)))
        qx, qy, qz = px + gx * 0.0001, py + gy * 0.0001, pz + gz * 0.0001  # :77 (the face normal)
        tex = [np.zeros(idx.size) for _ in range(3)]
        for mi, mat in enumerate(g.mats):
            sel = np.nonzero(g.mesh[r] == mi)[0]
            if sel.size == 0:
                continue
            if ug.images[mi] is not None:
                part = U.lookup(ug.images[mi], ug.uvs[r[sel]], u[sel], v[sel])
            elif mat.checker:
                m = O._checker_mask(px[sel], pz[sel])
                part = (1 * m, 1 * m, 1 * m)
            else:
                part = mat.tex
            for c in range(3):
                tex[c][sel] = part[c]
        out["id"][idx] = ids[S + g.mesh[r]]
        out["bary"][0, idx], out["bary"][1, idx] = u, v
        write(idx, (px, py, pz), (nx, ny, nz), (gx, gy, gz), tex, lit_bits(-1, px, py, pz, qx, qy, qz))
    for a in out.values():
        a.setflags(write=False)
    return out


def of_spec(spec, origin=None, dirs=None, rows=None, shape_ids=None, prune=None) -> dict:
    """``aovs`` of ``spec``'s frame (or of its rows ``rows``, or of the explicit rays ``origin``, ``dirs``)."""
    scene = O.scene_from_spec(spec)
    if dirs is None:
        origin = tuple(float(c) for c in scene.cam)
        dirs = O.ray_directions(scene.cam, scene.width, scene.height) if rows is None else \
            O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)
    return aovs(scene, U.group_of(spec), R.table_of(spec), tuple(origin), tuple(dirs), shape_ids, prune)


_FRAMES: dict = {}


def frame(key, spec_fn) -> tuple:
    """(spec, the passes of its whole frame) of ``spec_fn()``, computed once per ``key`` and read-only."""
    if key not in _FRAMES:
        spec = spec_fn()
        _FRAMES[key] = (spec, of_spec(spec))
    return _FRAMES[key]
