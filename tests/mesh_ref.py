"""NumPy restatement of triangle meshes (rtx_trace_mesh).

The reference has one shape, the sphere, so there is no reference output to pin a triangle to. This is
the reference's recursion (base.py:91-121, shader.py:63-112) over the spheres of a scene and one group
of triangles, lit by a table of lights as tests/lights_ref.py sums them, built from the oracle's own
pieces (``O.intersect``, ``O._norm``, ``O._dot``, ``O._specular``, ``O._iridescence``,
``O._checker_mask``) with the normal passed in, and the arithmetic of include/rtx_hip.h in float64 and
in that order. Every triangle is tried for every ray, in group order, with no tree:

    T = O - v0;  P = D x e2;  det = e1.P;  f = 1.0 / det
    u = f * T.P;  Q = T x e1;  v = f * D.Q;  t = f * e2.Q
    hit <=> det != 0, u >= 0, v >= 0, u + v <= 1, 0 < t < FARAWAY

The group's hit is the smallest t, the lowest number among equal t. The spheres at the nearest distance
shade in scene order, then the triangle if its t equals it. A hit is lit by a light unless a shape is
strictly nearer than its own distance along L from the nudged point, a triangle's own distance being
FARAWAY. ``prune``: a device table (meshes.mesh_table) whose tree's pruning is emulated per ray with the
tightest limit a walk can have; the frame must not depend on it.
"""

from dataclasses import dataclass
from functools import reduce

import numpy as np

from oracle import numpy_oracle as O
from python_ray_tracer_amd import meshes as M
from python_ray_tracer_amd import scenes

BLOCK = 1024  # triangles per block of the brute-force test


@dataclass
class Counts:
    """What the hits and the traced reflections of a frame cover."""

    tri_primary: int = 0  # level-0 rays whose nearest hit is a triangle
    smooth_hits: int = 0  # hits on a row with vertex normals, every level
    sphere_shadows_tri: int = 0  # (hit on a triangle, light) pairs that a sphere shadows
    tri_shadows_sphere: int = 0  # (hit on a sphere, light) pairs that only a triangle shadows
    self_shadow: int = 0  # (hit on a triangle, light) pairs that a triangle of the same mesh shadows
    sphere_to_tri: int = 0  # reflected rays from a sphere whose nearest hit is a triangle
    tri_to_sphere: int = 0  # reflected rays from a triangle whose nearest hit is a sphere
    ties: int = 0  # rays whose nearest distance a sphere and the triangle group share
    tri_ties: int = 0  # rays whose nearest triangle distance two triangles share
    rays: int = 0  # rays traced, every level


@dataclass
class Group:
    """The triangles of a scene in group order, and one material (an O.OSphere's fields) per mesh."""

    v0: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    ng: np.ndarray
    mesh: np.ndarray
    smooth: np.ndarray
    n0: np.ndarray
    n1: np.ndarray
    n2: np.ndarray
    mats: list


def group_of(spec) -> Group:
    """The triangle group of ``spec["meshes"]``, from the vertices and faces alone."""
    parts, mats = [], []
    for i, m in enumerate(spec["meshes"]):
        v, f, n = scenes.mesh_arrays(m)
        v0 = v[f[:, 0]]
        e1, e2 = v[f[:, 1]] - v0, v[f[:, 2]] - v0
        ng = np.cross(e1, e2)
        ng = ng / np.sqrt((ng * ng).sum(axis=1, keepdims=True))
        z = np.zeros_like(v0)
        nn = (z, z, z) if n is None else (n[f[:, 0]], n[f[:, 1]], n[f[:, 2]])
        parts.append((v0, e1, e2, ng, np.full(len(f), i), np.full(len(f), n is not None), *nn))
        sh = m["shader"]
        tex = sh["texture"]
        mats.append(O.OSphere(0.0, 0.0, 0.0, 1.0, sh["reflection_gain"], sh["specular_gain"], sh["specular_roughness"],
                              sh["iridescence_gain"], sh["diffuse_gain"], tex["kind"] == "checker",
                              tuple(tex.get("color", (1, 1, 1)))))
    cols = [np.concatenate(c) for c in zip(*parts)]
    return Group(*cols, mats)


def _tri_tests(g: Group, rows, ox, oy, oz, dx, dy, dz):
    """(t or FARAWAY, u, v) float64 [len(rows), n] of the triangles ``rows`` against n rays."""
    col = lambda a, i: a[rows, i].reshape(-1, 1)  # noqa: E731
    ox, oy, oz = (np.broadcast_to(np.asarray(a, dtype=np.float64), dx.shape).reshape(1, -1) for a in (ox, oy, oz))
    dx, dy, dz = (a.reshape(1, -1) for a in (dx, dy, dz))
    with np.errstate(all="ignore"):
        tx, ty, tz = ox - col(g.v0, 0), oy - col(g.v0, 1), oz - col(g.v0, 2)
        e1x, e1y, e1z = col(g.e1, 0), col(g.e1, 1), col(g.e1, 2)
        e2x, e2y, e2z = col(g.e2, 0), col(g.e2, 1), col(g.e2, 2)
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = O._dot(e1x, e1y, e1z, px, py, pz)
        f = 1.0 / det
        u = f * O._dot(tx, ty, tz, px, py, pz)
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        v = f * O._dot(dx, dy, dz, qx, qy, qz)
        t = f * O._dot(e2x, e2y, e2z, qx, qy, qz)
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < O.FARAWAY)
    return np.where(hit, t, O.FARAWAY), u, v


def nearest_triangle(g: Group, ox, oy, oz, dx, dy, dz, visible=None):
    """(t, number, u, v, how many triangles share t) of the group's hit per ray: the smallest t, the
    lowest number among equal t; t FARAWAY and number -1 on a miss. ``visible``: bool [T, n], the
    triangles a pruned walk tests."""
    n = dx.shape[0]
    best = np.full(n, O.FARAWAY)
    num = np.full(n, -1)
    bu, bv, share = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for k in range(0, g.v0.shape[0], BLOCK):
        rows = np.arange(k, min(k + BLOCK, g.v0.shape[0]))
        t, u, v = _tri_tests(g, rows, ox, oy, oz, dx, dy, dz)
        if visible is not None:
            t = np.where(visible[rows], t, O.FARAWAY)
        j = np.argmin(t, axis=0)  # (the first of equal t: the lowest number of the block)
        tj = t[j, np.arange(n)]
        same = (tj == best) & (tj != O.FARAWAY)
        share = np.where(tj < best, (t == tj).sum(axis=0), np.where(same, share + (t == tj).sum(axis=0), share))
        better = tj < best  # (strictly: an equal t of a later block has a higher number)
        best = np.where(better, tj, best)
        num = np.where(better, rows[j], num)
        bu = np.where(better, u[j, np.arange(n)], bu)
        bv = np.where(better, v[j, np.arange(n)], bv)
    return best, num, bu, bv, share


def _min_by_mesh(g: Group, qx, qy, qz, lx, ly, lz, visible=None):
    """The smallest triangle t per ray, over all triangles and over those of each mesh: ([n], [M, n])."""
    n = lx.shape[0]
    per = np.full((len(g.mats), n), O.FARAWAY)
    for k in range(0, g.v0.shape[0], BLOCK):
        rows = np.arange(k, min(k + BLOCK, g.v0.shape[0]))
        t, _, _ = _tri_tests(g, rows, qx, qy, qz, lx, ly, lz)
        if visible is not None:
            t = np.where(visible[rows], t, O.FARAWAY)
        for mi in np.unique(g.mesh[rows]):
            per[mi] = np.minimum(per[mi], t[g.mesh[rows] == mi].min(axis=0))
    return per.min(axis=0), per


# ---- the tree's pruning, per ray ---------------------------------------------------------------
class Pruner:
    """The triangles a walk of ``table``'s tree tests for a ray and a limit, per ray (the device enters
    a node when any lane of the wave may hit it, so it tests these and more): a triangle is visible
    if its leaf and every node above it pass node_may_hit (rtx_device.h) at the limit."""

    def __init__(self, table) -> None:
        from python_ray_tracer_amd.infrastructure.hip import _lib as L

        t = np.asarray(table)
        T, N = int(t[M.MH_NTRI]), int(t[M.MH_NNODES])
        self.nodes = t[int(t[M.MH_NODES]):][:N * L.NODE_WORDS].reshape(N, L.NODE_WORDS)
        rows = t[int(t[M.MH_TRIS]):][:T * M.TRI_WORDS].reshape(T, M.TRI_WORDS)
        self.number = rows[:, M.T_NUM].astype(np.int64)  # table row -> group number
        self.L = L
        skip = self.nodes[:, L.N_SKIP].astype(np.int64)
        self.parent = np.full(N, -1)
        stack = []
        for i in range(N):
            while stack and skip[stack[-1]] <= i:
                stack.pop()
            if stack:
                self.parent[i] = stack[-1]
            stack.append(i)

    def visible(self, ox, oy, oz, dx, dy, dz, tlim):
        L, nd = self.L, self.nodes
        n = dx.shape[0]
        o = [np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)).reshape(1, -1) for a in (ox, oy, oz)]
        oo = O._dot(*o, *o)
        m = nd[:, L.N_MARGIN].reshape(-1, 1) + 6e-7 * oo
        tn, tf = np.full((nd.shape[0], n), -np.inf), np.full((nd.shape[0], n), np.inf)
        with np.errstate(all="ignore"):
            for a, d, lo, hi in zip(o, (dx, dy, dz), (L.N_LOX, L.N_LOY, L.N_LOZ), (L.N_HIX, L.N_HIY, L.N_HIZ)):
                d = d.reshape(1, -1)
                inv = 1.0 / np.where(np.abs(d) < 1e-200, np.copysign(1e-200, d), d)
                a0 = ((nd[:, lo].reshape(-1, 1) - m) - a) * inv
                a1 = ((nd[:, hi].reshape(-1, 1) + m) - a) * inv
                tn, tf = np.fmax(tn, np.fmin(a0, a1)), np.fmin(tf, np.fmax(a0, a1))
        ok = (tn <= tf) & (tf >= 0.0) & (tn <= np.asarray(tlim).reshape(1, -1))
        for i in range(nd.shape[0]):  # (depth first: a parent comes before its children)
            if self.parent[i] >= 0:
                ok[i] &= ok[self.parent[i]]
        vis = np.zeros((self.number.shape[0], n), dtype=bool)
        for i in np.nonzero(nd[:, L.N_COUNT] > 0)[0]:
            first, cnt = int(nd[i, L.N_FIRST]), int(nd[i, L.N_COUNT])
            vis[self.number[first:first + cnt]] = ok[i]
        return vis


# ---- the recursion -----------------------------------------------------------------------------
def trace(scene, g: Group, table, origin, dirs, max_bounces, counts=None, level=0, prune=None, parent=None):
    """raytrace_scene over the spheres of ``scene`` (an O.OScene; it may have none) and the group ``g``
    under the lights of ``table`` (float64 [L, 6]) for a batch of rays. Levels 0..max_bounces are
    shaded. Returns [r, g, b] float64 arrays."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    n = dx.shape[0]
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]  # base.py:97
    near_s = reduce(np.minimum, dist, np.full(n, O.FARAWAY))
    vis = None if prune is None else prune.visible(ox, oy, oz, dx, dy, dz, near_s)
    tt, num, tu, tv, share = nearest_triangle(g, ox, oy, oz, dx, dy, dz, vis)
    if prune is not None:  # ... and with the tightest limit of a walk: the group's own nearest distance
        vis = prune.visible(ox, oy, oz, dx, dy, dz, np.minimum(near_s, tt))
        tt, num, tu, tv, share = nearest_triangle(g, ox, oy, oz, dx, dy, dz, vis)
    nearest = np.minimum(near_s, tt)  # base.py:98
    col = [np.zeros(n), np.zeros(n), np.zeros(n)]  # base.py:100
    on_tri = (nearest != O.FARAWAY) & (tt == nearest)
    if counts is not None:
        counts.rays += n
        counts.ties += int((on_tri & (near_s == nearest)).sum())
        counts.tri_ties += int((on_tri & (share > 1)).sum())
        if level == 0:
            counts.tri_primary += int((on_tri & (near_s != nearest)).sum())
        if parent == "sphere":
            counts.sphere_to_tri += int(on_tri.sum())
        if parent == "tri":
            counts.tri_to_sphere += int(((nearest != O.FARAWAY) & (near_s == nearest)).sum())
    bounded = level < max_bounces
    cpx, cpy, cpz = scene.cam
    hits = [(si, sp, (nearest != O.FARAWAY) & (d == nearest)) for si, (sp, d) in enumerate(zip(scene.spheres, dist))]
    hits.append((-1, None, on_tri))  # the group shades after the spheres
    for si, sp, hit in hits:
        if not np.any(hit):  # base.py:105
            continue
        idx = np.nonzero(hit)[0]
        sub = (lambda a: a if np.ndim(a) == 0 else a[idx])  # noqa: E731
        hx, hy, hz, hdx, hdy, hdz, t = sub(ox), sub(oy), sub(oz), dx[idx], dy[idx], dz[idx], nearest[idx]
        m = idx.shape[0]
        px, py, pz = hx + hdx * t, hy + hdy * t, hz + hdz * t  # shader.py:73
        if sp is not None:
            inv_r = 1.0 / sp.radius
            nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r  # :74
            gx, gy, gz = nx, ny, nz
            mats, which = [sp], np.zeros(m, dtype=np.int64)
        else:
            r = num[idx]
            flip = np.where(O._dot(g.ng[r, 0], g.ng[r, 1], g.ng[r, 2], hdx, hdy, hdz) > 0, -1.0, 1.0)
            gx, gy, gz = g.ng[r, 0] * flip, g.ng[r, 1] * flip, g.ng[r, 2] * flip
            u, v = tu[idx], tv[idx]
            w0 = (1.0 - u) - v
            sx, sy, sz = ((w0 * g.n0[r, c] + u * g.n1[r, c]) + v * g.n2[r, c] for c in range(3))
            sx, sy, sz = O._norm(sx, sy, sz)
            back = np.where(O._dot(sx, sy, sz, gx, gy, gz) < 0, -1.0, 1.0)
            smooth = g.smooth[r]
            nx, ny, nz = (np.where(smooth, s * back, f) for s, f in ((sx, gx), (sy, gy), (sz, gz)))
            mats, which = g.mats, g.mesh[r]
            if counts is not None:
                counts.smooth_hits += int(smooth.sum())
        vx, vy, vz = O._norm(cpx - px, cpy - py, cpz - pz)  # :76
        qx, qy, qz = px + gx * 0.0001, py + gy * 0.0001, pz + gz * 0.0001  # :77 (the face normal)
        for mi, mat in enumerate(mats):  # (one material at a time: the oracle's pieces take one)
            sel = np.nonzero(which == mi)[0]
            if sel.size == 0:
                continue
            s2 = (lambda a: a[sel])  # noqa: E731
            part = _shade(scene, g, table, si, mat, mi if sp is None else -1,
                          tuple(s2(a) for a in (px, py, pz)), tuple(s2(a) for a in (nx, ny, nz)),
                          tuple(s2(a) for a in (qx, qy, qz)), tuple(s2(a) for a in (vx, vy, vz)),
                          tuple(s2(a) for a in (hdx, hdy, hdz)), max_bounces, bounded, counts, level, prune)
            for c in range(3):
                col[c][idx[sel]] = col[c][idx[sel]] + part[c]  # base.py:119 (scene order)
    return col


def _shade(scene, g, table, si, mat, mesh_i, P, N, Q, V, D, max_bounces, bounded, counts, level, prune):
    """NumpyShader.create (shader.py:63-112) of hits on sphere ``si`` (or, si == -1, on triangles of mesh
    ``mesh_i``) with material ``mat``, summed over the lights as tests/lights_ref.py sums them."""
    (px, py, pz), (nx, ny, nz), (qx, qy, qz), (vx, vy, vz), (hdx, hdy, hdz) = P, N, Q, V, D
    m = px.shape[0]
    if mat.checker:
        mask = O._checker_mask(px, pz)
        tex = (1 * mask, 1 * mask, 1 * mask)
    else:
        tex = mat.tex
    gain, dg = mat.specular_gain, mat.diffuse_gain
    lits, specs = [], []
    diffuse = [np.zeros(m) for _ in range(3)]
    reach = [np.zeros(m) for _ in range(3)]  # sum_i lit_i * e_i
    for row in table:
        lx, ly, lz = O._norm(row[0] - px, row[1] - py, row[2] - pz)  # :75
        light_d = [O.intersect(o, qx, qy, qz, lx, ly, lz) for o in scene.spheres]  # :126
        tself = light_d[si] if si >= 0 else np.full(m, O.FARAWAY)
        vis = None if prune is None else prune.visible(qx, qy, qz, lx, ly, lz, tself)
        tri_d, per_mesh = _min_by_mesh(g, qx, qy, qz, lx, ly, lz, vis)
        sph_d = reduce(np.minimum, light_d, np.full(m, O.FARAWAY))
        lit = tself == np.minimum(sph_d, tri_d)  # :127-128 with the triangles taking part
        if counts is not None:
            if si >= 0:
                counts.tri_shadows_sphere += int(((tself == sph_d) & ~lit).sum())
            else:
                counts.sphere_shadows_tri += int((sph_d != O.FARAWAY).sum())
                counts.self_shadow += int((per_mesh[mesh_i] != O.FARAWAY).sum())
        dli = np.maximum(O._dot(nx, ny, nz, lx, ly, lz), 0)  # :138
        lits.append(lit)
        specs.append(O._specular(mat, nx, ny, nz, lx, ly, lz, vx, vy, vz))
        for c in range(3):
            diffuse[c] = diffuse[c] + (((tex[c] * dli) * lit) * dg) * row[3 + c]
            reach[c] = reach[c] + lit * row[3 + c]
    dome_i = 0.0
    dome_c = (1.0, 1.0, 1.0)
    for inten, dcol in scene.domes:  # shader.py:234-244 (light_direction = (0, 1, 0))
        dome_c = dcol
        dome_i += inten * np.maximum(O._dot(nx, ny, nz, 0, 1, 0), 0)
    irid = O._iridescence(mat, nx, ny, nz, vx, vy, vz)
    R = [np.zeros(m) for _ in range(3)]
    need = np.zeros(m, dtype=bool)
    if bounded and gain != 0:
        need = (reach[0] != 0) | (reach[1] != 0) | (reach[2] != 0)
    if need.any():
        dn = O._dot(hdx, hdy, hdz, nx, ny, nz)
        rx, ry, rz = O._norm(hdx - (nx * 2) * dn, hdy - (ny * 2) * dn, hdz - (nz * 2) * dn)  # :151
        child = trace(scene, g, table, (qx[need], qy[need], qz[need]), (rx[need], ry[need], rz[need]), max_bounces,
                      counts, level + 1, prune, "sphere" if si >= 0 else "tri")
        for c in range(3):
            R[c][need] = child[c]
    out = []
    for c in range(3):
        glossy = np.zeros(m)
        for row, lit, spec in zip(table, lits, specs):
            glossy = glossy + (((spec + R[c] * 0.5) * gain) * lit) * row[3 + c]
        out.append((((0.004 + diffuse[c]) + dome_c[c] * dome_i) + glossy) + irid[c])
    return out


# ---- the kernel's stack of pending rays ----------------------------------------------------------
def pushes(scene, g: Group, table, origin, dirs):
    """The reflected rays that the hits of a batch of rays send, in the order k_trace_mesh pushes them: the
    spheres at the nearest distance in scene order, then the triangle. A list of (indices into the batch,
    origins, directions); a ray appears at most once per entry. The decisions are ``trace``'s and ``_shade``'s
    (which shapes are at the nearest distance, ``specular_gain != 0`` and a light that reaches the hit),
    restated without the colours; the bounce cap is the caller's."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    n = dx.shape[0]
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]
    near_s = reduce(np.minimum, dist, np.full(n, O.FARAWAY))
    tt, num, tu, tv, _ = nearest_triangle(g, ox, oy, oz, dx, dy, dz)
    nearest = np.minimum(near_s, tt)
    hits = [(si, sp, (nearest != O.FARAWAY) & (d == nearest)) for si, (sp, d) in enumerate(zip(scene.spheres, dist))]
    hits.append((-1, None, (nearest != O.FARAWAY) & (tt == nearest)))
    out = []
    for si, sp, hit in hits:
        idx = np.nonzero(hit)[0]
        if idx.size == 0:
            continue
        sub = (lambda a: a if np.ndim(a) == 0 else a[idx])  # noqa: E731
        hx, hy, hz, hdx, hdy, hdz, t = sub(ox), sub(oy), sub(oz), dx[idx], dy[idx], dz[idx], nearest[idx]
        px, py, pz = hx + hdx * t, hy + hdy * t, hz + hdz * t
        if sp is not None:
            inv_r = 1.0 / sp.radius
            nx, ny, nz = (px - sp.cx) * inv_r, (py - sp.cy) * inv_r, (pz - sp.cz) * inv_r
            gx, gy, gz = nx, ny, nz
            gains = np.full(idx.size, sp.specular_gain)
        else:
            r = num[idx]
            flip = np.where(O._dot(g.ng[r, 0], g.ng[r, 1], g.ng[r, 2], hdx, hdy, hdz) > 0, -1.0, 1.0)
            gx, gy, gz = g.ng[r, 0] * flip, g.ng[r, 1] * flip, g.ng[r, 2] * flip
            u, v = tu[idx], tv[idx]
            w0 = (1.0 - u) - v
            sx, sy, sz = ((w0 * g.n0[r, c] + u * g.n1[r, c]) + v * g.n2[r, c] for c in range(3))
            sx, sy, sz = O._norm(sx, sy, sz)
            back = np.where(O._dot(sx, sy, sz, gx, gy, gz) < 0, -1.0, 1.0)
            nx, ny, nz = (np.where(g.smooth[r], s * back, f) for s, f in ((sx, gx), (sy, gy), (sz, gz)))
            gains = np.array([m.specular_gain for m in g.mats], dtype=np.float64)[g.mesh[r]]
        qx, qy, qz = px + gx * 0.0001, py + gy * 0.0001, pz + gz * 0.0001
        reach = [np.zeros(idx.size) for _ in range(3)]
        for row in table:
            lx, ly, lz = O._norm(row[0] - px, row[1] - py, row[2] - pz)
            light_d = [O.intersect(o, qx, qy, qz, lx, ly, lz) for o in scene.spheres]
            tself = light_d[si] if si >= 0 else np.full(idx.size, O.FARAWAY)
            tri_d, _ = _min_by_mesh(g, qx, qy, qz, lx, ly, lz)
            lit = tself == np.minimum(reduce(np.minimum, light_d, np.full(idx.size, O.FARAWAY)), tri_d)
            for c in range(3):
                reach[c] = reach[c] + lit * row[3 + c]
        need = (gains != 0) & ((reach[0] != 0) | (reach[1] != 0) | (reach[2] != 0))
        if need.any():
            dn = O._dot(hdx, hdy, hdz, nx, ny, nz)
            rx, ry, rz = O._norm(hdx - (nx * 2) * dn, hdy - (ny * 2) * dn, hdz - (nz * 2) * dn)
            out.append((idx[need], (qx[need], qy[need], qz[need]), (rx[need], ry[need], rz[need])))
    return out


def pending_need(scene, g: Group, table, origin, dirs, max_bounces, level=0):
    """Per ray, the largest number of pending rays that k_trace_mesh's depth-first walk would hold with an
    unbounded stack (the kernel's holds 2 * max_bounces + 2; a lane that needs more drops rays and reports
    RTX_ST_STACK_OVERFLOW). Arguments as ``trace``; an int64 array, at least 1: the ray itself.

    The walk pops a ray, shades its hits one per round (``pushes``' order) and, when level < max_bounces,
    each hit pushes at most one ray; it pops the last pushed first and finishes that ray's whole tree before
    the next. So the j-th ray a node pushed (from 0) is popped with j siblings still below it, and a node
    needs max(1, max_j (j + need of its j-th child)) entries, itself included (tests/glass_ref.py's
    recursion). With k + 1 shapes at the nearest distance on every level that is max_bounces * k + 1."""
    n = np.asarray(dirs[0]).shape[0]
    need = np.ones(n, dtype=np.int64)
    if level >= max_bounces or n == 0:  # the next level is black: nothing is pushed
        return need
    pushed = np.zeros(n, dtype=np.int64)
    for rays, o2, d2 in pushes(scene, g, table, origin, dirs):
        child = pending_need(scene, g, table, o2, d2, max_bounces, level + 1)
        need[rays] = np.maximum(need[rays], pushed[rays] + child)
        pushed[rays] += 1
    return need


def table_of(spec):
    """The lights table of ``spec`` as the renderer builds it: every point light (lights.lights_table)
    if one of them has an intensity or a colour, else the one row (lights[0], 1, 1, 1)."""
    points = [li for li in spec["lights"] if li["kind"] == "point"]
    if not any("intensity" in li or "color" in li for li in points):
        points = points[:1]
    rows = []
    for li in points:
        inten = float(li.get("intensity", 1.0))
        rows.append([float(x) for x in li["position"]] + [inten * float(c) for c in li.get("color", (1.0, 1.0, 1.0))])
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 6)


def render(spec, max_bounces=3, rows=None, counts=None, prune=None):
    """The frame of ``spec`` (or its rows ``rows``, global indices in the given order): float64 [3, n]."""
    scene = O.scene_from_spec(spec)
    if rows is None:
        d = O.ray_directions(scene.cam, scene.width, scene.height)
    else:
        d = O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)
    return np.stack(trace(scene, group_of(spec), table_of(spec), tuple(float(c) for c in scene.cam), d, max_bounces,
                          counts, 0, prune))


def trace_rays(spec, origin, dirs, max_bounces=3, counts=None):
    """Explicit rays through ``spec``'s scene: ``origin`` three scalars or arrays, ``dirs`` three arrays."""
    scene = O.scene_from_spec(spec)
    return np.stack(trace(scene, group_of(spec), table_of(spec), origin, dirs, max_bounces, counts))
