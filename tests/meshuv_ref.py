"""NumPy restatement of image textures on meshes (rtx_trace_mesh_uv).

tests/mesh_ref.py with one more step: a hit on a triangle whose mesh has an image texture takes its
texture colour from the image at the hit's texture coordinates, in the arithmetic of include/rtx_hip.h,
float64, operation for operation:

    w0 = (1 - u) - v;  s = (w0*s0 + u*s1) + v*s2;  t = (w0*t0 + u*t1) + v*t2
    x = s*W - 0.5;  y = (1 - t)*H - 0.5;  x0 = floor(x);  fx = x - x0;  y0 = floor(y);  fy = y - y0
    i0 = x0 - W*floor(x0/W);  i1 = 0 if i0 + 1 == W else i0 + 1      (j0, j1 likewise with H)
    c = (c[j0][i0]*(1 - fx) + c[j0][i1]*fx)*(1 - fy) + (c[j1][i0]*(1 - fx) + c[j1][i1]*fx)*fy

mesh_ref's ``_shade`` takes its texture colour from the material alone and has no seam for a colour per
hit, so ``trace`` and ``_shade`` are restated here with that step; the triangle tests, the group's nearest
hit, the shadow distances and the tree's emulated pruning are mesh_ref's own functions. Every triangle is
tried for every ray. A sphere with an image texture takes the oracle's texel (O.image_texels). Where no
mesh has an image the frames are mesh_ref's, bit for bit (tests/test_meshuv_cpu.py).
"""

from dataclasses import dataclass, field
from functools import reduce

import numpy as np

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from tests import mesh_ref as R


@dataclass
class Counts(R.Counts):
    """mesh_ref's counters, and what the image lookups of a frame cover."""

    tex_primary: int = 0  # level-0 hits on a triangle of an image-textured mesh
    tex_reflected: int = 0  # such hits at level >= 1
    wrapped_x: int = 0  # lookups one of whose two columns was wrapped (x0 or x0 + 1 outside 0..W-1)
    wrapped_y: int = 0  # ... one of whose two rows was wrapped
    negative: int = 0  # lookups at a negative x or y
    fractional: int = 0  # lookups with fx != 0 or fy != 0
    seam_hits: int = 0  # textured hits on a triangle one of whose coordinates is 1 exactly (a seam segment's end)
    meshes_hit: set = field(default_factory=set)  # the image-textured meshes that were hit


@dataclass
class UvGroup:
    """mesh_ref's group, the rows' texture coordinates [T, 6] and every mesh's image ([H, W, 3] or None)."""

    g: R.Group
    uvs: np.ndarray
    images: list


def group_of(spec) -> UvGroup:
    g = R.group_of(spec)
    uvs, images = [], []
    for m in spec["meshes"]:
        mesh = scenes.mesh_of(m)
        F = len(mesh.faces)
        uvs.append(np.zeros((F, 6)) if mesh.uvs is None else np.asarray(mesh.uvs, dtype=np.float64).reshape(F, 6))
        tex = m["shader"]["texture"]
        images.append(np.asarray(tex["texels"], dtype=np.float64)[:, :, :3] if tex["kind"] == "image" else None)
    return UvGroup(g, np.concatenate(uvs), images)


def lookup(image, st, u, v, counts=None):
    """The image's colour (three arrays) at (u, v) of triangles with the coordinates ``st`` [m, 6]."""
    H, W = float(image.shape[0]), float(image.shape[1])
    w0 = (1.0 - u) - v
    s = (w0 * st[:, 0] + u * st[:, 2]) + v * st[:, 4]
    t = (w0 * st[:, 1] + u * st[:, 3]) + v * st[:, 5]
    x = s * W - 0.5
    y = (1.0 - t) * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    i0 = x0 - W * np.floor(x0 / W)
    j0 = y0 - H * np.floor(y0 / H)
    i1 = np.where(i0 + 1.0 == W, 0.0, i0 + 1.0)
    j1 = np.where(j0 + 1.0 == H, 0.0, j0 + 1.0)
    assert ((i0 >= 0) & (i0 < W) & (j0 >= 0) & (j0 < H)).all()
    a0, a1, b0, b1 = (a.astype(np.int64) for a in (i0, i1, j0, j1))
    if counts is not None:
        counts.wrapped_x += int(((x0 < 0) | (x0 + 1.0 >= W)).sum())
        counts.wrapped_y += int(((y0 < 0) | (y0 + 1.0 >= H)).sum())
        counts.negative += int(((x < 0) | (y < 0)).sum())
        counts.fractional += int(((fx != 0) | (fy != 0)).sum())
    gx, gy = 1.0 - fx, 1.0 - fy
    return tuple((image[b0, a0, c] * gx + image[b0, a1, c] * fx) * gy + (image[b1, a0, c] * gx + image[b1, a1, c] * fx) * fy
                 for c in range(3))


def trace(scene, ug: UvGroup, table, origin, dirs, max_bounces, counts=None, level=0, prune=None, parent=None):
    """mesh_ref.trace with a texture colour per hit (the same text up to the call of ``_shade``)."""
    g = ug.g
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = (np.asarray(d, dtype=np.float64) for d in dirs)
    ox, oy, oz = origin
    n = dx.shape[0]
    dist = [O.intersect(sp, ox, oy, oz, dx, dy, dz) for sp in scene.spheres]  # base.py:97
    near_s = reduce(np.minimum, dist, np.full(n, O.FARAWAY))
    vis = None if prune is None else prune.visible(ox, oy, oz, dx, dy, dz, near_s)
    tt, num, tu, tv, share = R.nearest_triangle(g, ox, oy, oz, dx, dy, dz, vis)
    if prune is not None:
        vis = prune.visible(ox, oy, oz, dx, dy, dz, np.minimum(near_s, tt))
        tt, num, tu, tv, share = R.nearest_triangle(g, ox, oy, oz, dx, dy, dz, vis)
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
        u = v = r = None
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
            tex = None  # the material's own: a constant or the checker
            if sp is None and ug.images[mi] is not None:  # the image at the hit's texture coordinates
                st = ug.uvs[r[sel]]
                tex = lookup(ug.images[mi], st, u[sel], v[sel], counts)
                if counts is not None:
                    counts.tex_primary += sel.size if level == 0 else 0
                    counts.tex_reflected += sel.size if level > 0 else 0
                    counts.seam_hits += int((st == 1.0).any(axis=1).sum())
                    counts.meshes_hit.add(mi)
            part = _shade(scene, ug, table, si, mat, mi if sp is None else -1, tex,
                          tuple(s2(a) for a in (px, py, pz)), tuple(s2(a) for a in (nx, ny, nz)),
                          tuple(s2(a) for a in (qx, qy, qz)), tuple(s2(a) for a in (vx, vy, vz)),
                          tuple(s2(a) for a in (hdx, hdy, hdz)), max_bounces, bounded, counts, level, prune)
            for c in range(3):
                col[c][idx[sel]] = col[c][idx[sel]] + part[c]  # base.py:119 (scene order)
    return col


def _shade(scene, ug, table, si, mat, mesh_i, tex, P, N, Q, V, D, max_bounces, bounded, counts, level, prune):
    """mesh_ref._shade with the texture's colour ``tex`` given per hit (None: the material's own; a sphere
    with an image takes the oracle's texel)."""
    g = ug.g
    (px, py, pz), (nx, ny, nz), (qx, qy, qz), (vx, vy, vz), (hdx, hdy, hdz) = P, N, Q, V, D
    m = px.shape[0]
    if tex is not None:
        pass
    elif mat.checker:
        mask = O._checker_mask(px, pz)
        tex = (1 * mask, 1 * mask, 1 * mask)
    elif si >= 0 and mat.image is not None:
        tex = O.image_texels(mat, px, py, pz)
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
        tri_d, per_mesh = R._min_by_mesh(g, qx, qy, qz, lx, ly, lz, vis)
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
    R_ = [np.zeros(m) for _ in range(3)]
    need = np.zeros(m, dtype=bool)
    if bounded and gain != 0:
        need = (reach[0] != 0) | (reach[1] != 0) | (reach[2] != 0)
    if need.any():
        dn = O._dot(hdx, hdy, hdz, nx, ny, nz)
        rx, ry, rz = O._norm(hdx - (nx * 2) * dn, hdy - (ny * 2) * dn, hdz - (nz * 2) * dn)  # :151
        child = trace(scene, ug, table, (qx[need], qy[need], qz[need]), (rx[need], ry[need], rz[need]), max_bounces,
                      counts, level + 1, prune, "sphere" if si >= 0 else "tri")
        for c in range(3):
            R_[c][need] = child[c]
    out = []
    for c in range(3):
        glossy = np.zeros(m)
        for row, lit, spec in zip(table, lits, specs):
            glossy = glossy + (((spec + R_[c] * 0.5) * gain) * lit) * row[3 + c]
        out.append((((0.004 + diffuse[c]) + dome_c[c] * dome_i) + glossy) + irid[c])
    return out


def render(spec, max_bounces=3, rows=None, counts=None, prune=None):
    """The frame of ``spec`` (or its rows ``rows``, global indices in the given order): float64 [3, n]."""
    scene = O.scene_from_spec(spec)
    if rows is None:
        d = O.ray_directions(scene.cam, scene.width, scene.height)
    else:
        d = O.ray_directions_rows(scene.cam, scene.width, scene.height, rows)
    return np.stack(trace(scene, group_of(spec), R.table_of(spec), tuple(float(c) for c in scene.cam), d, max_bounces,
                          counts, 0, prune))


def trace_rays(spec, origin, dirs, max_bounces=3, counts=None):
    """Explicit rays through ``spec``'s scene: ``origin`` three scalars or arrays, ``dirs`` three arrays."""
    scene = O.scene_from_spec(spec)
    return np.stack(trace(scene, group_of(spec), R.table_of(spec), origin, dirs, max_bounces, counts))
