"""Host maths of triangle meshes (``rtx_trace_mesh``): the routing rule, an OBJ loader,
a few generators, the triangle test in NumPy and the device table with its bounding-volume tree.

A scene is a mesh scene if and only if ``scene.shapes`` holds at least one ``domain.TriangleMesh``.
The triangles of every mesh form one group, numbered in scene order, then face order; the table holds
them in the tree's leaf order, each with its number. Nothing here touches the GPU: a bad value raises
ValueError before any device call.
"""

from __future__ import annotations

import hashlib
from typing import NamedTuple

import numpy as np

from python_ray_tracer_amd.domain import TriangleMesh

FARAWAY = 1.0e39
MAX_TRIANGLES = 1 << 20  # RTX_MAX_TRIANGLES
MAX_BOUNCES = 16  # RTX_MESH_MAX_BOUNCES
MAGIC = 1296388936.0  # RTX_MESH_MAGIC
HDR_WORDS = 16  # RTX_MESH_HDR_WORDS
# header words (RTX_MH_*)
MH_MAGIC, MH_NTRI, MH_NMESH, MH_NNODES, MH_TRIS, MH_MATS, MH_NODES, MH_WORDS = range(8)
# ... of a table with image textures (rtx_trace_mesh_uv): the word offsets of the UV part and
# of the texel blocks, 0 in a table without them
MH_UVS, MH_TEXELS = 8, 9
UV_WORDS = 6  # RTX_UV_WORDS: s0 t0 s1 t1 s2 t2 per triangle row
UV_MAX = 1024.0  # RTX_MESH_UV_MAX: the largest |s|, |t| (the lookup's indices stay exact ints)
MAX_TEXELS = 1 << 20  # RTX_MAX_TEXELS
TRI_WORDS = 24  # RTX_TRI_WORDS
# triangle row words (RTX_T_*): v0, e1 = v1 - v0, e2 = v2 - v0, the unit face normal, the mesh, 1 for
# vertex normals, the three vertex normals, the triangle's number in the group
T_V0, T_E1, T_E2, T_NG, T_MESH, T_SMOOTH, T_N0, T_N1, T_N2, T_NUM = 0, 3, 6, 9, 12, 13, 14, 17, 20, 23
MARGIN = 2e-7  # a node's margin is MARGIN * (1 + the largest |corner|^2), DESIGN.md §17


def is_mesh_scene(shapes) -> bool:
    """Whether ``shapes`` holds a ``TriangleMesh`` (nothing is validated)."""
    return any(isinstance(sh, TriangleMesh) for sh in shapes)


def shape_ids(shapes) -> np.ndarray:
    """What rtx_mesh_aovs' ``id`` pass reports (its ``shape_ids``), int32: the indices in ``shapes`` of the
    shapes that are no ``TriangleMesh`` (the spheres, in the packer's order), then those of the meshes (in
    the table's order)."""
    meshes = [i for i, sh in enumerate(shapes) if isinstance(sh, TriangleMesh)]
    others = [i for i, sh in enumerate(shapes) if not isinstance(sh, TriangleMesh)]
    return np.asarray(others + meshes, dtype=np.int32)


def triangle_faces(shapes, numbers) -> tuple:
    """(shape_index, face_index), int64 arrays shaped like ``numbers``: for every triangle number of the
    scene's group (the ``triangle`` pass of render_mesh_aovs: scene order, then face order) the index in
    ``shapes`` of the mesh that owns it and the face's index in that mesh's ``faces``; -1 and -1 where the
    number is -1. ValueError for a number outside -1..T - 1."""
    num = np.asarray(numbers)
    if not np.issubdtype(num.dtype, np.integer):
        raise ValueError(f"triangle_faces: numbers must be integers, got {num.dtype}")
    num = num.astype(np.int64)
    where = [i for i, sh in enumerate(shapes) if isinstance(sh, TriangleMesh)]
    ends = np.cumsum([len(shapes[i].faces) for i in where], dtype=np.int64)  # the first number after each mesh
    total = int(ends[-1]) if len(where) else 0
    if num.size and (num.min() < -1 or num.max() >= total):
        raise ValueError(f"triangle_faces: a number lies outside -1..{total - 1} (the scene has {total} triangles)")
    hit = num >= 0
    mesh = np.searchsorted(ends, np.where(hit, num, 0), side="right")
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64) if len(where) else np.zeros(0, dtype=np.int64)
    if not len(where):
        return np.full(num.shape, -1, dtype=np.int64), np.full(num.shape, -1, dtype=np.int64)
    shape_index = np.where(hit, np.asarray(where, dtype=np.int64)[mesh], -1)
    face_index = np.where(hit, num - starts[mesh], -1)
    return shape_index, face_index


def check_bounces(max_bounces) -> int:
    """The bounce cap of a mesh render: an int in 0..MAX_BOUNCES. ValueError for None (the kernel keeps
    a lane's pending rays in a stack sized by the cap) and for a larger cap."""
    if max_bounces is None:
        raise ValueError("a scene with a TriangleMesh needs a finite bounce cap: "
                         f"HipRenderer(max_bounces=B) with B in 0..{MAX_BOUNCES}")
    if isinstance(max_bounces, bool) or int(max_bounces) != max_bounces or not 0 <= max_bounces <= MAX_BOUNCES:
        raise ValueError(f"a scene with a TriangleMesh renders with HipRenderer(max_bounces=B), B in "
                         f"0..{MAX_BOUNCES}, got {max_bounces!r}")
    return int(max_bounces)


# ---------------------------------------------------------------------------------------------
# the triangle test
# ---------------------------------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def intersect_triangles(v0, e1, e2, ox, oy, oz, dx, dy, dz):
    """The two-sided Möller–Trumbore test of include/rtx_hip.h for triangles [F] (``v0``, ``e1``, ``e2``
    float64 [F, 3]) against rays [n]: (t, u, v) float64 [F, n], t FARAWAY where the ray misses."""
    ox, oy, oz, dx, dy, dz = (np.asarray(a, dtype=np.float64).reshape(1, -1) for a in (ox, oy, oz, dx, dy, dz))
    c = [np.ascontiguousarray(a[:, i]).reshape(-1, 1) for a in (v0, e1, e2) for i in range(3)]
    v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z = c
    with np.errstate(all="ignore"):
        tx, ty, tz = ox - v0x, oy - v0y, oz - v0z
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = _dot(e1x, e1y, e1z, px, py, pz)
        f = 1.0 / det
        u = f * _dot(tx, ty, tz, px, py, pz)
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        v = f * _dot(dx, dy, dz, qx, qy, qz)
        t = f * _dot(e2x, e2y, e2z, qx, qy, qz)
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < FARAWAY)
    return np.where(hit, t, FARAWAY), u, v


def intersect_mesh(mesh, ray_origin, ray_direction):
    """``TriangleMesh.intersect``: the smallest t over the mesh's faces per ray (FARAWAY: a miss)."""
    v, f = mesh.vertices, mesh.faces
    v0 = v[f[:, 0]]
    d = [np.atleast_1d(np.asarray(c, dtype=np.float64)) for c in _components(ray_direction)]
    n = max(a.size for a in d)
    o = [np.broadcast_to(np.asarray(c, dtype=np.float64), (n,)) for c in _components(ray_origin)]
    d = [np.broadcast_to(a, (n,)) for a in d]
    best = np.full(n, FARAWAY)
    for k in range(0, len(f), 4096):  # (blocks: the [F, n] intermediates stay small)
        s = slice(k, k + 4096)
        t, _, _ = intersect_triangles(v0[s], v[f[s, 1]] - v0[s], v[f[s, 2]] - v0[s], *o, *d)
        best = np.minimum(best, t.min(axis=0))
    return best


def _components(v):
    return v.components() if hasattr(v, "components") else tuple(v)


# ---------------------------------------------------------------------------------------------
# OBJ files and generators
# ---------------------------------------------------------------------------------------------
def vertex_normals(vertices, faces) -> np.ndarray:
    """Area-weighted vertex normals [V, 3]: the sum of the faces' (unnormalised) cross products at each
    vertex, normalised (a vertex of no face, or whose faces cancel: the zero vector)."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = np.zeros_like(v)
    for i in range(3):
        np.add.at(out, f[:, i], fn)
    mag = np.sqrt((out * out).sum(axis=1, keepdims=True))
    return out / np.where(mag == 0, 1.0, mag)


def load_obj(path, shader, smooth: bool = False) -> TriangleMesh:
    """The mesh of a Wavefront OBJ file: ``v``, ``vn`` and ``vt`` records, ``f`` records with ``v``, ``v/vt``,
    ``v//vn`` and ``v/vt/vn`` indices (1-based, or negative: counted back from the latest record),
    polygons fan-triangulated from their first corner; comments and every other record are ignored.
    ``uvs`` (per corner, the first two numbers of a ``vt``) are kept if every corner of every face names a
    ``vt`` that exists, else the mesh has none.
    ``smooth``: with vertex normals, the file's ``vn`` where every corner names one (a vertex that
    several corners give different normals is split), else area-weighted ones (``vertex_normals``).
    ValueError for a record that does not parse and for an index out of range."""
    verts, norms, corners, faces = [], [], {}, []
    out_v, out_n = [], []
    any_vn, all_vn = False, True
    texs, face_uvs, all_vt = [], [], True

    def index(tok: str, count: int, what: str, line_no: int) -> int:
        try:
            i = int(tok)
        except ValueError:
            raise ValueError(f"{path}:{line_no}: bad {what} index {tok!r}") from None
        j = i - 1 if i > 0 else count + i
        if i == 0 or not 0 <= j < count:
            raise ValueError(f"{path}:{line_no}: {what} index {i} out of range (1..{count})")
        return j

    with open(path, encoding="utf-8", errors="replace") as fh:
        for line_no, line in enumerate(fh, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            if parts[0] in ("v", "vn"):
                try:
                    xyz = [float(x) for x in parts[1:4]]
                except ValueError:
                    raise ValueError(f"{path}:{line_no}: bad {parts[0]} record") from None
                if len(xyz) != 3:
                    raise ValueError(f"{path}:{line_no}: a {parts[0]} record needs three numbers")
                (verts if parts[0] == "v" else norms).append(xyz)
            elif parts[0] == "vt":  # (never an error: a record that does not parse leaves the mesh without uvs)
                try:
                    st = [float(x) for x in parts[1:3]]
                except ValueError:
                    st = []
                texs.append(st if len(st) == 2 else None)
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{line_no}: a face needs at least three corners")
                poly, poly_uv = [], []
                for tok in parts[1:]:
                    fields = tok.split("/")
                    vi = index(fields[0], len(verts), "vertex", line_no)
                    st = None
                    if len(fields) >= 2 and fields[1].lstrip("-").isdigit() and int(fields[1]) != 0:
                        ti = int(fields[1])
                        ti = ti - 1 if ti > 0 else len(texs) + ti
                        st = texs[ti] if 0 <= ti < len(texs) else None
                    all_vt = all_vt and st is not None
                    poly_uv.append(st)
                    ni = None
                    if len(fields) >= 3 and fields[2] != "":
                        ni = index(fields[2], len(norms), "normal", line_no)
                        any_vn = True
                    else:
                        all_vn = False
                    key = (vi, ni)
                    if key not in corners:
                        corners[key] = len(out_v)
                        out_v.append(verts[vi])
                        out_n.append(norms[ni] if ni is not None else (0.0, 0.0, 0.0))
                    poly.append(corners[key])
                faces += [(poly[0], poly[i], poly[i + 1]) for i in range(1, len(poly) - 1)]
                face_uvs += [(poly_uv[0], poly_uv[i], poly_uv[i + 1]) for i in range(1, len(poly) - 1)]
    use_vn = smooth and any_vn and all_vn
    if not use_vn:  # the file's vertices in the file's order: corners that differ in their normal alone are one
        remap = np.zeros(len(out_v), dtype=np.int64)
        for (vi, _ni), k in corners.items():
            remap[k] = vi
        out_v = verts
        faces = remap[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    v = np.asarray(out_v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    normals = None
    if use_vn:
        normals = np.asarray(out_n, dtype=np.float64).reshape(-1, 3)
    elif smooth:
        normals = vertex_normals(v, f)
    uvs = np.asarray(face_uvs, dtype=np.float64).reshape(-1, 3, 2) if all_vt and face_uvs else None
    return TriangleMesh(v, f, shader, normals, uvs)


_QUAD_UV = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], dtype=np.float64)  # faces (0,1,2), (0,2,3)


def quad(corners, shader, uv: bool = False) -> TriangleMesh:
    """Two triangles (0, 1, 2) and (0, 2, 3) over four corners given in order round the quad. ``uv``: the
    corners get the texture coordinates (0, 0), (1, 0), (1, 1), (0, 1)."""
    c = np.asarray(corners, dtype=np.float64).reshape(4, 3)
    return TriangleMesh(c, [(0, 1, 2), (0, 2, 3)], shader, None, _QUAD_UV if uv else None)


def box(lo, hi, shader, uv: bool = False) -> TriangleMesh:
    """The axis-aligned box from ``lo`` to ``hi``: 8 vertices, 12 triangles, normals outwards. ``uv``: every
    face gets the texture coordinates 0..1, as ``quad`` gives them to its corners in the face's order."""
    (x0, y0, z0), (x1, y1, z1) = (tuple(float(x) for x in lo), tuple(float(x) for x in hi))
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    q = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return TriangleMesh(v, f, shader, None, np.tile(_QUAD_UV, (6, 1, 1)) if uv else None)


def icosphere(level: int, shader, smooth: bool = False) -> TriangleMesh:
    """The unit sphere about the origin as an icosahedron subdivided ``level`` times (each triangle
    into four, the new vertices pushed onto the sphere): 20 * 4**level triangles. ``smooth``: the
    vertex normals are the vertices themselves."""
    if isinstance(level, bool) or int(level) != level or not 0 <= level <= 7:
        raise ValueError(f"icosphere: level must be an int in 0..7, got {level!r}")
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
                  (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)], dtype=np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
                  (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
                  (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    for _ in range(int(level)):
        nv = len(v)
        edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.sqrt((mid * mid).sum(axis=1, keepdims=True))
        v = np.concatenate([v, mid])
        m = nv + inv.reshape(3, -1)  # the midpoints of edges (0,1), (1,2), (2,0) per face
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([b, m[1], m[0]], 1),
                            np.stack([c, m[2], m[1]], 1), np.stack([m[0], m[1], m[2]], 1)])
    return TriangleMesh(v, f, shader, v.copy() if smooth else None)


def torus(R: float, r: float, nu: int, nv: int, shader, smooth: bool = False, uv: bool = False) -> TriangleMesh:
    """A torus about the y axis through the origin: ``R`` the radius of the tube's centre circle, ``r``
    the tube's, ``nu`` segments round the axis and ``nv`` round the tube: 2 * nu * nv triangles.
    ``smooth``: the vertex normals point from the tube's centre circle. ``uv``: texture coordinates per
    corner, s = i / nu round the axis and t = j / nv round the tube; the last segment ends at 1, not 0 (the
    seam needs no split vertex)."""
    if int(nu) != nu or int(nv) != nv or nu < 3 or nv < 3:
        raise ValueError(f"torus: nu and nv must be ints >= 3, got {nu!r} and {nv!r}")
    nu, nv = int(nu), int(nv)
    a = (np.arange(nu) * (2.0 * np.pi / nu)).reshape(-1, 1)
    b = (np.arange(nv) * (2.0 * np.pi / nv)).reshape(1, -1)
    n = np.stack([np.cos(b) * np.cos(a), np.sin(b) * np.ones_like(a), np.cos(b) * np.sin(a)], axis=-1).reshape(-1, 3)
    centre = np.stack([np.cos(a) * np.ones_like(b), np.zeros((nu, nv)), np.sin(a) * np.ones_like(b)], axis=-1)
    v = float(R) * centre.reshape(-1, 3) + float(r) * n
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    p00, p10, p11, p01 = (i * nv + j).ravel(), (i1 * nv + j).ravel(), (i1 * nv + j1).ravel(), (i * nv + j1).ravel()
    f = np.concatenate([np.stack([p00, p11, p10], 1), np.stack([p00, p01, p11], 1)])
    uvs = None
    if uv:
        s0, s1, t0, t1 = (i / nu).ravel(), ((i + 1) / nu).ravel(), (j / nv).ravel(), ((j + 1) / nv).ravel()
        st = lambda a, b: np.stack([a, b], 1)  # noqa: E731
        uvs = np.concatenate([np.stack([st(s0, t0), st(s1, t1), st(s1, t0)], 1),
                              np.stack([st(s0, t0), st(s0, t1), st(s1, t1)], 1)])
    return TriangleMesh(v, f, shader, n if smooth else None, uvs)


# ---------------------------------------------------------------------------------------------
# the device table
# ---------------------------------------------------------------------------------------------
def _mesh_arrays(mesh, i: int):
    """(vertices [V, 3], faces [F, 3], normals or None) of mesh ``i``, validated."""
    v = np.asarray(mesh.vertices, dtype=np.float64)
    f = np.asarray(mesh.faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"mesh {i}: vertices must be [V, 3], got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"mesh {i}: faces must be int [F, 3], got {f.dtype} {f.shape}")
    if f.shape[0] == 0:
        raise ValueError(f"mesh {i}: no faces")
    if not np.isfinite(v).all():
        raise ValueError(f"mesh {i}: a vertex is not finite")
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError(f"mesh {i}: a face index lies outside 0..{v.shape[0] - 1}")
    n = mesh.normals
    if n is not None:
        n = np.asarray(n, dtype=np.float64)
        if n.shape != v.shape:
            raise ValueError(f"mesh {i}: normals must be [V, 3] like the vertices {v.shape}, got {n.shape}")
        if not np.isfinite(n).all():
            raise ValueError(f"mesh {i}: a vertex normal is not finite")
    return v, f.astype(np.int64), n


def _is_image(tex) -> bool:
    return hasattr(tex, "texels")


def has_image(shapes) -> bool:
    """Whether some mesh of ``shapes`` has an ``ImageTexture``: the scene's table gets a UV part and texel
    blocks and is traced by rtx_trace_mesh_uv."""
    return any(isinstance(sh, TriangleMesh) and _is_image(getattr(sh.shader, "diffuse_color", None)) for sh in shapes)


def _mesh_uvs(mesh, i: int, F: int):
    """The texture coordinates [F, 3, 2] of mesh ``i`` (``F`` faces), validated, or None."""
    uv = getattr(mesh, "uvs", None)
    if uv is None:
        return None
    uv = np.asarray(uv, dtype=np.float64)
    if uv.shape != (F, 3, 2):
        raise ValueError(f"mesh {i}: uvs must be [F, 3, 2] per corner ({F} faces) or [V, 2] per vertex, got {uv.shape}")
    if not np.isfinite(uv).all():
        raise ValueError(f"mesh {i}: a texture coordinate (uvs) is not finite")
    if np.abs(uv).max() > UV_MAX:
        raise ValueError(f"mesh {i}: a texture coordinate (uvs) lies outside -{UV_MAX:g}..{UV_MAX:g} (RTX_MESH_UV_MAX)")
    return uv


def _mesh_image(mesh, i: int):
    """The texels float64 [H, W, 3] of mesh ``i``'s ImageTexture, validated."""
    t = np.asarray(mesh.shader.diffuse_color.texels, dtype=np.float64)
    if t.ndim != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"mesh {i}: the ImageTexture's texels must be [H, W, 3], got {t.shape}")
    if t.shape[0] * t.shape[1] > MAX_TEXELS:
        raise ValueError(f"mesh {i}: the ImageTexture has {t.shape[0] * t.shape[1]} texels, more than {MAX_TEXELS} "
                         "(RTX_MAX_TEXELS)")
    return t


def _mesh_material(mesh, i: int) -> list:
    """The material row of mesh ``i``'s shader (the spheres' record, scene_pack._material_row). An
    ImageTexture's row is RTX_TEX_IMAGE with a block offset of 0, the width and the height: ``mesh_table``
    writes the offset of the image's texel block."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L
    from python_ray_tracer_amd.infrastructure.hip.scene_pack import _material_row

    sh = mesh.shader
    tex = sh.diffuse_color
    if getattr(sh, "transmission_gain", 0.0):
        raise ValueError(f"mesh {i}: transmission_gain != 0; there is no refraction through a mesh")
    if type(tex).__name__ == "TextureChecker":
        tex_fields = (L.TEX_CHECKER, 1.0, 1.0, 1.0)
    elif _is_image(tex):
        if getattr(mesh, "uvs", None) is None:
            raise ValueError(f"mesh {i}: an ImageTexture needs texture coordinates, which this mesh does not have "
                             "(TriangleMesh(..., uvs=...))")
        t = _mesh_image(mesh, i)
        tex_fields = (L.TEX_IMAGE, None, float(t.shape[1]), float(t.shape[0]))
    elif hasattr(tex, "color"):
        tex_fields = (L.TEX_CONST, float(tex.color.x), float(tex.color.y), float(tex.color.z))
    else:
        raise ValueError(f"mesh {i}: unsupported texture {type(tex).__name__}")
    return _material_row((None, None, tex_fields, sh.specular_gain, sh.diffuse_gain, sh.specular_roughness,
                          sh.specular_ior, sh.iridescence_gain, sh.thin_film_weight, sh.thin_film_thickness,
                          sh.thin_film_ior, sh.reflection_gain))


def triangle_rows(shapes):
    """(rows float64 [T, TRI_WORDS] in group order, material rows [M, MAT_WORDS], the rows' texture
    coordinates [T, UV_WORDS], zeros for a mesh without any) of the meshes of ``shapes``, validated.
    ValueError as ``mesh_table``."""
    rows, mats, uvs, base = [], [], [], 0
    meshes = [sh for sh in shapes if isinstance(sh, TriangleMesh)]
    if not meshes:
        raise ValueError("no TriangleMesh among the shapes")
    for i, mesh in enumerate(meshes):
        v, f, n = _mesh_arrays(mesh, i)
        F = f.shape[0]
        uv = _mesh_uvs(mesh, i, F)
        mats.append(_mesh_material(mesh, i))
        uvs.append(np.zeros((F, UV_WORDS)) if uv is None else uv.reshape(F, UV_WORDS))
        if base + F > MAX_TRIANGLES:
            raise ValueError(f"at most {MAX_TRIANGLES} triangles per scene (RTX_MAX_TRIANGLES), got more")
        v0 = v[f[:, 0]]
        e1, e2 = v[f[:, 1]] - v0, v[f[:, 2]] - v0
        ng = np.cross(e1, e2)
        with np.errstate(all="ignore"):
            ng = ng / np.sqrt((ng * ng).sum(axis=1, keepdims=True))
        bad = ~np.isfinite(ng).all(axis=1)
        if bad.any():
            raise ValueError(f"mesh {i}: face {int(np.nonzero(bad)[0][0])} is degenerate (its normal cannot be "
                             "normalised)")
        r = np.zeros((F, TRI_WORDS))
        r[:, T_V0:T_V0 + 3], r[:, T_E1:T_E1 + 3], r[:, T_E2:T_E2 + 3], r[:, T_NG:T_NG + 3] = v0, e1, e2, ng
        r[:, T_MESH] = i
        if n is not None:
            r[:, T_SMOOTH] = 1.0
            r[:, T_N0:T_N0 + 3], r[:, T_N1:T_N1 + 3], r[:, T_N2:T_N2 + 3] = n[f[:, 0]], n[f[:, 1]], n[f[:, 2]]
        r[:, T_NUM] = base + np.arange(F)
        rows.append(r)
        base += F
    return np.concatenate(rows), np.asarray(mats, dtype=np.float64).reshape(len(mats), -1), np.concatenate(uvs)


def build_tree(lo, hi, max_leaf):
    """A bounding-volume tree over boxes (``lo``, ``hi`` float64 [T, 3]), built level by level: every
    segment of more than ``max_leaf`` boxes (None: one leaf holds them all) is sorted by its boxes'
    centres along the longest axis of the centres' extent and cut at the median. Returns (order [T]:
    the boxes in leaf order, starts, ends [N]: every node's range of ``order`` in depth-first order)."""
    T = lo.shape[0]
    centre = (lo + hi) * 0.5
    order = np.arange(T)
    starts, ends = [np.array([0])], [np.array([T])]
    s, e = starts[0], ends[0]
    leaf = T if max_leaf is None else int(max_leaf)
    while True:
        big = (e - s) > leaf
        s, e = s[big], e[big]
        if s.size == 0:
            break
        # the triangles of the segments to cut, with their segment's number
        length = e - s
        seg = np.repeat(np.arange(s.size), length)
        pos = np.arange(length.sum()) - np.repeat(np.cumsum(length) - length, length) + np.repeat(s, length)
        c = centre[order[pos]]
        first = np.cumsum(length) - length
        ext = np.maximum.reduceat(c, first, axis=0) - np.minimum.reduceat(c, first, axis=0)
        axis = np.argmax(ext, axis=1)
        key = c[np.arange(c.shape[0]), axis[seg]]
        by = np.lexsort((order[pos], key, seg))  # (the triangle's index last: a total order)
        order[pos] = order[pos][by]
        mid = s + (length + 1) // 2
        s, e = np.concatenate([s, mid]), np.concatenate([mid, e])
        starts.append(s)
        ends.append(e)
    s, e = np.concatenate(starts), np.concatenate(ends)
    dfs = np.lexsort((-(e - s), s))  # depth first: by start, a parent before its first child
    return order, s[dfs], e[dfs]


def _content_digest(shapes) -> str:
    """The digest of everything a table is built from: every mesh's arrays and material row, its texture
    coordinates and its image's digest."""
    h = hashlib.blake2b(digest_size=16)
    k = 0
    for sh in shapes:
        if not isinstance(sh, TriangleMesh):
            continue
        h.update(np.asarray(_mesh_material(sh, k), dtype=np.float64).tobytes())
        tex = sh.shader.diffuse_color
        if _is_image(tex):
            h.update(b"image" + str(getattr(tex, "digest", None) or _texels_digest(tex.texels)).encode())
        for a in (sh.vertices, sh.faces, sh.normals, getattr(sh, "uvs", None)):
            a = np.ascontiguousarray(np.zeros(0) if a is None else a)
            h.update(repr((a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        k += 1
    return h.hexdigest()


def _texels_digest(texels) -> str:
    t = np.ascontiguousarray(texels, dtype=np.float64)
    return hashlib.blake2b(t.tobytes() + repr(t.shape).encode(), digest_size=16).hexdigest()


def mesh_table(shapes, max_leaf=4) -> np.ndarray:
    """The float64 table of ``rtx_trace_mesh`` for the meshes of ``shapes`` (layout in
    include/rtx_hip.h): a header, the triangle rows in the tree's leaf order, one material row per mesh
    and the tree's nodes in depth-first order with skip links, in the culling tree's node shape (box,
    first, count, skip, margin). ``max_leaf``: the most triangles of a leaf (None: one leaf). Cached by
    content. ValueError for vertices that are not finite, face indices out of range, a mesh without
    faces, a degenerate face (one whose normal cannot be normalised; none is dropped), normals of the
    wrong shape, a transmissive shader on a mesh, and more than MAX_TRIANGLES triangles.
    If some mesh's texture is an ``ImageTexture`` (``has_image``), the table is rtx_trace_mesh_uv's: after
    the nodes come a UV part, UV_WORDS words per triangle row in the rows' leaf order (zeros for a mesh
    without ``uvs``), and one texel block per distinct image (float64 RGB, row-major, row 0 the top), the
    two offsets in the header words MH_UVS and MH_TEXELS, and such a mesh's material row holds its block's
    word offset, width and height. Then also ValueError for an ImageTexture on a mesh without ``uvs``, for
    ``uvs`` of the wrong shape, not finite or beyond UV_MAX, for an image of more than MAX_TEXELS texels
    and for a table of 2^31 words or more. Otherwise the table is the one of a scene without ``uvs``."""
    return mesh_table_entry(shapes, max_leaf)[0]


def mesh_table_entry(shapes, max_leaf=4) -> tuple:
    """(``mesh_table``, its content key): the key names the meshes' content and ``max_leaf``."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    if max_leaf is not None and (isinstance(max_leaf, bool) or int(max_leaf) != max_leaf or max_leaf < 1):
        raise ValueError(f"max_leaf must be None or an int >= 1, got {max_leaf!r}")
    shapes = list(shapes)
    key = (_content_digest(shapes), max_leaf)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit, key
    image = has_image(shapes)
    rows, mats, uvs = triangle_rows(shapes)
    v0, e1, e2 = rows[:, T_V0:T_V0 + 3], rows[:, T_E1:T_E1 + 3], rows[:, T_E2:T_E2 + 3]
    corners = np.stack([v0, v0 + e1, v0 + e2])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    order, s, e = build_tree(lo, hi, max_leaf)
    lo, hi = lo[order], hi[order]
    T, N = rows.shape[0], s.shape[0]
    # every node's box: reduceat over (start, end) pairs, a sentinel row for end == T
    pairs = np.stack([s, e], axis=1).ravel()
    nlo = np.minimum.reduceat(np.concatenate([lo, lo[-1:]]), pairs, axis=0)[::2]
    nhi = np.maximum.reduceat(np.concatenate([hi, hi[-1:]]), pairs, axis=0)[::2]
    nodes = np.zeros((N, L.NODE_WORDS))
    nodes[:, L.N_LOX:L.N_LOX + 3], nodes[:, L.N_HIX:L.N_HIX + 3] = nlo, nhi
    inner = np.zeros(N, dtype=bool)
    inner[:-1] = s[1:] == s[:-1]  # a node followed by one of the same start has children
    nodes[:, L.N_FIRST] = s
    nodes[:, L.N_COUNT] = np.where(inner, 0, e - s)
    nodes[:, L.N_SKIP] = np.searchsorted(s, e, side="left")  # the first node at or after the range's end
    far = (np.maximum(np.abs(nlo), np.abs(nhi)) ** 2).sum(axis=1)  # the largest |corner|^2
    nodes[:, L.N_MARGIN] = MARGIN * (1.0 + far)
    head = np.zeros(HDR_WORDS)
    tris_at = HDR_WORDS
    mats_at = tris_at + T * TRI_WORDS
    nodes_at = mats_at + mats.size
    words = nodes_at + nodes.size
    head[[MH_MAGIC, MH_NTRI, MH_NMESH, MH_NNODES, MH_TRIS, MH_MATS, MH_NODES, MH_WORDS]] = (
        MAGIC, T, mats.shape[0], N, tris_at, mats_at, nodes_at, words)
    parts = [head, rows[order].ravel(), mats, nodes.ravel()]
    if image:  # the UV part in the rows' leaf order, then one texel block per distinct image
        head[MH_UVS] = words
        parts.append(uvs[order].ravel())
        words += uvs.size
        head[MH_TEXELS] = words
        head[MH_WORDS] = _texel_blocks(shapes, mats, words, parts)
    parts[2] = mats.ravel()
    table = np.concatenate(parts)
    table.setflags(write=False)
    if len(_TABLES) >= 8:
        _TABLES.pop(next(iter(_TABLES)))
    _TABLES[key] = table
    return table, key


_TABLES: dict = {}  # (content digest, max_leaf) -> table


def _texel_blocks(shapes, mats, words: int, parts: list) -> int:
    """One texel block per distinct image of ``shapes``' meshes appended to ``parts`` from word ``words`` on, each
    image mesh's material row (``mats``) given its block's offset: the table's length with them. ValueError for
    a table of 2^31 words or more."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    blocks = {}
    for i, mesh in enumerate(sh for sh in shapes if isinstance(sh, TriangleMesh)):
        tex = mesh.shader.diffuse_color
        if not _is_image(tex):
            continue
        t = _mesh_image(mesh, i)
        digest = getattr(tex, "digest", None) or _texels_digest(t)
        if digest not in blocks:
            blocks[digest] = words
            parts.append(t.ravel())
            words += t.size
        mats[i, L.M_TR] = blocks[digest]
    if words >= 1 << 31:
        raise ValueError(f"the mesh table would have {words} words; rtx_trace_mesh_uv takes fewer than 2^31")
    return words


# ---------------------------------------------------------------------------------------------
# the device build (rtx_mesh_build)
# ---------------------------------------------------------------------------------------------
class DeviceInputs(NamedTuple):
    """What rtx_mesh_build makes a scene's table from: the meshes' arrays one after the other and the
    skeleton, the table with everything that does not depend on a vertex."""

    vertices: np.ndarray  # float64 [V, 3]
    faces: np.ndarray  # int32 [T, 3], into ``vertices``
    tri_mesh: np.ndarray  # int32 [T]: each triangle's mesh
    normals: np.ndarray | None  # float64 [V, 3] (zeros for a flat mesh), None if no mesh is smooth
    smooth: np.ndarray | None  # int32 [M]: 1 for a mesh with vertex normals; None with ``normals``
    uvs: np.ndarray | None  # float64 [T, UV_WORDS] (zeros for a mesh without), None for a table without a UV part
    skeleton: np.ndarray  # float64 [words]
    first_triangle: np.ndarray  # int64 [M]: each mesh's first triangle number
    max_leaf: int  # rtx_mesh_build's: 0 for one leaf


def tree_ranges(T: int, max_leaf):
    """(starts, ends [N]) of the nodes of ``build_tree`` over ``T`` boxes in depth-first order: they depend on
    ``T`` and ``max_leaf`` alone. Cached."""
    hit = _RANGES.get((T, max_leaf))
    if hit is not None:
        return hit
    leaf = T if max_leaf is None else int(max_leaf)
    starts, ends = [np.array([0])], [np.array([T])]
    s, e = starts[0], ends[0]
    while True:
        big = (e - s) > leaf
        s, e = s[big], e[big]
        if s.size == 0:
            break
        mid = s + (e - s + 1) // 2
        s, e = np.concatenate([s, mid]), np.concatenate([mid, e])
        starts.append(s)
        ends.append(e)
    s, e = np.concatenate(starts), np.concatenate(ends)
    dfs = np.lexsort((-(e - s), s))
    if len(_RANGES) >= 8:
        _RANGES.pop(next(iter(_RANGES)))
    _RANGES[(T, max_leaf)] = s[dfs], e[dfs]
    return _RANGES[(T, max_leaf)]


def device_inputs(shapes, max_leaf=4) -> DeviceInputs:
    """The inputs of rtx_mesh_build for the meshes of ``shapes``, validated; cached by content like
    ``mesh_table``. The skeleton is ``mesh_table``'s header, material rows, every node's first, count and skip
    and the texel blocks, with zeros where the build writes (the rows, the nodes' boxes and margins, the UV
    part). ValueError as ``mesh_table``, but for a degenerate face: the device finds those."""
    return device_inputs_entry(shapes, max_leaf)[0]


def device_inputs_entry(shapes, max_leaf=4) -> tuple:
    """(``device_inputs``, its content key): the key is ``mesh_table_entry``'s."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    if max_leaf is not None and (isinstance(max_leaf, bool) or int(max_leaf) != max_leaf or max_leaf < 1):
        raise ValueError(f"max_leaf must be None or an int >= 1, got {max_leaf!r}")
    shapes = list(shapes)
    key = (_content_digest(shapes), max_leaf)
    hit = _INPUTS.get(key)
    if hit is not None:
        return hit, key
    meshes = [sh for sh in shapes if isinstance(sh, TriangleMesh)]
    if not meshes:
        raise ValueError("no TriangleMesh among the shapes")
    verts, faces, tri_mesh, normals, smooth, uvs, mats, first, base, vbase = [], [], [], [], [], [], [], [], 0, 0
    for i, mesh in enumerate(meshes):
        v, f, n = _mesh_arrays(mesh, i)
        F = f.shape[0]
        uv = _mesh_uvs(mesh, i, F)
        mats.append(_mesh_material(mesh, i))
        if base + F > MAX_TRIANGLES:
            raise ValueError(f"at most {MAX_TRIANGLES} triangles per scene (RTX_MAX_TRIANGLES), got more")
        verts.append(v)
        faces.append(f + vbase)
        tri_mesh.append(np.full(F, i, dtype=np.int32))
        normals.append(np.zeros_like(v) if n is None else n)
        smooth.append(0 if n is None else 1)
        uvs.append(np.zeros((F, UV_WORDS)) if uv is None else uv.reshape(F, UV_WORDS))
        first.append(base)
        base += F
        vbase += v.shape[0]
    if vbase >= 1 << 31:
        raise ValueError(f"the meshes have {vbase} vertices; rtx_mesh_build takes fewer than 2^31")
    mats = np.asarray(mats, dtype=np.float64).reshape(len(mats), -1)
    T = base
    s, e = tree_ranges(T, max_leaf)
    N = s.shape[0]
    nodes = np.zeros((N, L.NODE_WORDS))
    inner = np.zeros(N, dtype=bool)
    inner[:-1] = s[1:] == s[:-1]
    nodes[:, L.N_FIRST] = s
    nodes[:, L.N_COUNT] = np.where(inner, 0, e - s)
    nodes[:, L.N_SKIP] = np.searchsorted(s, e, side="left")
    head = np.zeros(HDR_WORDS)
    tris_at = HDR_WORDS
    mats_at = tris_at + T * TRI_WORDS
    nodes_at = mats_at + mats.size
    words = nodes_at + nodes.size
    head[[MH_MAGIC, MH_NTRI, MH_NMESH, MH_NNODES, MH_TRIS, MH_MATS, MH_NODES, MH_WORDS]] = (
        MAGIC, T, mats.shape[0], N, tris_at, mats_at, nodes_at, words)
    parts = [head, np.zeros(T * TRI_WORDS), mats, nodes.ravel()]
    image = has_image(shapes)
    if image:
        head[MH_UVS] = words
        parts.append(np.zeros(T * UV_WORDS))
        words += T * UV_WORDS
        head[MH_TEXELS] = words
        head[MH_WORDS] = _texel_blocks(shapes, mats, words, parts)
    parts[2] = mats.ravel()
    skeleton = np.concatenate(parts)
    any_smooth = any(smooth)
    out = DeviceInputs(np.ascontiguousarray(np.concatenate(verts)),
                       np.ascontiguousarray(np.concatenate(faces), dtype=np.int32), np.concatenate(tri_mesh),
                       np.ascontiguousarray(np.concatenate(normals)) if any_smooth else None,
                       np.asarray(smooth, dtype=np.int32) if any_smooth else None,
                       np.ascontiguousarray(np.concatenate(uvs)) if image else None, skeleton,
                       np.asarray(first, dtype=np.int64), 0 if max_leaf is None else int(max_leaf))
    for a in out[:7]:
        if a is not None:
            a.setflags(write=False)
    if len(_INPUTS) >= 8:
        _INPUTS.pop(next(iter(_INPUTS)))
    _INPUTS[key] = out
    return out, key


_INPUTS: dict = {}  # (content digest, max_leaf) -> DeviceInputs
_RANGES: dict = {}  # (T, max_leaf) -> (starts, ends) of the tree's nodes


def degenerate_face_error(inputs: DeviceInputs, triangle: int) -> ValueError:
    """``triangle_rows``' error for the group's triangle ``triangle`` (rtx_mesh_build's status word)."""
    i = int(np.searchsorted(inputs.first_triangle, triangle, side="right")) - 1
    return ValueError(f"mesh {i}: face {int(triangle - inputs.first_triangle[i])} is degenerate (its normal cannot be "
                      "normalised)")


def check_table(table) -> None:
    """ValueError unless ``table``'s header is that of a mesh table of its own length: the magic, the
    counts and the three parts within it (what rtx_trace_mesh's kernel checks before it reads them), and,
    where the header names a UV part or texel blocks (rtx_trace_mesh_uv), both of them and the block of
    every image material within it."""
    from python_ray_tracer_amd.infrastructure.hip import _lib as L

    t = np.asarray(table)
    if t.dtype != np.float64 or t.ndim != 1 or t.size < HDR_WORDS or t[MH_MAGIC] != MAGIC:
        raise ValueError("not a mesh table (meshes.mesh_table): float64 [words] with the mesh magic")
    T, M, N, a, b, c, w = (int(x) for x in t[[MH_NTRI, MH_NMESH, MH_NNODES, MH_TRIS, MH_MATS, MH_NODES, MH_WORDS]])
    ok = (1 <= T <= MAX_TRIANGLES and 1 <= M <= T and 1 <= N <= 2 * T and w == t.size and a >= HDR_WORDS
          and a + T * TRI_WORDS <= w and b >= HDR_WORDS and b + M * L.MAT_WORDS <= w and c >= HDR_WORDS
          and c + N * L.NODE_WORDS <= w)
    if not ok:
        raise ValueError("mesh table: the header's counts and offsets do not fit the table")
    u, x = t[MH_UVS], t[MH_TEXELS]
    if u == 0 and x == 0:
        return
    ok = (u >= HDR_WORDS and u == np.floor(u) and u + T * UV_WORDS <= w and x >= HDR_WORDS and x == np.floor(x)
          and x <= w)
    if ok:
        for m in t[b:b + M * L.MAT_WORDS].reshape(M, L.MAT_WORDS):
            if m[L.M_TEX] == L.TEX_IMAGE:
                off, W, H = m[L.M_TR], m[L.M_TG], m[L.M_TB]
                ok = ok and (off >= x and off == np.floor(off) and W >= 1 and H >= 1 and W == np.floor(W)
                             and H == np.floor(H) and W * H <= MAX_TEXELS and off + 3 * W * H <= w)
    if not ok:
        raise ValueError("mesh table: the offsets of the UV part, the texel blocks or an image material do not fit "
                         "the table")
