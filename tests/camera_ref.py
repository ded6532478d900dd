"""NumPy restatement of the perspective camera (python_ray_tracer_amd/camera.py, rtx_camera_rays).

``record_ref``: the six vectors of the camera record, in Python float64 scalars:

    f = target - position;  dist = sqrt(f.f);  fwd = f * (1.0/dist)
    r = cross(up, fwd);     right = r * (1.0/sqrt(r.r))     (left-handed: fwd=+z, up=+y -> right=+x)
    tup = cross(fwd, right)
    F = dist if focus_distance is None else focus_distance
    hh = tan(radians(fov)/2.0);  hw = hh * (float(W)/H)
    E = position;  C = fwd*F;  U = right*(hw*F);  V = tup*(hh*F);  LU = right*lens_radius;  LV = tup*lens_radius

``lens_table_ref``: the concentric (Shirley-Chiu) image of the k x k stratum centres, point by point.

``rays_ref``: the rays of the global rows ``rows`` with k x k samples per pixel, in the order of a
sample frame's rows, every operation in float64 in the order of include/rtx_hip.h, the hash in
np.uint32. Nothing here validates: the inputs are the tests' own.
"""

import math

import numpy as np

CAM_WORDS = 24
C_EYE, C_FWD, C_U, C_V, C_LU, C_LV = 0, 3, 6, 9, 12, 15


def _xyz(v):
    return (float(v.x), float(v.y), float(v.z)) if hasattr(v, "x") else tuple(float(t) for t in v)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _mul(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def basis_ref(camera):
    """(fwd, right, tup, dist) as tuples of Python floats."""
    position, target, up = _xyz(camera.position), _xyz(camera.target), _xyz(camera.up)
    f = (target[0] - position[0], target[1] - position[1], target[2] - position[2])
    dist = math.sqrt(_dot(f, f))
    fwd = _mul(f, 1.0 / dist)
    r = _cross(up, fwd)
    right = _mul(r, 1.0 / math.sqrt(_dot(r, r)))
    tup = _cross(fwd, right)
    return fwd, right, tup, dist


def record_ref(camera) -> np.ndarray:
    fwd, right, tup, dist = basis_ref(camera)
    F = dist if camera.focus_distance is None else float(camera.focus_distance)
    hh = math.tan(math.radians(float(camera.fov)) / 2.0)
    hw = hh * (float(int(camera.width)) / int(camera.height))
    lens_radius = float(camera.lens_radius)
    rec = np.zeros(CAM_WORDS, dtype=np.float64)
    rec[C_EYE:C_EYE + 3] = _xyz(camera.position)
    rec[C_FWD:C_FWD + 3] = _mul(fwd, F)
    rec[C_U:C_U + 3] = _mul(right, hw * F)
    rec[C_V:C_V + 3] = _mul(tup, hh * F)
    rec[C_LU:C_LU + 3] = _mul(right, lens_radius)
    rec[C_LV:C_LV + 3] = _mul(tup, lens_radius)
    return rec


def lens_table_ref(k: int) -> np.ndarray:
    out = np.zeros((2, k * k), dtype=np.float64)
    for b in range(k):
        for a in range(k):
            sx = 2 * (a + 0.5) / k - 1
            sy = 2 * (b + 0.5) / k - 1
            if sx == 0 and sy == 0:
                continue
            if abs(sx) > abs(sy):
                rad, th = sx, (np.pi / 4) * (sy / sx)
            else:
                rad, th = sy, np.pi / 2 - (np.pi / 4) * (sx / sy)
            out[0, b * k + a] = rad * np.cos(np.float64(th))
            out[1, b * k + a] = rad * np.sin(np.float64(th))
    return out


def rays_ref(camera, k: int, rows, lens=True):
    """(origins [3, n], dirs [3, n]) of the global rows ``rows`` (in that order: the tile's local
    rows), n = k*k*W*len(rows); ray (k*lr + sy)*(k*W) + k*c + sx is sample (sy, sx) of local row lr,
    column c. ``lens=False`` takes (0, 0) for every sample, as the kernel does without a table."""
    W, H = int(camera.width), int(camera.height)
    rec = record_ref(camera)
    E, C, U, V, LU, LV = (rec[o:o + 3] for o in (C_EYE, C_FWD, C_U, C_V, C_LU, C_LV))
    rows = np.asarray(rows, dtype=np.int64)
    kk = k * k
    # sample-frame coordinates of every ray: local sample row (k*lr + sy), sample column ix
    lr, sy, c, sx = np.meshgrid(np.arange(rows.size), np.arange(k), np.arange(W), np.arange(k), indexing="ij")
    lr, sy, c, sx = (a.reshape(-1) for a in (lr, sy, c, sx))
    gr = rows[lr]
    ix = k * c + sx
    iy = k * gr + sy
    iw = 1.0 / np.float64(k * W)
    ih = 1.0 / np.float64(k * H)
    u = (2 * ix + 1).astype(np.float64) * iw - 1.0
    v = 1.0 - (2 * iy + 1).astype(np.float64) * ih
    with np.errstate(over="ignore"):
        h = c.astype(np.uint32) * np.uint32(0x9E3779B1) ^ gr.astype(np.uint32) * np.uint32(0x85EBCA77)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    j = ((sy * k + sx) + (h % np.uint32(kk)).astype(np.int64)) % kk
    if lens:
        table = lens_table_ref(k)
        a, b = table[0][j], table[1][j]
    else:
        a = b = np.zeros(j.shape, dtype=np.float64)
    off = [LU[i] * a + LV[i] * b for i in range(3)]
    origins = np.stack([E[i] + off[i] for i in range(3)])
    d = [((C[i] + U[i] * u) + V[i] * v) - off[i] for i in range(3)]
    r = 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    dirs = np.stack([d[i] * r for i in range(3)])
    return origins, dirs
