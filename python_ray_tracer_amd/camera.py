"""Host maths of ``domain.PerspectiveCamera``: validation, the camera record and the lens table.

The reference's camera is a position in front of a screen fixed at z = 0 (base.py:123-141). A
``PerspectiveCamera`` adds a target, an up vector, a vertical field of view and a thin lens; this
module reduces one to the six vectors ``rtx_camera_rays`` (include/rtx_hip.h) generates rays from.
Everything here is Python float64 scalar arithmetic in a fixed order (tests/camera_ref.py restates
it), and nothing touches the GPU: a bad camera raises ValueError before any device call.

The basis is left-handed like the reference's screen: fwd = +z and up = +y give right = +x.
"""

from __future__ import annotations

import math

import numpy as np

from python_ray_tracer_amd.domain import PerspectiveCamera
from python_ray_tracer_amd.tiling import MAX_SAMPLES

# the camera record's layout: mirrors of include/rtx_hip.h (RTX_CAM_WORDS, RTX_C_*)
CAM_WORDS = 24
C_EYE, C_FWD, C_U, C_V, C_LU, C_LV = 0, 3, 6, 9, 12, 15


def is_perspective(camera) -> bool:
    return isinstance(camera, PerspectiveCamera)


def _xyz(v, what: str) -> tuple:
    try:
        c = (v.x, v.y, v.z) if hasattr(v, "x") else tuple(v)
        c = tuple(float(t) for t in c)
    except (TypeError, ValueError):
        raise ValueError(f"PerspectiveCamera.{what} must be a 3-vector of numbers, got {v!r}") from None
    if len(c) != 3:
        raise ValueError(f"PerspectiveCamera.{what} must have three components, got {v!r}")
    if not all(math.isfinite(t) for t in c):
        raise ValueError(f"PerspectiveCamera.{what} must be finite, got {c}")
    return c


def _number(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x):
        raise ValueError(f"PerspectiveCamera.{what} must be a finite number, got {x!r}")
    return float(x)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def camera_basis(camera) -> dict:
    """The validated camera as Python floats: ``eye``, the orthonormal ``fwd`` / ``right`` / ``tup``
    (the true up: ``up`` made perpendicular to the view), the focus distance ``F``, the half extents
    ``hw`` / ``hh`` of the view at distance 1 and ``lens_radius``. ValueError for a non-finite value,
    a target at the position, an up vector parallel to the view, or a field of view, lens radius or
    focus distance out of range."""
    if not is_perspective(camera):
        raise ValueError(f"expected a PerspectiveCamera, got {type(camera).__name__}")
    W, H = int(camera.width), int(camera.height)
    if W <= 0 or H <= 0:
        raise ValueError(f"camera size must be positive, got {W}x{H}")
    position = _xyz(camera.position, "position")
    target = _xyz(camera.target, "target")
    up = _xyz(camera.up, "up")
    fov = _number(camera.fov, "fov")
    lens_radius = _number(camera.lens_radius, "lens_radius")
    if not 0.0 < fov < 180.0:
        raise ValueError(f"PerspectiveCamera.fov is the vertical field of view in degrees, 0 < fov < 180, got {fov}")
    if lens_radius < 0.0:
        raise ValueError(f"PerspectiveCamera.lens_radius must be >= 0 (0: a pinhole), got {lens_radius}")
    f = (target[0] - position[0], target[1] - position[1], target[2] - position[2])
    dist = math.sqrt(_dot(f, f))
    if dist == 0 or not math.isfinite(dist):
        raise ValueError("PerspectiveCamera.target must differ from position (and lie at a finite distance): the "
                         "view has no direction")
    fwd = _scale(f, 1.0 / dist)
    r = _cross(up, fwd)
    rr = _dot(r, r)
    if not rr > 1e-24 * _dot(up, up):
        raise ValueError(f"PerspectiveCamera.up {up} is parallel to the view direction {fwd} (or zero): the frame "
                         "has no upward direction")
    right = _scale(r, 1.0 / math.sqrt(rr))
    tup = _cross(fwd, right)
    if camera.focus_distance is None:
        F = dist
    else:
        F = _number(camera.focus_distance, "focus_distance")
        if not F > 0.0:
            raise ValueError(f"PerspectiveCamera.focus_distance must be > 0 (None: the target's distance), got {F}")
    hh = math.tan(math.radians(fov) / 2.0)
    hw = hh * (float(W) / H)
    return {"eye": position, "fwd": fwd, "right": right, "tup": tup, "F": F, "hw": hw, "hh": hh,
            "lens_radius": lens_radius}


def camera_record(camera) -> np.ndarray:
    """The camera record of rtx_camera_rays: CAM_WORDS float64 words, E at C_EYE, C = fwd F at C_FWD,
    U = right (hw F) at C_U, V = tup (hh F) at C_V, LU = right lens_radius at C_LU, LV = tup
    lens_radius at C_LV, the rest zero. Raises ValueError like ``camera_basis``, and when the record
    overflows (a focus distance or field of view too large for float64)."""
    b = camera_basis(camera)
    F, lens_radius = b["F"], b["lens_radius"]
    rec = np.zeros(CAM_WORDS, dtype=np.float64)
    rec[C_EYE:C_EYE + 3] = b["eye"]
    rec[C_FWD:C_FWD + 3] = _scale(b["fwd"], F)
    rec[C_U:C_U + 3] = _scale(b["right"], b["hw"] * F)
    rec[C_V:C_V + 3] = _scale(b["tup"], b["hh"] * F)
    rec[C_LU:C_LU + 3] = _scale(b["right"], lens_radius)
    rec[C_LV:C_LV + 3] = _scale(b["tup"], lens_radius)
    if not np.all(np.isfinite(rec)):
        raise ValueError("PerspectiveCamera: the camera record is not finite (focus distance or field of view too "
                         "large)")
    return rec


def has_lens(camera) -> bool:
    return float(camera.lens_radius) > 0.0


def check_camera(camera, samples: int = 1) -> np.ndarray:
    """``camera_record`` for a render with ``samples`` samples per pixel side: also refuses a lens
    with ``samples == 1`` (depth of field comes from the samples of a pixel leaving through different
    points of the lens)."""
    rec = camera_record(camera)
    if has_lens(camera) and int(samples) < 2:
        raise ValueError(f"PerspectiveCamera.lens_radius={camera.lens_radius} needs samples >= 2: depth of field "
                         "averages the samples of a pixel, each through another point of the lens; construct "
                         "HipRenderer(samples=k) or use lens_radius=0")
    return rec


def lens_table(k: int) -> np.ndarray:
    """float64 [2, k*k]: the points of the unit disk the k x k samples of a pixel leave through. Entry
    t = b*k + a is the concentric (Shirley-Chiu) image of the stratum centre sx = 2 (a + 0.5) / k - 1,
    sy = 2 (b + 0.5) / k - 1 of the square [-1, 1]^2: (rad cos th, rad sin th) with rad = sx,
    th = (pi/4) (sy/sx) where |sx| > |sy| and rad = sy, th = pi/2 - (pi/4) (sx/sy) otherwise; (0, 0)
    maps to (0, 0). Row 0 holds the x coordinates, row 1 the y coordinates. Computed on the host, so
    the kernel needs no sine and its rays can be bit-exact."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_SAMPLES:
        raise ValueError(f"lens_table: k must be an int in 1..{MAX_SAMPLES}, got {k!r}")
    k = int(k)
    t = np.arange(k * k)
    sx = 2 * ((t % k) + 0.5) / k - 1
    sy = 2 * ((t // k) + 0.5) / k - 1
    wide = np.abs(sx) > np.abs(sy)
    zero = (sx == 0) & (sy == 0)
    safe_x = np.where(wide, sx, 1.0)
    safe_y = np.where(wide | zero, 1.0, sy)
    rad = np.where(wide, sx, sy)
    th = np.where(wide, (np.pi / 4) * (sy / safe_x), np.pi / 2 - (np.pi / 4) * (sx / safe_y))
    out = np.stack([rad * np.cos(th), rad * np.sin(th)])
    out[:, zero] = 0.0
    return out
