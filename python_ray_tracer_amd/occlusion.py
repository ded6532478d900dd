"""Host maths of the occlusion passes (``HipRenderer.render_occlusion``, ``rtx_occlusion``): the two
sample tables and the validation of the passes' parameters.

The kernel needs no sine, cosine or random number: the directions of a bundle come from
``hemisphere_table(side)`` (the concentric image of the side x side stratum centres, lifted onto the
unit hemisphere, so that the directions are cosine-distributed) turned about the surface normal by one
of the 64 rotations of ``rotation_table()``, which a hash of the hit point picks (include/rtx_hip.h).
Everything here is host float64 arithmetic in a fixed order (tests/occlusion_ref.py restates it), and
nothing touches the GPU: a bad argument raises ValueError before any device call.
"""

from __future__ import annotations

import math

import numpy as np

from python_ray_tracer_amd.camera import lens_table

MAX_SIDE = 8  # samples per bundle side (mirrors rtx_occlusion's bound)
ROTATIONS = 64  # entries of the rotation table
PASSES = ("ao", "soft_lit")  # in result order (the RTX_OCC_* bits 1, 2)
FARAWAY = 1.0e39  # base.py:12; the default (and largest) max_distance: nothing is too far to occlude


def check_side(side) -> int:
    if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or not 1 <= side <= MAX_SIDE:
        raise ValueError(f"side must be an int in 1..{MAX_SIDE} (side x side rays per hit), got {side!r}")
    return int(side)


def _number(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a number, got {x!r}")
    return float(x)


def check_max_distance(max_distance) -> float:
    """``max_distance`` as the kernel takes it: None is FARAWAY; a number in (0, 1e39]."""
    if max_distance is None:
        return FARAWAY
    d = _number(max_distance, "max_distance")
    if not 0.0 < d <= FARAWAY:
        raise ValueError(f"max_distance must lie in (0, {FARAWAY:g}] (None: no limit), got {max_distance!r}")
    return d


def check_light_radius(light_radius) -> float:
    r = _number(light_radius, "light_radius")
    if not (r >= 0.0 and math.isfinite(r)):
        raise ValueError(f"light_radius must be finite and >= 0 (0: the reference's point light), got {light_radius!r}")
    return r


def pass_names(passes) -> tuple:
    """The requested passes in the fixed order of PASSES; ValueError for an unknown or missing name."""
    if isinstance(passes, str):
        passes = (passes,)
    passes = tuple(passes)
    bad = [p for p in passes if p not in PASSES]
    if bad or not passes:
        raise ValueError(f"passes: need one or more of {PASSES}, got {passes!r}")
    return tuple(k for k in PASSES if k in passes)


def hemisphere_table(side: int) -> np.ndarray:
    """float64 [3, side*side]: rows 0 and 1 are ``camera.lens_table(side)``, the concentric image
    (a, b) of the stratum centres in the unit disk; row 2 is sqrt(max(0, 1 - (a*a + b*b))), the height
    of the unit hemisphere over that point (Malley's method: a uniform disk lifted onto the hemisphere
    is cosine-distributed)."""
    side = check_side(side)
    disk = lens_table(side)
    a, b = disk[0], disk[1]
    return np.stack([a, b, np.sqrt(np.maximum(0.0, 1.0 - (a * a + b * b)))])


def rotation_table() -> np.ndarray:
    """float64 [2, 64]: entry r is (cos phi, sin phi) with phi = 2 pi (r + 0.5) / 64, in Python floats."""
    out = np.empty((2, ROTATIONS), dtype=np.float64)
    for r in range(ROTATIONS):
        phi = 2.0 * math.pi * (r + 0.5) / ROTATIONS
        out[0, r] = math.cos(phi)
        out[1, r] = math.sin(phi)
    return out
