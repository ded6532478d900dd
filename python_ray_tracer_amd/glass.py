"""Host maths of transmission (glass spheres; ``rtx_trace_glass``): the side table of
the transmissive spheres and the validation of what a transmissive render needs.

A shader is transmissive when its ``transmission_gain`` is not 0. The attribute is optional: it is
read with ``getattr(shader, "transmission_gain", 0.0)``, so the reference's own ``NumpyShader``
objects work with or without it. The index of refraction is the shader's ``specular_ior``
(shader.py:51: "default value for glass"). Neither travels in the scene blob: the kernel reads them
from ``glass_table``'s float64 [2, S] (row 0 the gains, row 1 the indices). Nothing here touches the
GPU: a bad value raises ValueError before any device call.
"""

from __future__ import annotations

import math

import numpy as np

MAX_BOUNCES = 8  # RTX_GLASS_MAX_BOUNCES: the ray tree has up to 2^(B+1) rays per pixel


def _number(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a number, got {x!r}")
    return float(x)


def is_transmissive(shapes) -> bool:
    """Whether some shape's shader has a ``transmission_gain`` other than 0 (nothing is validated)."""
    for s in shapes:
        if getattr(getattr(s, "shader", None), "transmission_gain", 0.0) != 0:  # (None, NaN, a string: glass_table raises)
            return True
    return False


def glass_table(shapes):
    """float64 [2, S] for ``rtx_trace_glass`` (row 0: every shape's transmission_gain, row 1: its
    specular_ior), or None when every gain is 0: such a scene renders through the opaque path, bit
    for bit as before. ValueError for a gain that is not finite and >= 0, and for a transmissive
    sphere whose specular_ior is not finite and >= 1 or whose radius is not > 0."""
    shapes = list(shapes)
    table = np.zeros((2, len(shapes)), dtype=np.float64)
    table[1] = 1.0
    glass = False
    for i, s in enumerate(shapes):
        sh = getattr(s, "shader", None)
        gain = _number(getattr(sh, "transmission_gain", 0.0), f"shape {i}: transmission_gain")
        if not (gain >= 0.0 and math.isfinite(gain)):
            raise ValueError(f"shape {i}: transmission_gain must be finite and >= 0, got {gain!r}")
        if gain == 0.0:
            continue
        ior = _number(getattr(sh, "specular_ior", None), f"shape {i}: specular_ior")
        if not (ior >= 1.0 and math.isfinite(ior)):
            raise ValueError(f"shape {i}: a transmissive sphere needs a finite specular_ior >= 1 (the ray is refracted "
                             f"into a denser ball: no total internal reflection), got {ior!r}")
        radius = _number(getattr(s, "radius", None), f"shape {i}: radius")
        if not radius > 0.0:
            raise ValueError(f"shape {i}: a transmissive sphere needs a radius > 0, got {radius!r}")
        table[0, i] = gain
        table[1, i] = ior
        glass = True
    return table if glass else None


def check_bounces(max_bounces) -> int:
    """The bounce cap of a transmissive render: an int in 0..MAX_BOUNCES. ValueError for None (every
    glass hit adds a ray, so the tree has up to 2^(B+1) rays per pixel: there is no unbounded form)
    and for a larger cap."""
    if max_bounces is None:
        raise ValueError("a scene with a transmissive sphere (transmission_gain != 0) needs a finite bounce cap: "
                         f"HipRenderer(max_bounces=B) with B in 0..{MAX_BOUNCES} (every glass hit adds a ray)")
    if isinstance(max_bounces, bool) or int(max_bounces) != max_bounces or not 0 <= max_bounces <= MAX_BOUNCES:
        raise ValueError(f"a scene with a transmissive sphere renders with max_bounces in 0..{MAX_BOUNCES} (up to "
                         f"2^(B+1) rays per pixel), got {max_bounces!r}")
    return int(max_bounces)
