"""Host maths of several point lights (``rtx_trace_lights``): the routing rule, the
table of the lights and the validation of what a multi-light render needs.

A scene is a multi-light scene if and only if ``scene.lights`` holds at least one
``domain.ColoredPointLight``. Then every point light of the list contributes, in list order; a point
light is an object with a ``position`` that is not a ``DomeLight``, and a plain ``PointLight`` counts
as intensity 1 and white. A scene without a ``ColoredPointLight`` renders as before, lit by
``lights[0]`` alone (shader.py:75). The lights other than ``lights[0]`` do not travel in the scene
blob: the kernel reads them all from ``lights_table``'s float64 [L, 6]. Nothing here touches the GPU:
a bad value raises ValueError before any device call.
"""

from __future__ import annotations

import math

import numpy as np

from python_ray_tracer_amd.domain import ColoredPointLight

MAX_LIGHTS = 8  # RTX_MAX_POINT_LIGHTS
MAX_BOUNCES = 16  # RTX_LIGHTS_MAX_BOUNCES


def _number(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a number, got {x!r}")
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"{what} must be finite, got {x!r}")
    return x


def _triple(v, what: str) -> tuple:
    c = v.components() if hasattr(v, "components") else tuple(v)
    if len(c) != 3:
        raise ValueError(f"{what} must have three components, got {v!r}")
    return tuple(_number(x, f"{what}[{i}]") for i, x in enumerate(c))


def _is_point(light) -> bool:
    return hasattr(light, "position") and type(light).__name__ != "DomeLight"


def is_multi_light(lights) -> bool:
    """Whether ``lights`` holds a ``ColoredPointLight`` (nothing is validated)."""
    return any(isinstance(li, ColoredPointLight) for li in lights)


def lights_table(lights):
    """float64 [L, 6] for ``rtx_trace_lights``: row i is (px, py, pz, e_r, e_g, e_b) of the i-th point
    light of ``lights`` in list order, e = intensity * colour in float64 (a plain ``PointLight``: 1, 1,
    1; dome lights are skipped). None for a list without a ``ColoredPointLight``: such a scene renders
    through the one-light path, bit for bit as before. ValueError for a position, intensity or colour
    component that is not a finite number, for a negative intensity or colour component, and for more
    than ``MAX_LIGHTS`` point lights."""
    lights = list(lights)
    if not is_multi_light(lights):
        return None
    rows = []
    for i, li in enumerate(lights):
        if not _is_point(li):
            continue
        pos = _triple(li.position, f"light {i}: position")
        if isinstance(li, ColoredPointLight):
            inten = _number(li.intensity, f"light {i}: intensity")
            col = _triple(li.color, f"light {i}: color")
        else:
            inten, col = 1.0, (1.0, 1.0, 1.0)
        if inten < 0.0 or min(col) < 0.0:
            raise ValueError(f"light {i}: intensity and colour must be >= 0, got {inten!r} and {col!r}")
        rows.append(pos + tuple(inten * c for c in col))
    if len(rows) > MAX_LIGHTS:
        raise ValueError(f"at most {MAX_LIGHTS} point lights in a multi-light scene, got {len(rows)}")
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), 6)


def check_bounces(max_bounces) -> int:
    """The bounce cap of a multi-light render: an int in 0..MAX_BOUNCES. ValueError for None (the kernel
    keeps a lane's pending rays in a stack sized by the cap: there is no unbounded form) and for a
    larger cap."""
    if max_bounces is None:
        raise ValueError("a scene with a ColoredPointLight needs a finite bounce cap: "
                         f"HipRenderer(max_bounces=B) with B in 0..{MAX_BOUNCES}")
    if isinstance(max_bounces, bool) or int(max_bounces) != max_bounces or not 0 <= max_bounces <= MAX_BOUNCES:
        raise ValueError(f"a scene with a ColoredPointLight renders with HipRenderer(max_bounces=B), B in "
                         f"0..{MAX_BOUNCES}, got {max_bounces!r}")
    return int(max_bounces)
