"""Host maths of the environment map (``rtx_trace_lights_env`` / ``rtx_trace_glass_env``):
the routing rule, the image as the device reads it, the validation of what such a render needs, and
the two values the host computes for the kernel.

A scene is an environment scene if and only if ``scene.lights`` holds a ``domain.EnvironmentLight``
(exactly one: two raise ValueError). Then a ray that meets no shape returns the image's colour in its
direction instead of black, at every level of the recursion; nothing else changes. The image does not
travel in the scene blob and is not part of the scene key: the renderer uploads it once per content
(``digest``) and device. ``lights[0]`` must still be a point light; the packer's IndexError and
AttributeError stay as they are. Nothing here touches the GPU: a bad value raises ValueError before any
device call.

    gain[c] = intensity * color[c]          float64
    turn    = rotation / 360.0              rotation in degrees about +y
"""

from __future__ import annotations

import hashlib
import math

import numpy as np

from python_ray_tracer_amd.domain import EnvironmentLight
from python_ray_tracer_amd.lights import _number, _triple

MAX_TEXELS = 1 << 23  # RTX_ENV_MAX_TEXELS
MAX_BOUNCES = 16  # RTX_LIGHTS_MAX_BOUNCES: an environment scene without glass
GLASS_MAX_BOUNCES = 8  # RTX_GLASS_MAX_BOUNCES: with glass


def image_texels(image):
    """(texels, digest) of an environment image: a read-only float32 [H, W, 4] array (RGB and a zero
    word) and the blake2b hash of its content and shape. ``image``: a path (PIL, ``convert("RGB")``,
    ``/ 255.0``), an (H, W, 3) uint8 array (``/ 255.0``) or an (H, W, 3) float array. ValueError for
    another shape, more than ``MAX_TEXELS`` texels, or a texel that is negative or not finite (in
    float32: a value beyond its range counts as infinite)."""
    if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
        from PIL import Image

        arr = np.asarray(Image.open(image).convert("RGB")) / 255.0
    else:
        arr = np.asarray(image)
        if arr.dtype == np.uint8:
            arr = arr / 255.0
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] < 1 or arr.shape[1] < 1 or arr.dtype.kind not in "fiu":
        raise ValueError(f"environment image: need an (H, W, 3) array of numbers, got shape {arr.shape} of "
                         f"{arr.dtype}")
    h, w = int(arr.shape[0]), int(arr.shape[1])
    if h * w > MAX_TEXELS:
        raise ValueError(f"environment image: at most {MAX_TEXELS} texels, got {w} x {h}")
    texels = np.zeros((h, w, 4), dtype=np.float32)
    with np.errstate(over="ignore"):
        texels[:, :, :3] = arr
    if not np.isfinite(texels).all():
        raise ValueError("environment image: every texel must be finite")
    if (texels < 0).any():
        raise ValueError("environment image: every texel must be >= 0")
    texels.setflags(write=False)
    digest = hashlib.blake2b(texels.tobytes() + repr(texels.shape).encode(), digest_size=16).hexdigest()
    return texels, digest


def environment_of(lights):
    """The ``EnvironmentLight`` of ``lights``, or None for a list without one (nothing else is
    validated). ValueError for two of them."""
    found = None
    for li in lights:
        if isinstance(li, EnvironmentLight):
            if found is not None:
                raise ValueError("at most one EnvironmentLight in scene.lights: a ray that meets nothing sees one "
                                 "environment; combine the images into one")
            found = li
    return found


def env_params(light) -> tuple:
    """(gain, turn) of an ``EnvironmentLight`` as the kernel takes them: gain = intensity * colour per
    channel in float64, turn = rotation / 360.0. ValueError for an intensity, colour component or
    rotation that is not a finite number, and for a negative intensity or colour component."""
    inten = _number(light.intensity, "EnvironmentLight: intensity")
    col = _triple(light.color, "EnvironmentLight: color")
    rot = _number(light.rotation, "EnvironmentLight: rotation")
    if inten < 0.0 or min(col) < 0.0:
        raise ValueError(f"EnvironmentLight: intensity and colour must be >= 0, got {inten!r} and {col!r}")
    gain = tuple(inten * c for c in col)
    if not all(math.isfinite(g) for g in gain):
        raise ValueError(f"EnvironmentLight: intensity * colour must be finite, got {gain!r}")
    return gain, rot / 360.0


def check_bounces(max_bounces, with_glass: bool) -> int:
    """The bounce cap of an environment render: an int in 0..16, or 0..8 with glass in the scene.
    ValueError for None (both kernels keep a lane's pending rays in a stack sized by the cap: there is
    no unbounded form) and for a larger cap."""
    top = GLASS_MAX_BOUNCES if with_glass else MAX_BOUNCES
    what = "a scene with an EnvironmentLight" + (" and a transmissive sphere" if with_glass else "")
    if max_bounces is None:
        raise ValueError(f"{what} needs a finite bounce cap: HipRenderer(max_bounces=B) with B in 0..{top}")
    if isinstance(max_bounces, bool) or int(max_bounces) != max_bounces or not 0 <= max_bounces <= top:
        raise ValueError(f"{what} renders with HipRenderer(max_bounces=B), B in 0..{top}, got {max_bounces!r}")
    return int(max_bounces)


def unit_light_table(light0):
    """float64 [1, 6]: the one row (lights[0], 1, 1, 1) an environment scene without a
    ``ColoredPointLight`` is lit by, as the scene without the environment is (a second plain
    ``PointLight`` stays ignored)."""
    pos = _triple(light0.position, "light 0: position")
    return np.asarray([pos + (1.0, 1.0, 1.0)], dtype=np.float64)
