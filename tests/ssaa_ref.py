"""NumPy reference of the supersampling resolve (rtx_resolve_samples, HipRenderer(samples=k)).

Per output pixel (row r, col c) and channel, in float64 and in exactly this order:

    acc = 0.0
    for sy in 0..k-1:          # rows of the sample block, top to bottom
      for sx in 0..k-1:        # left to right
        acc = acc + clip(S[ch][k*r + sy][k*c + sx], 0.0, 1.0)
    out = acc / (double)(k*k)  # one correctly rounded division

vectorised over pixels, channels and frames; the adds stay in that order.
"""

import copy

import numpy as np


def resolve_ref(samples, k: int, width: int, rows: int) -> np.ndarray:
    """``samples``: float64 [..., 3, (k*rows)*(k*width)] (any leading frame axes), each plane a
    row-major (k*rows) x (k*width) sample frame. Returns float64 [..., 3, rows*width]."""
    s = np.asarray(samples, dtype=np.float64)
    lead = s.shape[:-1]
    s = s.reshape(lead + (rows, k, width, k))
    acc = np.zeros(lead + (rows, width), dtype=np.float64)
    for sy in range(k):
        for sx in range(k):
            acc = acc + np.clip(s[..., sy, :, sx], 0.0, 1.0)
    out = acc / np.float64(k * k)
    return out.reshape(lead + (rows * width,))


def to_f32(color: np.ndarray) -> np.ndarray:
    """float32 output: the float64 value rounded once."""
    return color.astype(np.float32)


def to_u8(color: np.ndarray, width: int, rows: int) -> np.ndarray:
    """uint8 output [..., rows, width, 3]: (uint8)(255 * out), truncated (out is in [0, 1])."""
    lead = color.shape[:-2]
    q = (255.0 * color).astype(np.uint8).reshape(lead + (3, rows, width))
    return np.moveaxis(q, -3, -1)


def spec_at(spec: dict, k: int) -> dict:
    """The spec of the sample frame: the same scene and camera position at (k W, k H)."""
    s = copy.deepcopy(spec)
    s["camera"]["width"] = k * spec["camera"]["width"]
    s["camera"]["height"] = k * spec["camera"]["height"]
    return s
