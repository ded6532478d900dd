"""NumPy restatement of adaptive anti-aliasing (HipRenderer(samples=k, adaptive=True); the contract in
include/rtx_hip.h and DESIGN.md §11).

* ``mask_ref``: which pixels are refined. Pixel p = (r, c) is flagged if ``hits[p] > 1`` or some
  neighbour q = (r + dr, c + dc) inside the frame (dr, dc in {-1, 0, 1}, not both 0) has another
  ``id``, another ``lit``, or ``max_ch |cb[ch][q] - cb[ch][p]| > contrast`` with cb = clip01(B), NaN
  sent to 0; strict, in float64.
* ``sample_pixels``: the pixel (row, column) of the (k W, k H) sample frame behind each sample ray
  ``j*k*k + sy*k + sx`` of the listed pixels.
* ``scatter_ref`` / ``adaptive_ref``: a flagged pixel is tests/ssaa_ref.resolve_ref of its samples,
  an unflagged pixel its base sample clipped.
"""

import numpy as np

from tests.ssaa_ref import resolve_ref


def clip01(color) -> np.ndarray:
    """clip(c, 0, 1) with a NaN sent to 0, as the resolve's clip sends it."""
    c = np.asarray(color, dtype=np.float64)
    return np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 1.0))


def mask_ref(color, ident, hits, lit, width: int, height: int, contrast) -> np.ndarray:
    """uint8 [height*width], 1 = flagged. ``color`` float64 [3, n] (unclipped base frame), ``ident`` /
    ``hits`` / ``lit`` [n]; ``contrast`` a float >= 0, or None (= +inf: the geometric test alone)."""
    thr = np.inf if contrast is None else np.float64(contrast)
    n = width * height
    cb = clip01(color).reshape(3, height, width)
    ident = np.asarray(ident).reshape(height, width)
    lit = np.asarray(lit).reshape(height, width)
    flag = (np.asarray(hits).reshape(height, width) > 1).copy()
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            # p over the pixels whose neighbour q = p + (dr, dc) is inside the frame
            pr = slice(max(0, -dr), height - max(0, dr))
            pc = slice(max(0, -dc), width - max(0, dc))
            qr = slice(max(0, dr), height - max(0, -dr))
            qc = slice(max(0, dc), width - max(0, -dc))
            far = (np.abs(cb[:, qr, qc] - cb[:, pr, pc]) > thr).any(axis=0)
            flag[pr, pc] |= (ident[qr, qc] != ident[pr, pc]) | (lit[qr, qc] != lit[pr, pc]) | far
    return flag.reshape(n).astype(np.uint8)


def pixel_list(mask) -> np.ndarray:
    """The flagged pixels in ascending pixel index, int32."""
    return np.nonzero(np.asarray(mask).reshape(-1))[0].astype(np.int32)


def sample_pixels(pixels, k: int, width: int) -> tuple:
    """(rows, cols) of the sample frame, each [len(pixels)*k*k]: ray j*k*k + sy*k + sx of listed pixel
    j = (r, c) is pixel (k*r + sy, k*c + sx) of the (k*width)-wide sample frame."""
    px = np.asarray(pixels, dtype=np.int64)
    r, c = px // width, px % width
    sy, sx = np.divmod(np.arange(k * k), k)
    rows = (k * r[:, None] + sy[None, :]).reshape(-1)
    cols = (k * c[:, None] + sx[None, :]).reshape(-1)
    return rows, cols


def gather_samples(frame, pixels, k: int, width: int) -> np.ndarray:
    """float64 [3, len(pixels)*k*k]: the samples of the listed pixels, in ray order, out of a whole
    sample frame [3, (k*height)*(k*width)]."""
    rows, cols = sample_pixels(pixels, k, width)
    return np.asarray(frame, dtype=np.float64)[:, rows * (k * width) + cols]


def scatter_ref(samples, k: int, n_flagged: int) -> np.ndarray:
    """float64 [3, n_flagged]: the resolve of each listed pixel's k*k samples ([3, n_flagged*k*k] in
    ray order): each listed pixel is a 1 x 1 frame of the resolve, samples row by row."""
    s = np.asarray(samples, dtype=np.float64).reshape(3, n_flagged, k * k)
    return resolve_ref(np.moveaxis(s, 1, 0), k, 1, 1)[..., 0].T if n_flagged else np.zeros((3, 0))


def adaptive_ref(base, sample_frame, mask, k: int, width: int, height: int) -> np.ndarray:
    """float64 [3, height*width]: where(mask, resolve_ref(sample frame), clip01(base)). ``0.0 + clip``
    for the unflagged pixels: the resolve with k = 1 adds the one sample to 0.0 and divides by 1.0."""
    full = resolve_ref(sample_frame, k, width, height)
    plain = (0.0 + clip01(base)) / 1.0
    return np.where(np.asarray(mask).astype(bool)[None, :], full, plain)
