"""Interleaved row tiling of a frame across ranks (the multi-GPU split of SURVEY.md §8e).

Rows are cut in blocks of ``row_block``; block b belongs to part ``b % n_parts``. A rank may render
a run of consecutive parts (a larger or smaller share of the frame, ``runs``): part_run *
row_block consecutive rows of every cycle. Interleaving
balances the load: sky rows (no hit, ~15 flops/pixel) and ground rows (thousands) alternate
across ranks instead of landing on one rank as contiguous strips would. Local row ``lr`` of part
``p`` is global row ``((lr // rb) * P + p) * rb + lr % rb`` — the mapping the kernel uses
(``global_row`` in rtx_device.h).

Gather layout: every part travels as one flat buffer of ``part_len`` elements (the same length on
every rank, as a collective needs), holding that part's tile exactly as ``render_tile`` returns
it — colour ``[3, rows_p*W]`` or uint8 ``[rows_p, W, 3]`` — at its start. ``assemble`` is the
host-side un-permute of such buffers (CPU tensors / NumPy); on the GPU the same layout is
un-permuted by ``rtx_assemble_rows``.
"""

from __future__ import annotations

import numpy as np


def n_local_rows(height: int, row_block: int, n_parts: int, part: int, run: int = 1) -> int:
    """Rows of the run of ``run`` consecutive parts from ``part``: run * row_block rows of every
    cycle of n_parts * row_block rows (the last cycle's prefix)."""
    if row_block <= 0 or n_parts <= 0 or run <= 0 or not 0 <= part <= n_parts - run:
        raise ValueError(f"bad tiling: row_block={row_block} n_parts={n_parts} part={part} run={run}")
    cycle, own = row_block * n_parts, row_block * run
    q, rem = divmod(int(height), cycle)
    return q * own + min(max(rem - part * row_block, 0), own)


def tile_rows(height: int, row_block: int, n_parts: int, part: int, run: int = 1) -> np.ndarray:
    """Global row index of each local row of the run of ``run`` parts from ``part`` (ascending)."""
    n = n_local_rows(height, row_block, n_parts, part, run)
    lr = np.arange(n)
    own = row_block * run
    return (lr // own) * (n_parts * row_block) + part * row_block + lr % own


MAX_SAMPLES = 8  # samples per pixel side of a supersampled render (rtx_resolve_samples)
SAMPLE_LIMIT = 1 << 31  # k*k*width*rows*frames stays below it: the resolve indexes pixels in 32 bits


def check_samples(k) -> int:
    """``k``, the samples per pixel side of a supersampled render: an int in 1..MAX_SAMPLES."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_SAMPLES:
        raise ValueError(f"samples must be an int in 1..{MAX_SAMPLES} (samples per pixel side), got {k!r}")
    return int(k)


def sample_tiling(height: int, row_block: int, k: int) -> tuple:
    """(height, row_block) of the sample frame of a supersampled render: k sample rows per row, so
    row blocks of k * row_block sample rows. With the same n_parts, part and run, the tile's
    sample rows are the k rows of each of its rows, in its local order: local sample row
    k * lr + sy is global sample row k * tile_rows[lr] + sy. A partial last block stays whole:
    k H - m k rb = k (H - m rb)."""
    return int(k) * int(height), int(k) * int(row_block)


def n_sample_rows(height: int, row_block: int, n_parts: int, part: int, run: int = 1, k: int = 1) -> int:
    """Sample rows of a tile of a supersampled render: k * n_local_rows."""
    return n_local_rows(*sample_tiling(height, row_block, k), n_parts, part, run)


def sample_tile_rows(height: int, row_block: int, n_parts: int, part: int, run: int = 1, k: int = 1) -> np.ndarray:
    """Global sample row of each local sample row of a tile of a supersampled render."""
    return tile_rows(*sample_tiling(height, row_block, k), n_parts, part, run)


def check_sample_count(k: int, width: int, rows: int, frames: int = 1) -> int:
    """Samples per colour plane of a supersampled render, k*k*width*rows*frames; ValueError at
    SAMPLE_LIMIT (2^31) and beyond, where rtx_resolve_samples refuses."""
    n = int(k) * int(k) * int(width) * int(rows) * int(frames)
    if n >= SAMPLE_LIMIT:
        raise ValueError(f"samples={k}: {k}x{k} samples of {width}x{rows} pixels x {frames} frame(s) = {n} "
                         f"samples per plane, the resolve takes fewer than 2^31; render row tiles (render_tile)")
    return n


def check_adaptive(adaptive, samples: int, contrast):
    """The arguments of an adaptive render (HipRenderer(samples=k, adaptive=True, contrast=c)) as
    (adaptive, contrast): ``adaptive`` a bool that needs samples >= 2; ``contrast`` None (no colour
    test: +inf) or a finite number >= 0. ValueError otherwise."""
    if not isinstance(adaptive, (bool, np.bool_)):
        raise ValueError(f"adaptive must be a bool, got {adaptive!r}")
    if adaptive and samples < 2:
        raise ValueError(f"adaptive=True refines edge pixels with samples x samples rays: it needs samples >= 2, "
                         f"got samples={samples}")
    if contrast is None:
        return bool(adaptive), float("inf")
    if isinstance(contrast, bool) or not isinstance(contrast, (int, float, np.integer, np.floating)) \
            or not np.isfinite(contrast) or contrast < 0:
        raise ValueError(f"contrast must be None (adaptive: the geometric test alone) or a finite number >= 0, "
                         f"got {contrast!r}")
    return bool(adaptive), float(contrast)


def check_adaptive_count(k: int, width: int, height: int, flagged: int | None = None) -> int:
    """Sample rays of an adaptive render, flagged*k*k (``flagged=None``: before the mask is known,
    the frame alone); ValueError where rtx_edge_mask / rtx_sample_dirs / rtx_resolve_scatter refuse:
    width*height or flagged*k*k at SAMPLE_LIMIT (2^31) and beyond."""
    n = int(width) * int(height)
    if n >= SAMPLE_LIMIT:
        raise ValueError(f"adaptive: {width}x{height} = {n} pixels, the edge mask takes fewer than 2^31")
    if flagged is None:
        return 0
    rays = int(flagged) * int(k) * int(k)
    if not 0 <= int(flagged) <= n or rays >= SAMPLE_LIMIT:
        raise ValueError(f"adaptive: {flagged} flagged pixels of {n} x {k}x{k} samples = {rays} sample rays, "
                         f"the resolve takes fewer than 2^31; lower samples or raise contrast")
    return rays


def runs(world: int, root_run: int = 1, run: int = 1):
    """(n_parts, [(first part, run) per rank]) of the shares: rank 0 renders parts [0, root_run),
    rank i >= 1 parts [root_run + (i - 1) run, root_run + i run)."""
    n_parts = root_run + (world - 1) * run
    return n_parts, [(0, root_run)] + [(root_run + (i - 1) * run, run) for i in range(1, world)]


def max_local_rows(height: int, row_block: int, n_parts: int) -> int:
    return n_local_rows(height, row_block, n_parts, 0)  # part 0 has the most rows


def tile_shape(height: int, width: int, row_block: int, n_parts: int, part: int, out: str | None = None,
               run: int = 1):
    """Shape ``render_tile`` returns for this part (or run of parts): (3, rows*W) colour or
    (rows, W, 3) uint8."""
    rows = n_local_rows(height, row_block, n_parts, part, run)
    return (rows, int(width), 3) if out == "u8" else (3, rows * int(width))


def part_len(height: int, width: int, row_block: int, n_parts: int, itemsize: int, out: str | None = None,
             root_run: int = 1, run: int = 1) -> int:
    """Elements of one gather buffer: the largest rank's tile (``n_parts`` ranks, shares as in
    ``runs``), rounded up to 16 bytes (so every tile of a [ranks, part_len] buffer starts 16-byte
    aligned for the device copy)."""
    np_, shares = runs(n_parts, root_run, run)
    n = 3 * max(n_local_rows(height, row_block, np_, f, k) for f, k in shares) * int(width)
    per16 = max(1, 16 // itemsize)
    return (n + per16 - 1) // per16 * per16


def assemble(tiles, height: int, width: int, row_block: int, out: str | None = None, root_run: int = 1,
             run: int = 1):
    """Un-permute gathered rank buffers ``tiles[r]`` (each ``part_len`` long, layout above; shares
    as in ``runs``) into one frame: [3, H*W] colour or [H, W, 3] uint8 (``out="u8"``). Torch tensors
    or NumPy arrays."""
    import torch

    n_parts, shares = runs(len(tiles), root_run, run)
    first = tiles[0]
    is_torch = isinstance(first, torch.Tensor)
    shape = (height, width, 3) if out == "u8" else (3, height, width)
    full = (torch.empty(shape, dtype=first.dtype, device=first.device) if is_torch
            else np.empty(shape, dtype=first.dtype))
    for p, (f, k_run) in enumerate(shares):
        rows = tile_rows(height, row_block, n_parts, f, k_run)
        k = len(rows)
        if k == 0:
            continue
        idx = torch.as_tensor(rows, device=first.device) if is_torch else rows
        src = tiles[p][:3 * k * width]
        if out == "u8":
            full[idx] = src.reshape(k, width, 3)
        else:
            full[:, idx] = src.reshape(3, k, width)
    return full if out == "u8" else full.reshape(3, height * width)
