"""PNG output with the standard library only (``zlib``, ``struct``).

:func:`write_png` writes 8-bit grey ``[H, W]`` or RGB ``[H, W, 3]`` arrays,
non-interlaced, every scanline with filter type 0. :func:`grid_png` lays ink
images out like ``render.svg.grid_strokes3``: ``maxcol`` cells per line, the
last line ragged, white background.
"""
from __future__ import annotations

import math
import struct
import zlib
from typing import Optional

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(array) -> bytes:
    a = np.asarray(array)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes a uint8 [H, W] or [H, W, 3] array, got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[0], a.shape[1]
    color_type = 0 if a.ndim == 2 else 2
    rows = np.ascontiguousarray(a).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()   # filter type 0 before every line
    ihdr = struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 9)) + _chunk(b"IEND", b"")


def write_png(path: str, array) -> None:
    data = png_bytes(array)
    with open(path, "wb") as f:
        f.write(data)


def grid_png(images, path: Optional[str] = "grid.png", maxcol: int = 5, margin: int = 2) -> Optional[np.ndarray]:
    """Grid of ``[n, S, S]`` ink images (floats in [0, 1], tensor or array;
    uint8 is taken as grey already), each in a cell of ``S + 2 * margin``
    pixels. Returns the ``[H, W]`` uint8 grid, ``None`` for no images."""
    from .raster import to_uint8
    grey = images if isinstance(images, np.ndarray) and images.dtype == np.uint8 else to_uint8(images)
    if grey.ndim != 3 or grey.shape[1] != grey.shape[2]:
        raise ValueError("grid_png takes [n, S, S] images, got %s" % (grey.shape,))
    if maxcol < 1 or margin < 0:
        raise ValueError("maxcol must be >= 1 and margin >= 0")
    n, S = grey.shape[0], grey.shape[1]
    if n == 0:
        return None
    cell = S + 2 * margin
    grid = np.full((math.ceil(n / maxcol) * cell, min(n, maxcol) * cell), 255, np.uint8)
    for k in range(n):
        y, x = (k // maxcol) * cell + margin, (k % maxcol) * cell + margin
        grid[y:y + S, x:x + S] = grey[k]
    if path:
        write_png(path, grid)
    return grid
