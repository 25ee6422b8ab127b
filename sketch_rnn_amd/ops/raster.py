"""Rasterise batches of stroke sequences into ``[B, S, S]`` ink images
(``csrc/raster.hip``).

One definition serves :func:`rasterize_torch` (the oracle), the kernel and the
tests.

**Input.** ``strokes [B, N, D]``: ``D = 3`` is stroke-3 ``(dx, dy, lift)``,
``D = 5`` magenta stroke-5 without the start token, whose lift is column 3 (as
in ``data.strokes.to_normal_strokes``). ``lengths [B]``: row ``t >=
lengths[b]`` takes part in nothing (a select before any arithmetic, as in
``ops.mdn_score``), so it may hold NaN. For ``D = 5``, ``lengths=None`` means
:func:`stroke5_lengths`.

**Points and segments.** ``P_0 = (0, 0)`` and ``P_{t+1} = P_t + (dx_t, dy_t)``
for ``t < L``. Segment ``P_t -> P_{t+1}`` is drawn iff ``1 <= t < L`` and
``lift[t-1] < 0.5``: the move from the origin to the first point is never
drawn (the pen rule of ``render.svg._polyline_paths``). A drawn segment of zero
length is a dot.

**Frame** ``(scale, ox, oy)``: a point ``P`` lands on pixel coordinates
``scale * P + (ox, oy)``. The bounding box is taken over ``P_0 .. P_L`` (the
origin included, as in ``render.svg._bounds3``); with ``e`` the larger of its
width and height, ``scale = (S - 2 * pad) / e`` if ``e > 0`` else 1, and
``(ox, oy)`` puts the box centre at ``(S / 2, S / 2)``. Pixel ``(row i, col
j)`` has its centre at ``(x, y) = (j + 0.5, i + 0.5)``; y grows downwards, as
in the SVGs. With ``frame [B, 3]`` given nothing is fitted and ink outside the
canvas is clipped.

**Ink** ``= clamp(width / 2 + 0.5 - d, 0, 1)`` with ``d`` the Euclidean
distance in pixels from the pixel centre to the nearest drawn segment (the
projection parameter clamped to [0, 1]; 0 for a zero-length segment); 0 with
no drawn segment. It is continuous in the inputs and, being a min over
segments, independent of their order.

The kernel path computes the points, the box and the point transform in fp64
and rounds the frame to fp32 before applying it, so the frame it returns,
handed back as ``frame=``, reproduces the image bit for bit; the per-pixel
arithmetic is fp32 and multiplies by ``1 / |b - a|^2`` where the transcription
divides (the distance is stationary in the projection parameter, so that
rounding is second order).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from ..utils import native

# False: every tile walks all drawn segments instead of the ones near it. The
# images are the same bit for bit (tests/test_raster_gpu.py); it exists for
# that test and for scripts/bench_raster.py.
CULL = True

MAX_SIZE = 512
# elements of the [pixels, segments] temporaries rasterize_torch holds at once
_TORCH_BUDGET = 1 << 22


def stroke5_lengths(strokes: torch.Tensor) -> torch.Tensor:
    """``[B]`` int64: the index of the first row of each stroke-5 sketch
    ``[B, N, 5]`` with ``p3 > 0`` (column 4), else ``N``.

    Deliberately not the rule of ``data.strokes.to_normal_strokes``, which
    treats an end-of-sketch in row 0 as "full length": here such a sketch has
    length 0."""
    if strokes.dim() != 3 or strokes.shape[-1] != 5:
        raise ValueError("stroke5_lengths takes [B, N, 5] strokes, got %s" % (tuple(strokes.shape),))
    B, N = strokes.shape[0], strokes.shape[1]
    if N == 0:
        return torch.zeros(B, dtype=torch.int64, device=strokes.device)
    idx = torch.arange(N, device=strokes.device).expand(B, N)
    return torch.where(strokes[..., 4] > 0, idx, torch.full_like(idx, N)).amin(dim=1)


def _check(strokes, lengths, size, width, pad, frame, out):
    """Validate the arguments; returns ``(lengths [B] int64 on the strokes'
    device, clamped to [0, N])``."""
    if not isinstance(strokes, torch.Tensor) or strokes.dim() != 3 or strokes.shape[-1] not in (3, 5):
        raise ValueError("strokes must be [B, N, 3] or [B, N, 5]")
    if not strokes.is_floating_point():
        raise ValueError("strokes must be a floating-point tensor")
    B, N, D = strokes.shape
    if isinstance(size, bool) or not isinstance(size, int) or not 1 <= size <= MAX_SIZE:
        raise ValueError("size must be an integer in 1..%d, got %r" % (MAX_SIZE, size))
    if not (math.isfinite(width) and width > 0):
        raise ValueError("width must be finite and > 0, got %r" % (width,))
    if not (math.isfinite(pad) and pad >= 0 and 2 * pad < size):
        raise ValueError("pad must satisfy 0 <= 2 * pad < size, got %r" % (pad,))
    if lengths is None:
        if D != 5:
            raise ValueError("stroke-3 input needs lengths")
        lengths = stroke5_lengths(strokes)
    else:
        lengths = torch.as_tensor(lengths)
        if lengths.shape != (B,) or lengths.is_floating_point() or lengths.dtype == torch.bool:
            raise ValueError("lengths must be [B] integers")
        lengths = lengths.to(device=strokes.device, dtype=torch.int64)
    if frame is not None:
        if not isinstance(frame, torch.Tensor) or frame.shape != (B, 3) or not frame.is_floating_point():
            raise ValueError("frame must be a [B, 3] floating-point tensor")
        # reading the values back is a synchronisation: not inside a graph capture
        capturing = frame.is_cuda and torch.cuda.is_current_stream_capturing()
        if not capturing and B and not bool((torch.isfinite(frame).all(dim=1) & (frame[:, 0] > 0)).all()):
            raise ValueError("frame must be finite with scale > 0")
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.shape != (B, size, size) or out.device != strokes.device
                or not out.is_contiguous()):
            raise ValueError("out must be a contiguous [B, size, size] tensor on the strokes' device")
    return lengths.clamp(0, N)


def rasterize_torch(strokes, lengths=None, size=64, width=1.0, pad=2.0, frame=None, out=None,
                    dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """The definition, transcribed. Every step runs in ``dtype`` (the oracle
    is fp64 on the CPU); returns ``(image [B, S, S], frame [B, 3])`` in it."""
    L = _check(strokes, lengths, size, width, pad, frame, out)
    if out is not None and out.dtype != dtype:
        raise ValueError("out must be %s" % dtype)
    B, N, D = strokes.shape
    S, dev = size, strokes.device
    zero, one = torch.zeros((), dtype=dtype, device=dev), torch.ones((), dtype=dtype, device=dev)
    t = torch.arange(N, device=dev).unsqueeze(0)
    live = t < L.unsqueeze(1)                                            # [B, N]
    s = strokes.to(dtype)
    # rows past the length are replaced before any arithmetic
    d = torch.where(live.unsqueeze(-1), s[..., 0:2], zero)
    lift = torch.where(live, s[..., 3 if D == 5 else 2], one)
    P = torch.cat([torch.zeros(B, 1, 2, dtype=dtype, device=dev), torch.cumsum(d, dim=1)], dim=1)   # P_0 .. P_N
    if frame is None:
        lo, hi = P.amin(dim=1), P.amax(dim=1)                            # [B, 2]; P_t = P_L for t > L
        e = (hi - lo).amax(dim=1)
        scale = torch.where(e > 0, (S - 2.0 * pad) / torch.where(e > 0, e, one), one)
        o = 0.5 * S - scale.unsqueeze(1) * (0.5 * (lo + hi))
        frame_used = torch.cat([scale.unsqueeze(1), o], dim=1)
    else:
        frame_used = frame.to(device=dev, dtype=dtype)
    Q = frame_used[:, 0:1].unsqueeze(-1) * P + frame_used[:, 1:3].unsqueeze(1)   # pixel coordinates
    prev_lift = torch.cat([torch.ones(B, 1, dtype=dtype, device=dev), lift[:, :-1]], dim=1) if N else lift
    drawn = (t >= 1) & live & (prev_lift < 0.5)                          # [B, N]
    image = out if out is not None else torch.empty(B, S, S, dtype=dtype, device=dev)
    if N == 0:
        image.zero_()
        return image, frame_used
    a, ab = Q[:, :-1], Q[:, 1:] - Q[:, :-1]                              # [B, N, 2]
    len2 = (ab * ab).sum(-1)                                             # [B, N]
    c = torch.arange(S, device=dev).to(dtype) + 0.5
    r = width / 2.0 + 0.5
    inf = torch.full((), math.inf, dtype=dtype, device=dev)
    nb = max(1, _TORCH_BUDGET // (S * S * N))
    nr = max(1, min(S, _TORCH_BUDGET // (S * N)))
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        ax, ay = a[b0:b1, None, None, :, 0], a[b0:b1, None, None, :, 1]  # [b, 1, 1, N]
        ux, uy = ab[b0:b1, None, None, :, 0], ab[b0:b1, None, None, :, 1]
        l2 = len2[b0:b1, None, None, :]
        for r0 in range(0, S, nr):
            r1 = min(S, r0 + nr)
            vx = c[None, None, :, None] - ax                             # [b, 1, S, N]
            vy = c[None, r0:r1, None, None] - ay                         # [b, rows, 1, N]
            tt = torch.where(l2 > 0, (vx * ux + vy * uy) / torch.where(l2 > 0, l2, one), zero).clamp(0.0, 1.0)
            qx, qy = vx - tt * ux, vy - tt * uy
            d2 = torch.where(drawn[b0:b1, None, None, :], qx * qx + qy * qy, inf).amin(dim=-1)
            image[b0:b1, r0:r1] = (r - torch.sqrt(d2)).clamp(0.0, 1.0)
    return image, frame_used


def rasterize_hip(strokes, lengths=None, size=64, width=1.0, pad=2.0, frame=None, out=None):
    """The kernel path: fp32 ``(image, frame)`` of CUDA strokes. Allocates by
    shape only and never synchronises (a given ``frame`` is validated by value
    outside a graph capture only), so the call can be captured in a HIP graph."""
    from ._hipapi import RasterArgs
    lib = native.require_hip()
    if not (isinstance(strokes, torch.Tensor) and strokes.is_cuda):
        raise ValueError("rasterize_hip takes CUDA strokes")
    L = _check(strokes, lengths, size, width, pad, frame, out)
    if out is not None and out.dtype != torch.float32:
        raise ValueError("out must be float32")
    B, N, D = strokes.shape
    dev = strokes.device
    x = strokes.detach().contiguous().float()
    L = L.contiguous()
    image = out if out is not None else torch.empty(B, size, size, device=dev, dtype=torch.float32)
    frame_used = torch.empty(B, 3, device=dev, dtype=torch.float32)
    seg = torch.empty(B, max(N, 1), 4, device=dev, dtype=torch.float32)
    count = torch.empty(max(B, 1), device=dev, dtype=torch.int32)
    fin = None if frame is None else frame.detach().to(device=dev, dtype=torch.float32).contiguous()
    a = RasterArgs()
    a.strokes, a.lengths, a.frame_in = x.data_ptr(), L.data_ptr(), (fin.data_ptr() if fin is not None else None)
    a.frame, a.seg, a.count, a.out = frame_used.data_ptr(), seg.data_ptr(), count.data_ptr(), image.data_ptr()
    a.B, a.N, a.D, a.S = B, N, D, size
    a.width, a.pad, a.cull, a.b0 = float(width), float(pad), int(bool(CULL)), 0
    with torch.cuda.device(dev):
        rc = lib.lib.skr_raster(C.byref(a), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("skr_raster failed (%d)" % rc)
    return image, frame_used


def rasterize(strokes, lengths=None, size=64, width=1.0, pad=2.0, frame=None,
              out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(image [B, S, S], frame [B, 3])``, both float32: the kernel for CUDA
    float32 strokes when the HIP backend is on, the fp32 transcription otherwise."""
    from . import use_hip
    if isinstance(strokes, torch.Tensor) and strokes.is_cuda and strokes.dtype == torch.float32 and use_hip(strokes):
        return rasterize_hip(strokes, lengths, size, width, pad, frame, out)
    return rasterize_torch(strokes, lengths, size, width, pad, frame, out, dtype=torch.float32)
