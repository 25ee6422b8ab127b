"""Pixel-space helpers over the ink images of ``ops.raster.rasterize``."""
from __future__ import annotations

import numpy as np
import torch


def soft_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``[B]``: ``sum(min(a, b)) / sum(max(a, b))`` over each pair of ink
    images ``[B, S, S]``; 1 where both are blank."""
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError("soft_iou takes two [B, S, S] batches of one shape, got %s and %s"
                         % (tuple(a.shape), tuple(b.shape)))
    inter = torch.minimum(a, b).flatten(1).sum(1)
    union = torch.maximum(a, b).flatten(1).sum(1)
    return torch.where(union > 0, inter / torch.where(union > 0, union, torch.ones_like(union)),
                       torch.ones_like(union))


def to_uint8(image) -> np.ndarray:
    """Ink in [0, 1] (tensor or array, any shape) as 8-bit grey: black ink on white."""
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu().numpy()
    ink = np.clip(np.asarray(image, dtype=np.float64), 0.0, 1.0)
    return (255 - np.rint(ink * 255.0)).astype(np.uint8)
