"""Per-sketch likelihood scores of the MDN head (``csrc/mdn_score.hip``).

``shape[t, b]`` and ``pen[t, b]`` are the per-row terms of
``models.mdn.mdn_loss_torch(mode="magenta", is_training=False)`` before its
mask and mean: ``shape = -logaddexp(log S, log eps)`` and ``pen`` the softmax
cross-entropy of the three pen logits. The scores sum them over each
sketch's real positions::

    score_shape[b] = sum_{t < len[b]} shape[t, b]
    score_pen[b]   = sum_{t < len[b]} pen[t, b]   (+ pen[len[b], b] with
                     include_end when len[b] < T: the end-of-sketch row)

The mask is a select on ``lengths``: rows past a sketch's counted positions
contribute exactly zero whatever they contain.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from ..utils import native

# Work groups the time slabs aim for (ceil(B / 16) sketch blocks x S slabs):
# a slab costs nothing extra (every 4-step round streams W^T once whatever
# slab it belongs to), so the grid is cut fine enough to fill 256 CUs twice.
SCORE_TARGET_WGS = 1024


def score_fused_ok(x: torch.Tensor, W: torch.Tensor, M: int) -> bool:
    """The score kernel applies where the fused head does (``head_fused_ok``):
    bf16 HIP compute, ``M <= 24``, a decoder width that is a multiple of 128."""
    from . import gemm, use_hip
    return (x.is_cuda and use_hip(x) and gemm.lp_dtype() == torch.bfloat16 and 1 <= M <= 24 and x.numel() > 0
            and W.shape[0] % 128 == 0 and W.shape[1] == 3 + 6 * M)


def _masks(lengths: torch.Tensor, T: int, include_end: bool):
    t = torch.arange(T, device=lengths.device).unsqueeze(1)
    L = lengths.to(torch.int64).clamp(0, T).unsqueeze(0)
    return t < L, t < L + (1 if include_end else 0)


def mdn_head_score_torch(x, W, b, target, lengths, M, include_end=False, eps=1e-6):
    """PyTorch form of the definition (CPU, fp32 and ineligible shapes)."""
    from . import gemm
    from ..models.mdn import log_mixture_density
    T, B = target.shape[0], target.shape[1]
    m_shape, m_pen = _masks(lengths, T, include_end)
    # uncounted rows are replaced before any arithmetic: whatever they hold never reaches a sum
    xs = torch.where(m_pen.unsqueeze(-1), x.reshape(T, B, -1), torch.zeros((), dtype=x.dtype, device=x.device))
    tg = torch.where(m_pen.unsqueeze(-1), target.float(), torch.zeros((), device=target.device))
    z = gemm.linear(xs.reshape(T * B, -1), W, b).float()
    tg = tg.reshape(T * B, 5)
    logS = log_mixture_density(z, tg[:, 0], tg[:, 1], M)
    shape = -torch.logaddexp(logS, torch.full_like(logS, math.log(eps)))
    pen = -(tg[:, 2:5] * torch.log_softmax(z[:, 0:3], -1)).sum(-1)
    zero = torch.zeros((), device=z.device)
    return (torch.where(m_shape, shape.view(T, B), zero).sum(0),
            torch.where(m_pen, pen.view(T, B), zero).sum(0))


def _padded_wt(W: torch.Tensor) -> torch.Tensor:
    Hd, NOUT = W.shape
    Wt = torch.zeros((NOUT + 31) // 32 * 32, Hd, device=W.device, dtype=torch.bfloat16)
    Wt[:NOUT] = W.detach().t()
    return Wt


def slabs(T: int, B: int):
    """``(tps, S)``: time steps per slab (a multiple of the 4 steps of a
    round) and the number of slabs."""
    nblk = -(-B // 16)
    S = max(1, min(-(-T // 4), SCORE_TARGET_WGS // nblk))
    tps = -(-(-(-T // S)) // 4) * 4
    return tps, -(-T // tps)


def mdn_head_score_hip(x, W, b, target, lengths, M, include_end=False, eps=1e-6, x_lp=None):
    from ._hipapi import HeadScore
    from . import gemm
    from .mdn_hip import _lp_rows
    lib = native.require_hip()
    T, B = target.shape[0], target.shape[1]
    Hd, NOUT = W.shape
    dev = x.device
    XL = _lp_rows(x_lp, x, Hd)
    a = HeadScore()
    if XL is not None:
        a.X, a.ldx, a.x_bf16 = XL.data_ptr(), XL.stride(0), 1
    else:
        X2 = x.detach().reshape(T * B, Hd).contiguous().float()
        a.X, a.ldx, a.x_bf16 = X2.data_ptr(), X2.stride(0), 0
    Wt = gemm.derived(W, "score_wt", _padded_wt)   # inference: made once per weight version
    bias = b.detach().contiguous().float()
    tgt = target.detach().reshape(T * B, 5).contiguous().float()
    lens = lengths.to(device=dev, dtype=torch.int64).contiguous()
    tps, S = slabs(T, B)
    part = torch.empty(S, B, 2, device=dev, dtype=torch.float32)
    score = torch.empty(B, 2, device=dev, dtype=torch.float32)
    a.Hd, a.Wt, a.bias, a.tgt, a.ldt, a.lengths = Hd, Wt.data_ptr(), bias.data_ptr(), tgt.data_ptr(), 5, lens.data_ptr()
    a.T, a.B, a.M, a.NOUT, a.NOUTP, a.include_end = T, B, M, NOUT, Wt.shape[0], int(bool(include_end))
    a.tps, a.S, a.log_floor = tps, S, math.log(eps)
    a.part, a.score = part.data_ptr(), score.data_ptr()
    rc = lib.lib.skr_mdn_head_score(C.byref(a), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("skr_mdn_head_score failed (%d)" % rc)
    return score[:, 0], score[:, 1]
