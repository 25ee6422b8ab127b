"""Training batches assembled from a concatenated corpus (``csrc/batch.hip``):
a stateless epoch shuffle, per-sketch random scaling, the point-drop
augmentation and padding to magenta stroke-5.

One definition serves :func:`assemble_reference` (the oracle), the kernel and
the tests. Every random draw is a hash of ``(seed, stream, step, index)``
(``mix32`` / ``hash_key`` / ``hash_uniform`` of ``csrc/common.h``, mirrored in
``models/cells.py``), so a batch is a pure function of its arguments: there is
no RNG state to save, and the rows of a global batch do not depend on how many
ranks share it.

**Corpus** (:class:`Corpus`). ``points [P, 3] float32`` are the stroke-3 rows
``(dx, dy, lift)`` of all sketches, ``offsets [S + 1] int64`` (sketch ``i`` is
rows ``offsets[i]:offsets[i + 1]``), ``labels [S] int64``. ``1 <= S <= 2^30``
and ``lift`` is 0 or 1; every length ``n_i`` is at most ``Nmax`` (checked when
the corpus is built, and per call against the call's ``Nmax``).

**Selection.** Row ``b`` of the call is global row ``g = row0 + b`` of a global
batch of ``G = world_rows`` rows (``row0 = rank * B``, ``G = B * world``).
With ``q = step * G + g`` (int64), ``epoch = q // S`` and ``p = q % S``:

* ``key = hash_key(seed, STREAM_SHUFFLE, epoch mod 2^32)``;
* ``k >= 1`` is the smallest integer with ``4^k >= S`` and ``mask = 2^k - 1``;
* ``x = p``; then, until ``x < S`` (cycle walking; at least once): ``L = x >>
  k``, ``R = x & mask``; four rounds ``(L, R) = (R, L ^ (mix32(R ^ mix32(key +
  r)) & mask))`` for ``r = 0..3``, all in uint32; ``x = (L << k) | R``;
* ``index = x``.

The Feistel map is a bijection of ``[0, 4^k)``, so the walk ends and the ``S``
positions of an epoch visit every sketch exactly once. ``indices [B]`` given
explicitly bypass the selection.

**Scale.** For ``axis`` in (0, 1): ``u = hash_uniform(hash_key(seed,
STREAM_SCALE, step mod 2^32), (2 g + axis) mod 2^32)``, ``s = ((u - 0.5f) *
2.0f) * f + 1.0f`` with every operation a single fp32 operation (no
contraction; ``f`` is rounded to fp32 first), and ``x'_t = fp32(x_t * s)``.
``f = 0`` gives ``s = 1``: the values are untouched.

**Drop.** For ``t < n``: ``lift_t = (points[t, 2] == 1)``, ``lift_{-1}`` is
true, ``first_t`` is the greatest ``r <= t`` with ``lift_{r-1}``, ``elig_t =
!lift_t && !lift_{t-1} && t - first_t > 2``, ``u_t = hash_uniform(hash_key(
seed, STREAM_DROP, step mod 2^32), (g Nmax + t) mod 2^32)`` and ``drop_t =
elig_t && fp64(u_t) < prob``. This is ``data.strokes.augment_strokes`` fed the
same uniforms: its ``prev[2]`` is always the lift of the previous source row
and its ``count`` the distance from the stroke's first point. The kept points
``k_0 < k_1 < ...`` are the rest. Output point ``j`` has ``x = fp32(x'_{k_j} +
x'_{k_j + 1} + ...)`` over the dropped points that follow ``k_j``, summed in
fp64 one at a time in ascending ``t`` (``y`` alike), and the pen of row
``k_j``. ``prob = 0`` drops nothing.

**Output**, every element written: ``strokes [B, Nmax + 1, 5] float32`` with
row 0 ``(0, 0, 1, 0, 0)``, row ``j + 1`` ``(x, y, 1 - lift, lift, 0)`` and the
rows past the new length ``(0, 0, 0, 0, 1)``; ``lengths [B] int64`` (the number
of kept points); ``labels [B] int64``.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ..utils import native

MAX_N = 2048          # as ops.simplify
MAX_S = 1 << 30       # the shuffle's Feistel state is 2 k <= 30 bits of a uint32

# Hash streams. In use elsewhere in the tree, each also at +1 (the hyper cell's
# second mask) and at + 0x3C6EF372 (hash_normal's second uniform): 0 (the
# default of every drop_stream argument), 7 (models/reference.py), 11, 13, 17,
# 23, 29, 31 (models/vae.py), 0x5A3D (sample/sampler.py).
STREAM_SHUFFLE = 37
STREAM_SCALE = 41
STREAM_DROP = 43

_M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------
# the hash of csrc/common.h on Python integers and on uint64 arrays
# ------------------------------------------------------------------------------------
def mix32(x):
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint64) & np.uint64(_M32)
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x7FEB352D)) & np.uint64(_M32)
        x = x ^ (x >> np.uint64(15))
        x = (x * np.uint64(0x846CA68B)) & np.uint64(_M32)
        return x ^ (x >> np.uint64(16))
    x = int(x) & _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def hash_key(seed: int, stream: int, step: int) -> int:
    return mix32(((int(seed) & _M32) * 0x9E3779B1 + (stream & _M32) * 0x85EBCA77 + (int(step) & _M32) * 0xC2B2AE3D) & _M32)


def hash_uniform(key: int, idx):
    """float32 U[0, 1) of ``idx mod 2^32``: a Python integer or an integer array."""
    if isinstance(idx, np.ndarray):
        i = idx.astype(np.int64).astype(np.uint64) & np.uint64(_M32)
        h = mix32(i ^ np.uint64(key))
        h = mix32(h + np.uint64(key))
        return (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    h = mix32((int(idx) & _M32) ^ key)
    h = mix32(h + key)
    return np.float32(h >> 8) * np.float32(1.0 / 16777216.0)


def feistel_bits(S: int) -> int:
    k = 1
    while (1 << (2 * k)) < S:
        k += 1
    return k


def shuffle_positions(seed: int, epoch: int, p: np.ndarray, S: int) -> np.ndarray:
    """The sketches at positions ``p`` (integers in ``[0, S)``) of one epoch, int64."""
    key = hash_key(seed, STREAM_SHUFFLE, epoch)
    k = np.uint64(feistel_bits(S))
    mask = np.uint64((1 << int(k)) - 1)
    x = np.asarray(p, np.int64).astype(np.uint64).reshape(-1)
    todo = np.ones(len(x), bool)                      # every position walks at least once
    while todo.any():
        L, R = x[todo] >> k, x[todo] & mask
        for r in range(4):
            L, R = R, L ^ (mix32(R ^ np.uint64(mix32((key + r) & _M32))) & mask)
        x[todo] = (L << k) | R
        todo = x >= np.uint64(S)
    return x.astype(np.int64)


def shuffle_index(seed: int, step: int, g: int, G: int, S: int) -> int:
    """The sketch that global row ``g`` of step ``step`` trains on."""
    epoch, p = divmod(int(step) * int(G) + int(g), S)
    return int(shuffle_positions(seed, epoch, np.asarray([p]), S)[0])


def scale_factors(seed: int, step: int, g: int, f: float) -> Tuple[np.float32, np.float32]:
    key = hash_key(seed, STREAM_SCALE, step)
    f32 = np.float32(f)
    return tuple(((hash_uniform(key, 2 * g + axis) - np.float32(0.5)) * np.float32(2.0)) * f32 + np.float32(1.0)
                 for axis in (0, 1))


def drop_uniforms(seed: int, step: int, g: int, Nmax: int, n: int) -> np.ndarray:
    """``u_t`` float32 for ``t < n``."""
    return hash_uniform(hash_key(seed, STREAM_DROP, step), int(g) * int(Nmax) + np.arange(n, dtype=np.int64))


def eligible(lift: np.ndarray) -> np.ndarray:
    """``elig_t`` of one sketch from its lift flags."""
    n = len(lift)
    lift = np.asarray(lift, bool)
    prev = np.concatenate([[True], lift[:-1]]) if n else np.zeros(0, bool)
    t = np.arange(n)
    first = np.maximum.accumulate(np.where(prev, t, 0)) if n else t
    return ~lift & ~prev & (t - first > 2)


# ------------------------------------------------------------------------------------
# corpus
# ------------------------------------------------------------------------------------
class Corpus(NamedTuple):
    points: torch.Tensor     # [P, 3] float32
    offsets: torch.Tensor    # [S + 1] int64
    labels: torch.Tensor     # [S] int64
    max_len: int             # the longest sketch

    @property
    def S(self) -> int:
        return self.labels.shape[0]

    def to(self, device) -> "Corpus":
        return Corpus(self.points.to(device), self.offsets.to(device), self.labels.to(device), self.max_len)


def make_corpus(strokes: Sequence[np.ndarray], labels=None, Nmax: Optional[int] = None, device="cpu") -> Corpus:
    """Concatenate stroke-3 sketches. Raises ``ValueError`` for a sketch longer
    than ``Nmax``, a lift that is neither 0 nor 1, or a size the shuffle cannot
    address."""
    S = len(strokes)
    if not 1 <= S <= MAX_S:
        raise ValueError("a corpus holds 1 .. 2^30 sketches, got %d" % S)
    lens = np.asarray([len(s) for s in strokes], np.int64)
    if Nmax is not None and int(lens.max()) > Nmax:
        raise ValueError("sketch %d has %d points, more than Nmax = %d" % (int(lens.argmax()), int(lens.max()), Nmax))
    offsets = np.zeros(S + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    rows = [np.asarray(s, np.float32).reshape(-1, 3) for s in strokes]
    points = np.concatenate(rows, 0) if offsets[-1] else np.zeros((0, 3), np.float32)
    if not bool(np.isin(points[:, 2], (0.0, 1.0)).all()):
        raise ValueError("the lift column must hold 0 or 1")
    lab = np.zeros(S, np.int64) if labels is None else np.asarray(labels, np.int64).reshape(-1)
    if lab.shape != (S,):
        raise ValueError("labels must be [S]")
    if len(points) == 0:               # the kernel takes no null pointer: one row that no sketch owns
        points = np.zeros((1, 3), np.float32)
    return Corpus(torch.from_numpy(np.ascontiguousarray(points)), torch.from_numpy(offsets),
                  torch.from_numpy(lab), int(lens.max())).to(device)


# ------------------------------------------------------------------------------------
# checks shared by the reference and the kernel path
# ------------------------------------------------------------------------------------
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check(corpus, Nmax, B, seed, step, row0, world_rows, f, prob, indices, out, trusted=False):
    if not isinstance(corpus, Corpus):
        raise ValueError("corpus must be an ops.batch.Corpus")
    if not _is_int(Nmax) or not 1 <= Nmax <= MAX_N:
        raise ValueError("Nmax must be in 1..%d, got %r" % (MAX_N, Nmax))
    if corpus.max_len > Nmax:
        raise ValueError("the corpus holds a sketch of %d points, more than Nmax = %d" % (corpus.max_len, Nmax))
    if not _is_int(B) or B < 0:
        raise ValueError("B must be an integer >= 0")
    if not (_is_int(seed) and _is_int(step) and _is_int(row0)) or step < 0 or row0 < 0:
        raise ValueError("seed, step and row0 are integers, step and row0 >= 0")
    G = max(row0 + B, 1) if world_rows is None else world_rows
    if not _is_int(G) or G < max(row0 + B, 1):
        raise ValueError("world_rows must be an integer >= row0 + B")
    if (step + 1) * G >= 1 << 62:
        raise ValueError("step * world_rows does not fit an int64")
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 <= prob <= 1.0:
        raise ValueError("augment_stroke_prob must be in [0, 1], got %r" % (prob,))
    if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 <= f < 1.0:
        raise ValueError("random_scale_factor must be in [0, 1), got %r" % (f,))
    dev = corpus.points.device
    if indices is not None:
        if not isinstance(indices, torch.Tensor):
            arr = np.asarray(indices)
            if arr.dtype.kind not in "iu":
                raise ValueError("indices must be integers")
            indices = torch.from_numpy(arr.astype(np.int64))
        if indices.dtype != torch.int64 or indices.shape != (B,):
            raise ValueError("indices must be [B] int64")
        # reading device values back is a synchronisation: not inside a graph capture
        capturing = indices.is_cuda and torch.cuda.is_current_stream_capturing()
        if not trusted and not capturing and B and not bool(((indices >= 0) & (indices < corpus.S)).all()):
            raise ValueError("indices must be in [0, %d)" % corpus.S)
        indices = indices.to(dev).contiguous()
    if out is not None:
        s, l, c = out
        for t, shape, dt in ((s, (B, Nmax + 1, 5), torch.float32), (l, (B,), torch.int64), (c, (B,), torch.int64)):
            if not (isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == dt and t.device == dev
                    and t.is_contiguous()):
                raise ValueError("out must be contiguous (strokes [B, Nmax + 1, 5] float32, lengths [B] int64, "
                                 "labels [B] int64) on the corpus' device")
    return G, indices


# ------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------
def assemble_one(rows: np.ndarray, seed: int, step: int, g: int, Nmax: int, f: float, prob: float):
    """One sketch through scale and drop: ``(xy [n', 2] float32, lift [n'] bool)``."""
    n = len(rows)
    sx, sy = scale_factors(seed, step, g, f)
    x = rows[:, 0].astype(np.float32) * sx            # fp32 products
    y = rows[:, 1].astype(np.float32) * sy
    lift = rows[:, 2] == 1
    drop = eligible(lift) & (drop_uniforms(seed, step, g, Nmax, n).astype(np.float64) < prob)
    keep = np.nonzero(~drop)[0]
    xy = np.zeros((len(keep), 2), np.float32)
    for j, k in enumerate(keep.tolist()):
        ax, ay = float(x[k]), float(y[k])             # fp64
        t = k + 1
        while t < n and drop[t]:
            ax += float(x[t])
            ay += float(y[t])
            t += 1
        xy[j] = (np.float32(ax), np.float32(ay))
    return xy, lift[keep]


def assemble_reference(corpus: Corpus, Nmax: int, B: int, *, seed: int, step: int, row0: int = 0,
                       world_rows: Optional[int] = None, random_scale_factor: float = 0.0,
                       augment_stroke_prob: float = 0.0, indices=None, out=None):
    """The definition on the host: NumPy, one sketch at a time. Returns
    ``(strokes, lengths, labels)`` on the CPU, or fills ``out``."""
    G, indices = _check(corpus, Nmax, B, seed, step, row0, world_rows, random_scale_factor, augment_stroke_prob,
                        indices, out)
    pts = corpus.points.cpu().numpy()
    offs = corpus.offsets.cpu().numpy()
    labs = corpus.labels.cpu().numpy()
    S = corpus.S
    strokes = np.zeros((B, Nmax + 1, 5), np.float32)
    lengths = np.zeros(B, np.int64)
    labels = np.zeros(B, np.int64)
    idx = None if indices is None else indices.cpu().numpy()
    for b in range(B):
        g = row0 + b
        i = int(idx[b]) if idx is not None else shuffle_index(seed, step, g, G, S)
        xy, lift = assemble_one(pts[offs[i]:offs[i + 1]], seed, step, g, Nmax, random_scale_factor,
                                float(augment_stroke_prob))
        m = len(xy)
        strokes[b, 0] = (0, 0, 1, 0, 0)
        strokes[b, 1:m + 1, 0:2] = xy
        strokes[b, 1:m + 1, 3] = lift
        strokes[b, 1:m + 1, 2] = 1 - strokes[b, 1:m + 1, 3]
        strokes[b, m + 1:, 4] = 1
        lengths[b] = m
        labels[b] = labs[i]
    res = (torch.from_numpy(strokes), torch.from_numpy(lengths), torch.from_numpy(labels))
    if out is not None:
        for dst, src in zip(out, res):
            dst.copy_(src)
        return tuple(out)
    return res


# ------------------------------------------------------------------------------------
# kernel path
# ------------------------------------------------------------------------------------
def assemble_hip(corpus: Corpus, Nmax: int, B: int, *, seed: int, step: int, row0: int = 0,
                 world_rows: Optional[int] = None, random_scale_factor: float = 0.0,
                 augment_stroke_prob: float = 0.0, indices=None, out=None, _trusted_indices: bool = False):
    """The kernel path for a corpus on the GPU: one launch on the current
    stream, no synchronisation (device ``indices`` are validated by value,
    which reads them back, outside a graph capture only)."""
    if not (isinstance(corpus, Corpus) and corpus.points.is_cuda):
        raise ValueError("the kernel path takes a corpus on the GPU")
    G, indices = _check(corpus, Nmax, B, seed, step, row0, world_rows, random_scale_factor, augment_stroke_prob,
                        indices, out, trusted=_trusted_indices)
    from ._hipapi import BatchArgs
    lib = native.require_hip()
    dev = corpus.points.device
    if out is None:
        out = (torch.empty(B, Nmax + 1, 5, device=dev, dtype=torch.float32),
               torch.empty(B, device=dev, dtype=torch.int64), torch.empty(B, device=dev, dtype=torch.int64))
    if B == 0:
        return tuple(out)
    a = BatchArgs()
    a.points, a.offsets, a.labels_in = corpus.points.data_ptr(), corpus.offsets.data_ptr(), corpus.labels.data_ptr()
    a.indices = indices.data_ptr() if indices is not None else None
    a.strokes, a.lengths, a.labels = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    a.S, a.seed, a.step, a.row0, a.G = corpus.S, int(seed) & _M32, int(step), int(row0), int(G)
    a.prob, a.f = float(augment_stroke_prob), float(random_scale_factor)
    a.B, a.Nmax, a.kbits = B, Nmax, feistel_bits(corpus.S)
    a.s_shuffle, a.s_scale, a.s_drop = STREAM_SHUFFLE, STREAM_SCALE, STREAM_DROP
    with torch.cuda.device(dev):
        rc = lib.lib.skr_batch_assemble(C.byref(a), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("skr_batch_assemble failed (%d)" % rc)
    return tuple(out)


def assemble(corpus: Corpus, Nmax: int, B: int, *, seed: int, step: int, row0: int = 0,
             world_rows: Optional[int] = None, random_scale_factor: float = 0.0,
             augment_stroke_prob: float = 0.0, indices=None, out=None):
    """``(strokes [B, Nmax + 1, 5] float32, lengths [B] int64, labels [B]
    int64)`` on the corpus' device: the kernel for a corpus on the GPU when the
    HIP backend is on, the host reference otherwise."""
    kw = dict(seed=seed, step=step, row0=row0, world_rows=world_rows, random_scale_factor=random_scale_factor,
              augment_stroke_prob=augment_stroke_prob, indices=indices, out=out)
    if isinstance(corpus, Corpus) and corpus.points.is_cuda:
        from . import use_hip
        if use_hip(corpus.points):
            return assemble_hip(corpus, Nmax, B, **kw)
        dev = corpus.points.device
        kw["out"] = None
        res = tuple(t.to(dev) for t in assemble_reference(corpus, Nmax, B, **kw))
        if out is not None:
            _check(corpus, Nmax, B, seed, step, row0, world_rows, random_scale_factor, augment_stroke_prob, None, out)
            for dst, src in zip(out, res):
                dst.copy_(src)
            return tuple(out)
        return res
    return assemble_reference(corpus, Nmax, B, **kw)
