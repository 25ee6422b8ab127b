"""A :class:`~.dataset.StrokeDataset` held on the device as one concatenated
corpus, with batches assembled there (:mod:`..ops.batch`).

Filtering, clipping, order, normalisation and labels are the host dataset's:
build one, ``normalize()`` it, then ``DeviceStrokeDataset.from_dataset(ds,
device)``. ``get_batch`` returns what the host dataset's returns, bit for bit.
``random_batch(step, rank, world)`` is a pure function of ``(seed, step)`` and
the global row: the ranks' batches of ``B`` rows, concatenated, are the
one-rank batch of ``B * world`` rows, and there is no RNG state to save or
restore (``state_dict()`` is empty). On ``cpu`` the NumPy reference serves,
with the same bits as the kernel.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import batch as OB
from .dataset import StrokeDataset


class DeviceStrokeDataset:
    def __init__(self, corpus: OB.Corpus, batch_size: int = 100, max_seq_length: int = 250,
                 random_scale_factor: float = 0.0, augment_stroke_prob: float = 0.0, seed: int = 0,
                 scale_factor: float = 1.0):
        if corpus.max_len > max_seq_length:
            raise ValueError("the corpus holds a sketch of %d points, more than max_seq_length = %d"
                             % (corpus.max_len, max_seq_length))
        self.corpus = corpus
        self.batch_size = batch_size
        self.max_seq_length = max_seq_length
        self.random_scale_factor = float(random_scale_factor)
        self.augment_stroke_prob = float(augment_stroke_prob)
        self.seed = int(seed)
        self.scale_factor = scale_factor
        self.num_batches = corpus.S // batch_size
        self._ranges = {}

    @classmethod
    def from_dataset(cls, ds: StrokeDataset, device="cpu", seed: Optional[int] = None) -> "DeviceStrokeDataset":
        """The host dataset as it stands (after ``normalize()``). ``seed``
        defaults to 0: the host dataset keeps RNGs, not the seed they came from."""
        corpus = OB.make_corpus(ds.strokes, ds.labels, ds.max_seq_length, device=device)
        return cls(corpus, ds.batch_size, ds.max_seq_length, ds.random_scale_factor, ds.augment_stroke_prob,
                   0 if seed is None else seed, ds.scale_factor)

    @property
    def device(self) -> torch.device:
        return self.corpus.points.device

    def __len__(self):
        return self.corpus.S

    def state_dict(self) -> dict:
        return {}

    def load_state_dict(self, sd: dict) -> None:
        pass

    def random_batch(self, step: int, rank: int = 0, world: int = 1, out=None, batch_size: Optional[int] = None):
        """Rank ``rank``'s ``B`` rows of step ``step``'s global batch of ``B *
        world`` rows: ``(strokes, lengths, labels)`` on the device, written
        into ``out`` when given. Does not synchronise."""
        b = batch_size or self.batch_size
        return OB.assemble(self.corpus, self.max_seq_length, b, seed=self.seed, step=int(step), row0=rank * b,
                           world_rows=b * world, random_scale_factor=self.random_scale_factor,
                           augment_stroke_prob=self.augment_stroke_prob, out=out)

    def get_batch(self, idx: int, out=None):
        """Sketches ``idx * B .. idx * B + B - 1`` without augmentation."""
        if not 0 <= idx < self.num_batches:
            raise IndexError("batch %d of %d" % (idx, self.num_batches))
        rng = self._ranges.get(idx)
        if rng is None:             # in range by construction: no read-back to validate it
            rng = self._ranges[idx] = torch.arange(idx * self.batch_size, (idx + 1) * self.batch_size,
                                                   dtype=torch.int64, device=self.device)
        kw = dict(seed=self.seed, step=0, indices=rng, out=out)
        if self.corpus.points.is_cuda:
            from ..ops import use_hip
            if use_hip(self.corpus.points):
                return OB.assemble_hip(self.corpus, self.max_seq_length, self.batch_size, _trusted_indices=True, **kw)
        return OB.assemble(self.corpus, self.max_seq_length, self.batch_size, **kw)
