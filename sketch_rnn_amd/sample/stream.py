"""Bulk generation: many sketches through a fixed number of decoder rows,
with finished rows refilled instead of padded.

:class:`~.sampler.GraphDecoder` runs a batch until its longest sketch ends,
so most row-steps of a batch are end-of-sketch padding on rows that finished
long ago. :class:`StreamDecoder` takes a list of J jobs (latents) and keeps
``slots`` decoder rows busy with them: when a row's sketch ends, the row gets
the next job.

Contract. ``run(z [J, Z], ...)`` returns ``(strokes [J, N, 5], lengths [J])``.
Job j is decoded with the sampler noise of (seed, local step, row
``first_row + j``) -- ``csrc/mdn_sample.h``'s ``hash_key(seed, 0x5A3D,
step)``, element ``4 * row + k`` -- so its N rows (end-of-sketch padding
included) and its length are those of row j of
``GraphDecoder(model, batch=J, steps=N).run(seed, z=z, temperature=...)``:
bit for bit when both run the same launch geometry (J and ``slots`` both
<= 128; ``gemm.plan_splits`` and the cell geometry depend on the row count
only through the number of 128-row blocks and the co-resident capacity). The
result does not depend on ``slots`` within one geometry class, on ``chunk``,
or on which slot decoded a job at which global step; jobs come out in the
order they went in; there are no atomics and two runs are bit-identical.

Two implementations (``impl``):

``"recycle"`` -- the four-launch HyperLSTM stroke (``sample/hyper_step.py``
``step_fused``; bf16, ``hyper_step_ok(model, slots)``, ``slots`` <= 128 or a
multiple of 128 up to 1024 on the wide decoder). A per-slot map in device
memory (``job[slot]``, ``pos[slot]``: the local index of the stroke the next
sampler call draws, -1 for a fresh slot) tells the sampler folded into
``csrc/decode_step.hip`` which job, local step and output row a slot works
on. One captured graph holds ``chunk`` steps followed by the refill pair of
``csrc/decode_refill.hip``, which hands finished slots (``done != 0``, the
only criterion) the next jobs by copying their constants into the in-place
state, and writes the word the host reads once per replay: jobs left + slots
still drawing. The host replays the graph until that word is zero. The
output buffer is filled with the padding row once per run, so whatever a
slot does not store is already right. The LayerNorm exchange buffers of the
clustered cells are zeroed at the top of every chunk, inside the graph: a
replay reuses its step numbers, and their tags are ``step + 1``.

The per-job constants -- condition, initial state ``[h0 | hh0]`` (bf16),
``c0``, ``hc0`` and the z projections, formed by the calls
``HyperStepDecoder.begin`` makes, over all jobs of a run at once (1024 rows
at a time beyond that) -- are held for the whole run: 4 (G + Gh) + 4 (H + Hh)
+ 2 (H + Hh) bytes per job plus the ``N x 5`` output, about 55 KB per job
on vae_large. Callers with more jobs than memory run super-batches and pass
``first_row`` on (``vae_sample --mode bulk`` does, 16384 jobs at a time).
Consequence for a split job list: ``first_row`` gives every job the noise it
has in the unsplit run, but on the GPU the constants' products (the library
GEMM of ``initial_state``, ``SmallGroup.mm`` with its row-count-dependent
split-K plan) are not row-count invariant, so a job's last bits may depend
on how many jobs its run holds, and a split run is not guaranteed to be bit
for bit the unsplit one. What is guaranteed is the match with
``GraphDecoder(batch=J)`` for the J jobs of the same run. On the CPU (blocks)
a split at a multiple of ``slots`` is bit-identical.

``"blocks"`` -- everything else (CPU, other decoders, slot counts the
stepper refuses): blocks of ``slots`` jobs through :class:`GraphDecoder`,
``run(row0=first_row + block start)`` keeping every job's noise row (a last
partial block runs at its own size). Each block pays its padding; ``row0``
is a device word of the decoder, so the blocks replay one set of graphs.

Stroke prefixes and ``fp8`` are not taken (``ValueError``).

``POISON`` (tests): the refill NaN-fills the state, z-projection and stroke
rows of every slot it leaves idle; results must not change.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .sampler import GraphDecoder, check_temperature

POISON = False
# Steps per replayed graph of the recycling path (one host read and one refill
# pair each). Measured on vae_large trained 300 steps, N = 250, temperature
# 0.5, 16 x slots jobs (profiles/r19/stream): valid strokes/s at 1024 slots
# 4.83M with 5, 4.61M with 10, 4.00M with 25; at 128 slots 2.07M / 2.09M /
# 1.85M. A longer chunk leaves finished slots idle longer (occupancy 0.69 /
# 0.65 / 0.55 at 1024 slots); a shorter one pays the refill pair more often.
CHUNK = 5


class StreamDecoder:
    def __init__(self, model, slots: int, steps: int, temperature: float = 1.0, greedy: bool = False,
                 chunk: Optional[int] = None, use_graph: bool = True, fp8: bool = False):
        if not hasattr(model, "encoder"):
            raise ValueError("StreamDecoder: needs a VAE model")
        if fp8:
            raise ValueError("StreamDecoder: fp8 is not taken in bulk generation")
        if int(slots) < 1 or int(steps) < 1:
            raise ValueError("StreamDecoder: slots and steps must be >= 1")
        if chunk is not None and int(chunk) < 1:
            raise ValueError("StreamDecoder: chunk must be >= 1")
        self.model, self.S, self.N = model, int(slots), int(steps)
        self.temp, self.greedy = float(temperature), bool(greedy)
        if not self.temp > 0:
            raise ValueError("StreamDecoder: temperature must be greater than 0 (greedy decoding is the greedy flag)")
        self.dev = next(model.parameters()).device
        self.use_graph = bool(use_graph) and self.dev.type == "cuda"
        self._chunk_arg = chunk
        self.chunk = int(chunk or CHUNK)
        self.impl = "recycle" if self._recycle_ok() else "blocks"
        self.steps_run = self.slot_steps = self.valid_strokes = 0
        self.occupancy = 0.0
        self._graph = self._sig = self._st = self._blocks = None
        self._cap = -1
        if self.impl == "recycle":
            S, dev, i32 = self.S, self.dev, torch.int32
            self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
            self.first_row = torch.zeros(1, dtype=i32, device=dev)
            self.ctl = torch.zeros(4, dtype=i32, device=dev)       # next job, jobs, the host's word
            self.done = torch.ones(S, dtype=i32, device=dev)
            self.job = torch.full((S,), -1, dtype=i32, device=dev)
            self.pos = torch.full((S,), -1, dtype=i32, device=dev)
            self.assign = torch.full((S,), -2, dtype=i32, device=dev)
            self.temps = torch.full((S,), self.temp, dtype=torch.float32, device=dev)

    def _recycle_ok(self) -> bool:
        from . import sampler
        if self.dev.type != "cuda" or not sampler.STEP_DECODER:
            return False
        from .hyper_step import fused_ok
        return fused_ok(self.model, self.S)

    # -- recycling path -------------------------------------------------------------
    def _reserve(self, J: int) -> None:
        """Per-job buffers for J jobs (grown, never shrunk; the captured graph
        holds their addresses, so growth captures again)."""
        if J <= self._cap:
            return
        st, dev, f32 = self._st, self.dev, torch.float32
        n = max(J, 1)
        self.out = torch.empty(n, self.N, 5, dtype=f32, device=dev)
        self.jA = torch.empty(n, st.K, dtype=torch.bfloat16, device=dev)
        self.jCC = torch.empty(n, st.H, dtype=f32, device=dev)
        self.jHCC = torch.empty(n, st.Hh, dtype=f32, device=dev)
        self.jZP = torch.empty(n, st.G + st.Gh, dtype=f32, device=dev)
        self.jtemps = torch.empty(n, dtype=f32, device=dev)
        self._cap, self._graph = n, None

    @torch.no_grad()
    def _constants(self, z, labels, J: int) -> None:
        from ..ops import gemm
        model, st = self.model, self._st
        cfg, p = model.cfg, model.dec
        H, G = st.H, st.G
        IN = p.W_x.shape[0]
        for j0 in range(0, J, 1024):
            n = min(1024, J - j0)
            lab = labels[j0:j0 + n] if (labels is not None and cfg.num_classes > 0) else None
            if lab is None and cfg.num_classes > 0:
                lab = torch.zeros(n, dtype=torch.int64, device=self.dev)
            zc = model.condition(z[j0:j0 + n] if cfg.conditional else None, lab, n, self.dev)
            h0, c0, hh0, hc0 = model.initial_state(zc, n, self.dev)
            self.jA[j0:j0 + n, :H].copy_(h0)
            self.jA[j0:j0 + n, H:].copy_(hh0)
            self.jCC[j0:j0 + n].copy_(c0)
            self.jHCC[j0:j0 + n].copy_(hc0)
            if zc is not None:
                g = gemm.SmallGroup(self.dev)
                g.mm(zc.float().contiguous(), p.W_x[5:].detach(), out=self.jZP[j0:j0 + n, :G])
                g.mm(zc.float().contiguous(), p.hyp_W_x[5:IN].detach(), out=self.jZP[j0:j0 + n, G:])
                g.run()
            else:
                self.jZP[j0:j0 + n].zero_()

    def _refill(self) -> None:
        from ..ops._hipapi import RefillArgs
        st = self._st
        r = RefillArgs()
        r.slots, r.chunk, r.poison = self.S, self.chunk, int(bool(POISON))
        r.ctl, r.done, r.job, r.pos, r.assign = (t.data_ptr() for t in (self.ctl, self.done, self.job, self.pos,
                                                                         self.assign))
        r.A, r.jA, r.a_bytes = st.A.data_ptr(), self.jA.data_ptr(), 2 * st.K
        r.CC, r.jCC, r.cc_bytes = st.CC.data_ptr(), self.jCC.data_ptr(), 4 * st.H
        r.HCC, r.jHCC, r.hcc_bytes = st.HCC.data_ptr(), self.jHCC.data_ptr(), 4 * st.Hh
        r.ZP, r.jZP, r.zp_bytes = st.ZP.data_ptr(), self.jZP.data_ptr(), 4 * (st.G + st.Gh)
        r.temps, r.jtemps, r.X = self.temps.data_ptr(), self.jtemps.data_ptr(), st.X.data_ptr()
        rc = st.lib.skr_decode_refill(ctypes.byref(r), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError("skr_decode_refill failed (%d)" % rc)

    @torch.no_grad()
    def _chunk_steps(self) -> None:
        """``chunk`` strokes of every slot with the slot-map sampler, then the
        refill pair: the body of the replayed graph."""
        st = self._st
        for cl in (st.clm, st.clh):        # a replay reuses its step numbers: stale partials carry valid tags
            if cl.on:
                cl.part.zero_()
        for tt in range(self.chunk):
            smp = st.sample_args(tt, 0, self.out, self.done, self.seed, st.M, 1, self.temp, self.greedy, False,
                                 temps=self.temps)
            smp.job, smp.pos, smp.first_row = self.job.data_ptr(), self.pos.data_ptr(), self.first_row.data_ptr()
            smp.nsteps = self.N
            st.step_fused(tt, smp)
        self._refill()

    @torch.no_grad()
    def _run_recycle(self, z, labels, temps, seed: int, first_row: int, J: int):
        from ..ops import gemm
        from ..train.graph import capture
        if self._st is None:
            from .hyper_step import HyperStepDecoder
            self._st = HyperStepDecoder(self.model, self.S, self.dev)
            assert self._st.fused and not self._st.fp8
        st = self._st
        self._reserve(J)
        st.prepare()
        sig = (gemm.WEIGHTS_EPOCH[0], bool(POISON), bool(self.use_graph)) + tuple(
            p._version for p in self.model.parameters())
        if sig != self._sig:
            self._graph = None
        self._sig = sig
        self.seed.fill_(int(seed))
        self.first_row.fill_(int(first_row))
        # every slot finished and no jobs: a chunk run in this state (warm-up) stores nothing
        self.done.fill_(1)
        self.pos.fill_(-1)
        self.job.fill_(-1)
        self.ctl.zero_()
        if self.use_graph and self._graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._chunk_steps()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with capture(g):
                self._chunk_steps()
            self._graph = g
            self.pos.fill_(-1)
        if J > 0:
            self._constants(z, labels, J)
            self.jtemps[:J].copy_(temps)
            self.out[:J].zero_()
            self.out[:J, :, 4] = 1.0
        self.ctl.copy_(torch.tensor([0, J, 0, 0], dtype=torch.int32))
        self._refill()                     # the first fill: every slot is marked finished
        ran = 0
        # each job occupies a slot for at most ceil((N + 1) / chunk) + 1 chunks
        limit = (-(-J // self.S) + 1) * (-(-(self.N + 1) // self.chunk) + 1)
        while int(self.ctl[2]) != 0:       # one host read per chunk: jobs left + slots still drawing
            if ran >= limit * self.chunk:
                raise RuntimeError("StreamDecoder: the refill loop did not finish in %d chunks" % limit)
            if self.use_graph:
                self._graph.replay()
            else:
                self._chunk_steps()
            ran += self.chunk
        return self.out[:J].clone(), ran

    # -- blocks of `slots` jobs through GraphDecoder ------------------------------------
    def _block_decoder(self, n: int) -> GraphDecoder:
        if self._blocks is None:
            self._blocks = {}
        if n not in self._blocks:
            self._blocks[n] = GraphDecoder(self.model, n, self.N, self.temp, self.greedy, use_graph=self.use_graph,
                                           chunk=self._chunk_arg)
        return self._blocks[n]

    @torch.no_grad()
    def _run_blocks(self, z, labels, temps, seed: int, first_row: int, J: int):
        S, N, dev = self.S, self.N, self.dev
        cfg = self.model.cfg
        out = torch.zeros(J, N, 5, device=dev)
        ran = 0
        for j0 in range(0, J, S):
            n = min(S, J - j0)       # (a last partial block runs at its own size: no padded rows)
            dec = self._block_decoder(n)
            zb = z[j0:j0 + n] if cfg.conditional else None
            lb = labels[j0:j0 + n] if labels is not None else torch.zeros(n, dtype=torch.int64, device=dev)
            s, _ = dec.run(seed=seed, z=zb, labels=lb, temperature=temps[j0:j0 + n], row0=first_row + j0)
            out[j0:j0 + n] = s
            ran += dec.steps_run
        return out, ran

    @torch.no_grad()
    def run(self, z: torch.Tensor, labels: Optional[torch.Tensor] = None, temperature=None, seed: int = 0,
            first_row: int = 0, prefix=None, prefix_len=None):
        """``z [J, Z]`` (any J >= 0; an unconditional model reads only J from
        it) -> ``(strokes [J, N, 5], lengths [J])``. ``temperature``: a float
        or a ``[J]`` vector, None for the constructor's value. ``first_row``:
        the noise row of job 0 (a caller splitting a long job list into
        several runs passes the number of jobs before this run)."""
        if prefix is not None or prefix_len is not None:
            raise ValueError("StreamDecoder.run: stroke prefixes are not taken in bulk generation")
        cfg = self.model.cfg
        z = torch.as_tensor(z)
        if z.dim() != 2 or (cfg.conditional and z.shape[1] != cfg.z_size):
            raise ValueError("StreamDecoder.run: z must be [J, %d]" % cfg.z_size)
        J = z.shape[0]
        z = z.to(self.dev, torch.float32)
        if labels is not None:
            labels = torch.as_tensor(labels).to(self.dev, torch.int64)
            if labels.shape != (J,):
                raise ValueError("StreamDecoder.run: labels must be [J]")
        if int(first_row) < 0 or int(first_row) + J >= 2 ** 30:
            raise ValueError("StreamDecoder.run: first_row must be >= 0 and first_row + J below 2^30")
        temps = check_temperature("StreamDecoder.run", self.temp if temperature is None else temperature, J, self.dev)
        fn = self._run_recycle if self.impl == "recycle" else self._run_blocks
        strokes, ran = fn(z, labels, temps, int(seed), int(first_row), J)
        hits = strokes[:, :, 4] > 0
        lengths = torch.where(hits.any(1), hits.float().argmax(1) + 1,
                              torch.full((J,), self.N, dtype=torch.long, device=self.dev))
        self.steps_run = int(ran)
        self.slot_steps = self.S * self.steps_run
        self.valid_strokes = int(lengths.sum()) if J > 0 else 0
        self.occupancy = self.valid_strokes / self.slot_steps if self.slot_steps else 0.0
        return strokes, lengths

    def counters(self) -> dict:
        return {"steps_run": self.steps_run, "slot_steps": self.slot_steps, "valid_strokes": self.valid_strokes,
                "occupancy": self.occupancy}
