"""Fused whole-sketch decoders: the reference model (``csrc/decode_ref.hip``)
and the VAE's plain and LayerNorm LSTM decoders (``csrc/decode_vae.hip``,
``csrc/decode_vae_ln.hip``).

The reference samples one stroke per ``sess.run`` (``model.py:187-264``:
two host transfers per stroke, ~486 strokes/s here). :class:`GraphDecoder`
removes the host from the loop but still replays a chain of kernels per
stroke (step GEMMs, cells, head, sampler). :class:`FusedRefDecoder` runs
the whole decode -- both LSTM layers, the MDN head and the sampler, every
step -- as ONE kernel launch per batch: weights stay in LDS, the cell state
in registers, and strokes travel between the workgroups through in-launch
hand-offs.

Semantics are those of ``GraphDecoder`` in reference mode (identical hash
random numbers, the reference's pen-temperature bug unless
``fix_pen_temperature``, per-step eoc state hold, end-of-sketch padding of
finished rows), with bf16 MFMA operands and fp32 state. Eligible models:
``lstm`` cells, ``rnn_size`` 256, 1 or 2 layers, at most 32 mixtures
(:func:`fused_decode_ok`); anything else keeps using ``GraphDecoder``.

:class:`FusedVAEDecoder` does the same for a :class:`SketchVAE` whose decoder
is a plain ``lstm`` of size 256 (up to 32 mixtures) or 512 (up to 20)
(:func:`fused_vae_ok`): one launch per chunk of steps and rows, with the
latent's input projection folded into a per-row bias, an all-done exit
between chunks, and per-row stroke prefixes (sketch completion).
:class:`FusedLNVAEDecoder` (``csrc/decode_vae_ln.hip``) is the same decoder
for ``layer_norm`` decoders of those sizes (:func:`fused_vae_ln_ok`): the
row statistics of the two layer norms span all workgroups of a row block, so
each step exchanges per-row partial sums between them inside the launch.
:func:`fused_vae_decoder` returns the class that takes a model. ``hyper``
decoders stay on ``GraphDecoder``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from ..utils import native

_H = 256
_FLAG_STRIDE = 64
_LN_FLAG_STRIDE = 128      # csrc/decode_vae_ln.hip kLnFlagStride: h | head | gate statistics | cell statistics
_XLD = 8

# Debug knob of FusedLNVAEDecoder: NaN-fill every in-launch hand-off buffer
# (statistics slots, hbuf[1:], the rows of xin[1:] no prefix supplies) before
# each run. Results must not change.
LN_DECODE_POISON = False


def fused_decode_ok(model) -> bool:
    cfg = model.cfg
    return (getattr(cfg, "kind", "") == "reference" and cfg.model == "lstm" and cfg.rnn_size == _H
            and cfg.num_layers in (1, 2) and 1 <= cfg.num_mixture <= 32)


class NotCoResident(RuntimeError):
    """The launch's workgroups cannot all be resident at once on this device
    (``skr_decode_ref`` returned -8); callers fall back to ``GraphDecoder``."""


def fused_vae_ok(model) -> bool:
    """A :class:`SketchVAE` with a plain ``lstm`` decoder that
    ``csrc/decode_vae.hip`` takes: ``dec_rnn_size`` 256 with at most 32
    mixtures, or 512 with at most 20 (the head's weights must fit in LDS).
    Conditional, unconditional and class-conditional models all qualify."""
    from ..models.vae import SketchVAE
    if not isinstance(model, SketchVAE) or model.cfg.dec_model != "lstm":
        return False
    H, M = model.cfg.dec_rnn_size, model.cfg.num_mixture
    return (H == 256 and 1 <= M <= 32) or (H == 512 and 1 <= M <= 20)


def fused_vae_ln_ok(model) -> bool:
    """A :class:`SketchVAE` with a ``layer_norm`` decoder that
    ``csrc/decode_vae_ln.hip`` takes: the sizes and mixture counts of
    :func:`fused_vae_ok`."""
    from ..models.vae import SketchVAE
    if not isinstance(model, SketchVAE) or model.cfg.dec_model != "layer_norm":
        return False
    H, M = model.cfg.dec_rnn_size, model.cfg.num_mixture
    return (H == 256 and 1 <= M <= 32) or (H == 512 and 1 <= M <= 20)


def fused_vae_kind(model) -> Optional[str]:
    """``"lstm"`` / ``"layer_norm"``: which whole-sketch kernel decodes
    ``model`` (:func:`fused_vae_decoder`); None if neither does."""
    if fused_vae_ok(model):
        return "lstm"
    if fused_vae_ln_ok(model):
        return "layer_norm"
    return None


def _chunk_rows(L: int, mtw: int, cus: int = 256, H: int = _H) -> int:
    """Rows one launch can take: every workgroup must be co-resident (one
    ~100 KB-LDS workgroup per CU, ``cus`` CUs -- 256 on MI355X; L*(H/16) + 1
    workgroups per row block)."""
    return (cus // (L * (H // 16) + 1)) * 16 * mtw


class FusedRefDecoder:
    """B sketches of N strokes from a reference :class:`SketchRNN` in one launch
    per chunk of rows. ``run()`` returns ``(strokes [B, N, 5], lengths [B])``
    like :meth:`GraphDecoder.run` (offsets multiplied by ``data_scale``)."""

    def __init__(self, model, batch: int, steps: int, temperature: float = 1.0, greedy: bool = False,
                 fix_pen_temperature: bool = False):
        if not fused_decode_ok(model):
            raise ValueError("FusedRefDecoder: needs a reference lstm model with rnn_size 256, 1-2 layers, M <= 32")
        self.lib = native.require_hip()
        self.model = model
        self.B, self.N = int(batch), int(steps)
        self.temp, self.greedy, self.fix_pen = float(temperature), bool(greedy), bool(fix_pen_temperature)
        cfg = model.cfg
        self.L, self.M = cfg.num_layers, cfg.num_mixture
        self.nout = 3 + 6 * self.M
        self.noutp = -(-self.nout // 16) * 16
        self.dev = next(model.parameters()).device
        self.mtw = 1 if self.B <= 16 else 2
        cus = torch.cuda.get_device_properties(self.dev).multi_processor_count if self.dev.type == "cuda" else 256
        self.rows = _chunk_rows(self.L, self.mtw, cus)
        if self.rows <= 0:
            raise NotCoResident("FusedRefDecoder: %d CUs cannot hold one row block (%d workgroups)"
                                % (cus, self.L * (_H // 16) + 1))
        self.seed = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._w = None
        self._sig = None

    # -- weights (bf16 operands, refreshed when the parameters change) -------------------
    @torch.no_grad()
    def _weights(self):
        sig = tuple(p._version for p in self.model.parameters()) + tuple(p.data_ptr() for p in self.model.parameters())
        if self._w is not None and sig == self._sig:
            return self._w
        m, bf = self.model, torch.bfloat16
        p0 = m.layers[0]
        w = {
            "WT0": p0.W_h.detach().t().to(bf).contiguous(),                      # [4H, H]
            "Wx0": p0.W_x.detach().float().contiguous(),                         # [5, 4H]
            "b0": p0.bias.detach().float().contiguous(),
            "bo": m.output_b.detach().float().contiguous(),
        }
        if self.L == 2:
            p1 = m.layers[1]
            w["WT1"] = torch.cat([p1.W_x.detach(), p1.W_h.detach()], 0).t().to(bf).contiguous()   # [4H, 2H]
            w["b1"] = p1.bias.detach().float().contiguous()
        WoT = torch.zeros(self.noutp, _H, dtype=bf, device=self.dev)
        WoT[: self.nout] = m.output_w.detach().t().to(bf)
        w["WoT"] = WoT
        self._w, self._sig = w, sig
        return w

    def _launch(self, r0: int, Bc: int, xin: torch.Tensor, forced: bool, zout: Optional[torch.Tensor],
                temps: Optional[torch.Tensor] = None):
        from ..ops._hipapi import DecArgs
        from ..ops.recurrent import cluster_error_flag
        w = self._weights()
        N, L, dev, bf, f32 = self.N, self.L, self.dev, torch.bfloat16, torch.float32
        RB = 16 * self.mtw
        nrb = -(-Bc // RB)
        a = DecArgs()
        a.N, a.B, a.L, a.H, a.mtw, a.nrb = N, Bc, L, _H, self.mtw, nrb
        a.M, a.nout, a.noutp, a.mode = self.M, self.nout, self.noutp, 0
        a.greedy, a.fix_pen, a.forced, a.row0 = int(self.greedy), int(self.fix_pen), int(forced), int(r0)
        a.temp, a.forget_bias = self.temp, 1.0
        keep = []
        for l in range(L):
            ly = a.ly[l]
            z = torch.zeros(Bc, _H, dtype=f32, device=dev)          # reference sampling starts from the zero state
            hbuf = torch.empty(N + 1, Bc, _H, dtype=bf, device=dev)
            hbuf[0].zero_()
            hup = torch.empty(N, Bc, _H, dtype=bf, device=dev)
            ly.WT = w["WT0" if l == 0 else "WT1"].data_ptr()
            ly.bias = w["b0" if l == 0 else "b1"].data_ptr()
            ly.h0, ly.c0, ly.hbuf, ly.hup = z.data_ptr(), z.data_ptr(), hbuf.data_ptr(), hup.data_ptr()
            ly.hT = ly.cT = None
            keep += [z, hbuf, hup]
        out = torch.empty(Bc, N, 5, dtype=f32, device=dev)
        done = torch.zeros(Bc, dtype=torch.int32, device=dev)
        flags = torch.empty(nrb * _FLAG_STRIDE, dtype=torch.int32, device=dev)   # zeroed by the launcher
        a.Wx0, a.WoT, a.bo = w["Wx0"].data_ptr(), w["WoT"].data_ptr(), w["bo"].data_ptr()
        a.xin, a.out, a.done = xin.data_ptr(), out.data_ptr(), done.data_ptr()
        a.zout = zout.data_ptr() if zout is not None else None
        a.temps = temps[r0:].data_ptr() if temps is not None else None    # indexed by the launch's local row
        a.seed, a.flags, a.err = self.seed.data_ptr(), flags.data_ptr(), cluster_error_flag(dev).data_ptr()
        rc = self.lib.lib.skr_decode_ref(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc == -8:
            raise NotCoResident("skr_decode_ref: workgroups cannot be co-resident on this device (code -8)")
        if rc != 0:
            raise RuntimeError("skr_decode_ref: launch failed (code %d)" % rc)
        keep += [flags, done]
        return out, keep

    @torch.no_grad()
    def run(self, seed: int = 0, return_z: bool = False, temperature=None):
        """Returns ``(strokes, lengths)`` (plus the head outputs ``z [N, B, 3+6M]``
        with ``return_z``). ``temperature``: a float or a vector of B per-row
        values for this run (None: the constructor's)."""
        from ..ops.recurrent import check_cluster_errors
        from .sampler import check_temperature
        temps = (torch.full((self.B,), self.temp, dtype=torch.float32, device=self.dev) if temperature is None
                 else check_temperature("FusedRefDecoder.run", temperature, self.B, self.dev))
        self.seed.fill_(int(seed))
        outs, zs, keep = [], [], []
        for r0 in range(0, self.B, self.rows):
            Bc = min(self.rows, self.B - r0)
            xin = torch.zeros(self.N + 1, Bc, _XLD, device=self.dev)        # x(0) = 0 (model.py:200)
            zout = torch.empty(self.N, Bc, self.nout, device=self.dev) if return_z else None
            o, k = self._launch(r0, Bc, xin, False, zout, temps)
            outs.append(o)
            zs.append(zout)
            keep += k + [xin, temps]
        strokes = torch.cat(outs, 0)
        check_cluster_errors(self.dev)
        hits = strokes[:, :, 3] > 0
        lengths = torch.where(hits.any(1), hits.float().argmax(1) + 1,
                              torch.full_like(hits[:, 0], self.N, dtype=torch.long))
        strokes[:, :, 0:2] *= self.model.cfg.data_scale
        if return_z:
            return strokes, lengths, torch.cat(zs, 1)
        return strokes, lengths

    @torch.no_grad()
    def forced(self, xs: torch.Tensor) -> torch.Tensor:
        """Teacher-forced decode: ``xs [N, B, 5]`` fed inputs -> head outputs
        ``z [N, B, 3+6M]`` (the kernel's numerics against the step oracle)."""
        from ..ops.recurrent import check_cluster_errors
        N, B = xs.shape[0], xs.shape[1]
        assert N == self.N and B == self.B
        zs, keep = [], []
        for r0 in range(0, B, self.rows):
            Bc = min(self.rows, B - r0)
            xin = torch.zeros(N + 1, Bc, _XLD, device=self.dev)
            xin[:N, :, :5] = xs[:, r0:r0 + Bc].to(self.dev, torch.float32)
            zout = torch.empty(N, Bc, self.nout, device=self.dev)
            _, k = self._launch(r0, Bc, xin, True, zout)
            zs.append(zout)
            keep += k + [xin]
        z = torch.cat(zs, 1)
        check_cluster_errors(self.dev)
        return z


class _FusedVAEBase:
    """Host side of the whole-sketch VAE decoders: the latent, the buffers,
    the chunked launch loop with the all-done exit, prefixes. A subclass
    names its kernel: ``_eligible`` / ``_NEEDS``, ``_cell_weights``, ``_row_term``
    (the per-row fp32 gate term), ``_FLAGS`` (flag words per row block),
    ``_extra`` (per-launch-chunk buffers of its own) and ``_launch``."""

    _NEEDS = ""
    _FLAGS = _FLAG_STRIDE

    @staticmethod
    def _eligible(model) -> bool:
        raise NotImplementedError

    def __init__(self, model, batch: int, steps: int, temperature: float = 1.0, greedy: bool = False,
                 chunk: int = 50, early_exit: bool = True):
        self._name = type(self).__name__
        if not self._eligible(model):
            raise ValueError("%s: needs a SketchVAE with %s decoder of size 256 (M <= 32) or 512 (M <= 20)"
                             % (self._name, self._NEEDS))
        self.lib = native.require_hip()
        self.model = model
        self.B, self.N = int(batch), int(steps)
        self.temp, self.greedy = float(temperature), bool(greedy)
        cfg = model.cfg
        self.H, self.M = cfg.dec_rnn_size, cfg.num_mixture
        self.nout = 3 + 6 * self.M
        self.noutp = -(-self.nout // 16) * 16
        self.dev = next(model.parameters()).device
        cus = torch.cuda.get_device_properties(self.dev).multi_processor_count if self.dev.type == "cuda" else 256
        self.rows = _chunk_rows(1, 1 if self.B <= 16 else 2, cus, self.H)
        if self.rows <= 0:
            raise NotCoResident("%s: %d CUs cannot hold one row block (%d workgroups)"
                                % (self._name, cus, self.H // 16 + 1))
        c = max(int(chunk), 1)
        self.ranges = [(t, min(t + c, self.N)) for t in range(0, self.N, c)]
        self.early_exit = bool(early_exit)
        self.steps_run = 0
        self.seed = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._w = None
        self._sig = None

    # -- weights (bf16 operands, refreshed when the parameters change) -------------------
    @torch.no_grad()
    def _weights(self):
        sig = tuple(p._version for p in self.model.parameters()) + tuple(p.data_ptr() for p in self.model.parameters())
        if self._w is not None and sig == self._sig:
            return self._w
        m, bf, p = self.model, torch.bfloat16, self.model.dec
        WoT = torch.zeros(self.noutp, self.H, dtype=bf, device=self.dev)
        WoT[: self.nout] = m.output_w.detach().t().to(bf)
        Wx = p.W_x.detach().float()
        self._w = {
            "WT": p.W_h.detach().t().to(bf).contiguous(),            # [4H, H]
            "Wx": Wx[:5].contiguous(),                               # [5, 4H] stroke rows
            "Wz": Wx[5:].contiguous(),                               # [z_in, 4H] rows of the conditioning
            "WoT": WoT,
            "bo": m.output_b.detach().float().contiguous(),
        }
        self._w.update(self._cell_weights(p))
        self._sig = sig
        return self._w

    def _latent(self, seed: int, z, labels):
        """``(zc, (h0, c0))`` as ``GraphDecoder`` conditions a run."""
        cfg, B, dev = self.model.cfg, self.B, self.dev
        if cfg.conditional:
            if z is None:
                g = torch.Generator(device=dev).manual_seed(int(seed))
                z = torch.randn((B, max(cfg.z_size, 1)), device=dev, generator=g)
            z = z.to(dev, torch.float32)
        lab = None
        if cfg.num_classes > 0:
            lab = torch.zeros(B, dtype=torch.int64, device=dev) if labels is None else labels.to(dev, torch.int64)
        zc = self.model.condition(z if cfg.conditional else None, lab, B, dev)
        return zc, self.model.initial_state(zc, B, dev)

    def _begin(self, seed: int, z, labels, xin: torch.Tensor, nforced: Optional[torch.Tensor], want_z: bool,
               temps: Optional[torch.Tensor] = None):
        """Buffers of one decode: whole-batch ones the launches index by row
        slice, and per-launch-chunk ones laid out ``[step][row of the chunk]``."""
        w = self._weights()
        B, N, H, dev, f32 = self.B, self.N, self.H, self.dev, torch.float32
        zc, (h0, c0) = self._latent(seed, z, labels)
        st = {
            "zb": self._row_term(zc, w).contiguous(), "c": c0.to(f32).contiguous().clone(),
            "out": torch.empty(B, N, 5, dtype=f32, device=dev),
            "done": torch.zeros(B, dtype=torch.int32, device=dev),
            "nforced": nforced.to(dev, torch.int32).contiguous() if nforced is not None else None,
            "temps": temps,
            "chunks": [],
        }
        h0 = h0.to(torch.bfloat16)
        for r0 in range(0, B, self.rows):
            Bc = min(self.rows, B - r0)
            mtw = 1 if Bc <= 16 else 2
            nrb = -(-Bc // (16 * mtw))
            hbuf = torch.empty(N + 1, Bc, H, dtype=torch.bfloat16, device=dev)
            hbuf[0] = h0[r0:r0 + Bc]
            if self._poison():
                hbuf[1:] = float("nan")
            ch = self._extra(nrb, mtw)
            ch.update({
                "r0": r0, "Bc": Bc, "mtw": mtw, "nrb": nrb, "hbuf": hbuf,
                "xin": xin[:, r0:r0 + Bc].contiguous(),
                "zout": torch.zeros(N, Bc, self.nout, dtype=f32, device=dev) if want_z else None,
                "flags": torch.empty(nrb * self._FLAGS, dtype=torch.int32, device=dev),   # zeroed by the launcher
            })
            st["chunks"].append(ch)
        return st

    # -- what a subclass supplies ---------------------------------------------------------
    def _cell_weights(self, p) -> dict:
        """fp32 parameters of the cell beyond W_x / W_h (bias or layer norms)."""
        raise NotImplementedError

    def _row_term(self, zc, w) -> torch.Tensor:
        """``[B, 4H]`` fp32 term the kernel adds to every step's gates of a row."""
        raise NotImplementedError

    def _poison(self) -> bool:
        return False

    def _extra(self, nrb: int, mtw: int) -> dict:
        return {}

    def _fill_common(self, a, st, ch, t0: int, t1: int):
        """The fields both kernels' argument structs name alike."""
        from ..ops.recurrent import cluster_error_flag
        w = self._weights()
        r0, Bc = ch["r0"], ch["Bc"]
        a.N, a.B, a.H, a.mtw, a.nrb = self.N, Bc, self.H, ch["mtw"], ch["nrb"]
        a.M, a.nout, a.noutp, a.greedy, a.row0 = self.M, self.nout, self.noutp, int(self.greedy), int(r0)
        a.t0, a.t1, a.temp, a.forget_bias = int(t0), int(t1), self.temp, 1.0
        a.WT, a.Wx, a.WoT, a.bo = w["WT"].data_ptr(), w["Wx"].data_ptr(), w["WoT"].data_ptr(), w["bo"].data_ptr()
        a.c0 = a.cT = st["c"][r0:].data_ptr()
        a.hbuf, a.xin = ch["hbuf"].data_ptr(), ch["xin"].data_ptr()
        a.out, a.done = st["out"][r0:].data_ptr(), st["done"][r0:].data_ptr()
        a.nforced = st["nforced"][r0:].data_ptr() if st["nforced"] is not None else None
        a.temps = st["temps"][r0:].data_ptr() if st["temps"] is not None else None
        a.zout = ch["zout"].data_ptr() if ch["zout"] is not None else None
        a.seed, a.flags = self.seed.data_ptr(), ch["flags"].data_ptr()
        a.err = cluster_error_flag(self.dev).data_ptr()
        return w

    def _call(self, fn, name: str, a):
        rc = fn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc == -8:
            raise NotCoResident("%s: workgroups cannot be co-resident on this device (code -8)" % name)
        if rc != 0:
            raise RuntimeError("%s: launch failed (code %d)" % (name, rc))

    def _launch(self, st, ch, t0: int, t1: int):
        raise NotImplementedError

    @torch.no_grad()
    def run(self, seed: int = 0, z: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
            prefix: Optional[torch.Tensor] = None, prefix_len: Optional[torch.Tensor] = None,
            return_z: bool = False, temperature=None):
        """Returns ``(strokes [B, N, 5], lengths [B])`` like
        :meth:`GraphDecoder.run` (plus the head outputs ``z [N, B, 3+6M]`` with
        ``return_z``; steps an early exit skipped are zero there).

        ``prefix [B, P, 5]`` with ``prefix_len [B]`` (default P for every row)
        completes sketches: the first ``prefix_len[b]`` strokes of row b are
        the prefix's and the decoder continues from them.

        ``temperature``: a float or a vector of B per-row values for this run
        (None: the constructor's); each launch reads its rows' slice."""
        from ..ops.recurrent import check_cluster_errors
        from .sampler import check_temperature
        B, N, dev = self.B, self.N, self.dev
        temps = (torch.full((B,), self.temp, dtype=torch.float32, device=dev) if temperature is None
                 else check_temperature(self._name + ".run", temperature, B, dev))
        self.seed.fill_(int(seed))
        xin = torch.zeros(N + 1, B, _XLD, device=dev)
        xin[0, :, 2] = 1.0                                          # start token
        nforced = None
        if prefix is not None:
            from .sampler import check_prefix
            prefix, plen = check_prefix(self._name + ".run", prefix, prefix_len, B, N, dev)
            P = prefix.shape[1]
            inside = torch.arange(P, device=dev)[None, :] < plen[:, None]
            Pn = min(P, N)
            xin[1:Pn + 1, :, :5] = (prefix[:, :Pn] * inside[:, :Pn, None]).transpose(0, 1)
            nforced = plen
        if self._poison():            # rows of xin[1:] no prefix supplies: the head must write them first
            free = torch.ones(N, B, dtype=torch.bool, device=dev)
            if nforced is not None:
                free = torch.arange(1, N + 1, device=dev)[:, None] > nforced[None, :]
            xin[1:][free] = float("nan")
        st = self._begin(seed, z, labels, xin, nforced, return_z, temps)
        ran = N
        for t0, t1 in self.ranges:
            for ch in st["chunks"]:
                self._launch(st, ch, t0, t1)
            ran = t1
            if self.early_exit and t1 < N and bool(st["done"].all()):   # one host read per chunk of steps
                break
        strokes = st["out"]
        if ran < N:            # strokes the skipped launches would have drawn: all padding
            strokes[:, ran:] = 0.0
            strokes[:, ran:, 4] = 1.0
        self.steps_run = ran
        check_cluster_errors(dev)
        hits = strokes[:, :, 4] > 0
        lengths = torch.where(hits.any(1), hits.float().argmax(1) + 1,
                              torch.full_like(hits[:, 0], N, dtype=torch.long))
        if return_z:
            return strokes, lengths, torch.cat([ch["zout"] for ch in st["chunks"]], 1)
        return strokes, lengths

    @torch.no_grad()
    def forced(self, xs: torch.Tensor, z: Optional[torch.Tensor] = None,
               labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Teacher-forced decode: ``xs [N, B, 5]`` fed inputs (``xs[0]`` the
        start token) -> head outputs ``z [N, B, 3+6M]`` (the kernel's numerics
        against the step oracle). ``z`` None on a conditional model draws the
        latent as ``run(seed=0)`` does."""
        from ..ops.recurrent import check_cluster_errors
        N, B = xs.shape[0], xs.shape[1]
        assert N == self.N and B == self.B
        self.seed.fill_(0)
        xin = torch.zeros(N + 1, B, _XLD, device=self.dev)
        xin[:N, :, :5] = xs.to(self.dev, torch.float32)
        st = self._begin(0, z, labels, xin, torch.full((B,), N, dtype=torch.int32, device=self.dev), True)
        for ch in st["chunks"]:
            self._launch(st, ch, 0, N)
        check_cluster_errors(self.dev)
        return torch.cat([ch["zout"] for ch in st["chunks"]], 1)


class FusedVAEDecoder(_FusedVAEBase):
    """B sketches of N strokes from a :class:`SketchVAE` with a plain ``lstm``
    decoder (``csrc/decode_vae.hip``): the LSTM layer, the MDN head and the
    sampler of every step of ``chunk`` steps in one launch per chunk of rows.

    Semantics are those of ``GraphDecoder`` in VAE mode (start token
    ``[0, 0, 1, 0, 0]``, identical hash random numbers, temperature on
    mixture, pen and sigma, end-of-sketch padding of finished rows), with
    bf16 MFMA operands and fp32 state. After each chunk of steps the host
    reads whether every row has ended; if so the remaining chunks are not
    launched and their strokes are filled with padding (``steps_run`` records
    the steps executed). Chunking does not change a single bit of the result.
    ``layer_norm`` decoders are :class:`FusedLNVAEDecoder`'s
    (:func:`fused_vae_decoder` picks); ``hyper`` decoders are not eligible
    and keep using ``GraphDecoder``.
    """

    _NEEDS = "an lstm"
    _eligible = staticmethod(fused_vae_ok)

    def _cell_weights(self, p):
        return {"b": p.bias.detach().float().contiguous()}

    def _row_term(self, zc, w):
        """``zb [B, 4H] = zc @ W_x[5:] + bias``."""
        if zc is None:
            return w["b"].expand(self.B, 4 * self.H)
        return zc.to(torch.float32) @ w["Wz"] + w["b"]

    def _launch(self, st, ch, t0: int, t1: int):
        from ..ops._hipapi import DecVaeArgs
        a = DecVaeArgs()
        self._fill_common(a, st, ch, t0, t1)
        a.zb = st["zb"][ch["r0"]:].data_ptr()
        self._call(self.lib.lib.skr_decode_vae, "skr_decode_vae", a)


class FusedLNVAEDecoder(_FusedVAEBase):
    """:class:`FusedVAEDecoder` for a ``layer_norm`` decoder
    (``csrc/decode_vae_ln.hip``): same surface, same semantics, same host
    loop. Per step the ``H/16`` layer workgroups of a row block exchange the
    per-row partial statistics of the two layer norms (gates, then the new
    cell) inside the launch; :func:`ln_decode_step_transcription` is the
    kernel's arithmetic in PyTorch. With the module attribute
    ``LN_DECODE_POISON`` set, every buffer workgroups hand to each other inside
    a launch (statistics slots, ``hbuf[1:]``, the rows of ``xin[1:]`` no
    prefix supplies) is NaN-filled before each run, so a read that precedes
    its write shows in the output."""

    _NEEDS = "a layer_norm"
    _FLAGS = _LN_FLAG_STRIDE
    _eligible = staticmethod(fused_vae_ln_ok)

    def _cell_weights(self, p):
        return {k: getattr(p, k).detach().float().contiguous()
                for k in ("ln_gamma", "ln_beta", "lnc_gamma", "lnc_beta")}

    def _row_term(self, zc, w):
        """``zp [B, 4H] = zc @ W_x[5:]`` (LNLSTMParams has no bias)."""
        if zc is None:
            return torch.zeros(self.B, 4 * self.H, device=self.dev)
        return zc.to(torch.float32) @ w["Wz"]

    def _poison(self) -> bool:
        return bool(LN_DECODE_POISON)

    def _extra(self, nrb: int, mtw: int) -> dict:
        # [parity][row block][workgroup][row][gate][mean, M2] and [...][row][mean, M2]
        n = 2 * nrb * (self.H // 16) * 16 * mtw
        fill = float("nan") if self._poison() else 0.0
        return {"gstat": torch.full((n * 8,), fill, device=self.dev),
                "cstat": torch.full((n * 2,), fill, device=self.dev)}

    def _launch(self, st, ch, t0: int, t1: int):
        from ..ops._hipapi import DecVaeLnArgs
        a = DecVaeLnArgs()
        w = self._fill_common(a, st, ch, t0, t1)
        a.zp = st["zb"][ch["r0"]:].data_ptr()
        a.ln_g, a.ln_b = w["ln_gamma"].data_ptr(), w["ln_beta"].data_ptr()
        a.lnc_g, a.lnc_b = w["lnc_gamma"].data_ptr(), w["lnc_beta"].data_ptr()
        a.gstat, a.cstat = ch["gstat"].data_ptr(), ch["cstat"].data_ptr()
        self._call(self.lib.lib.skr_decode_vae_ln, "skr_decode_vae_ln", a)


def fused_vae_decoder(model, batch: int, steps: int, temperature: float = 1.0, greedy: bool = False,
                      chunk: int = 50, early_exit: bool = True):
    """The whole-sketch decoder that takes ``model``: :class:`FusedVAEDecoder`
    (plain ``lstm``) or :class:`FusedLNVAEDecoder` (``layer_norm``);
    ``ValueError`` for every other model (:func:`fused_vae_kind` is None)."""
    kind = fused_vae_kind(model)
    if kind is None:
        raise ValueError("fused_vae_decoder: needs a SketchVAE with an lstm or layer_norm decoder of size 256 "
                         "(M <= 32) or 512 (M <= 20)")
    cls = FusedVAEDecoder if kind == "lstm" else FusedLNVAEDecoder
    return cls(model, batch, steps, temperature, greedy, chunk, early_exit)


@torch.no_grad()
def ln_decode_step_transcription(model, x: torch.Tensor, zp: Optional[torch.Tensor], h: torch.Tensor,
                                 c: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One step of ``csrc/decode_vae_ln.hip`` in PyTorch, in the form the
    kernel computes it (the direct form: statistics of the complete gate
    pre-activations, exchanged after the stroke is known).

    ``x [B, 5]`` the fed stroke, ``zp [B, 4H] = zc @ W_x[5:]`` (None: no z
    input), ``h [B, H]`` the carried h **already rounded to bf16** (held as
    fp32), ``c [B, H]`` fp32. Returns ``(z [B, 3+6M], h', c')`` with ``h'``
    rounded to bf16 again, as the kernel stores it.

    What it models: W_h, W_out and the carried h in bf16 with fp32
    accumulation; the stroke and z terms in fp32; per block of 16 units a
    ``(mean_k, M2_k)`` partial, combined over the ``H/16`` blocks in block
    order as ``mean = sum mean_k / NW``, ``M2 = sum M2_k + 16 sum (mean_k -
    mean)^2``, ``rstd = rsqrt(M2 / H + 1e-3)``; the un-normalised fp32 ``c'``
    carried. What it does not: the MFMA's accumulation order and the
    device's exp / reciprocal -- the factor 2 in the GPU test's bound."""
    p, H, f32, bf = model.dec, model.cfg.dec_rnn_size, torch.float32, torch.bfloat16
    NW = H // 16

    def stats(v):                       # v [..., H] -> mean, rstd [..., 1]
        blk = v.reshape(*v.shape[:-1], NW, 16)
        mk = blk.sum(-1) * (1.0 / 16)
        qk = ((blk - mk[..., None]) ** 2).sum(-1)
        sm, sq = torch.zeros_like(mk[..., 0]), torch.zeros_like(mk[..., 0])
        for k in range(NW):             # block order
            sm = sm + mk[..., k]
            sq = sq + qk[..., k]
        mean = sm * (1.0 / NW)
        sd = torch.zeros_like(mean)
        for k in range(NW):
            sd = sd + (mk[..., k] - mean) ** 2
        rstd = torch.rsqrt((sq + 16.0 * sd) * (1.0 / H) + 1e-3)
        return mean[..., None], rstd[..., None]

    Wh = p.W_h.detach().to(bf).to(f32)
    Wx = p.W_x.detach().to(f32)
    g = h.to(f32) @ Wh + x.to(f32) @ Wx[:5]
    if zp is not None:
        g = g + zp
    B = g.shape[0]
    g4 = g.reshape(B, 4, H)
    mean, rstd = stats(g4)
    gn = (g4 - mean) * rstd * p.ln_gamma.detach().to(f32).reshape(4, H) + p.ln_beta.detach().to(f32).reshape(4, H)
    i, j, f, o = gn.unbind(1)
    c2 = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    mean, rstd = stats(c2)
    h2 = torch.tanh(p.lnc_gamma.detach().to(f32) * (c2 - mean) * rstd + p.lnc_beta.detach().to(f32)) * torch.sigmoid(o)
    h2 = h2.to(bf).to(f32)
    z = h2 @ model.output_w.detach().to(bf).to(f32) + model.output_b.detach().to(f32)
    return z, h2, c2
