"""Sketch generation.

Host samplers (exact semantics, any device, one sketch at a time):

* :func:`sample_reference` -- the reference's ``Model.sample``
  (``model.py:187-264``): zero first input, mixture temperature applied from
  step 2 on, inverse-CDF draws with the "-1 -> last component" rule, sigma
  NOT temperature-scaled, optional early stop on ``eoc`` (the ``eoc`` row is
  kept), offsets multiplied by ``data_scale``. The reference's pen-temperature
  bug (``pi_pdf /= temp_pen``, ``model.py:230``) is reproduced by default;
  ``fix_pen_temperature=True`` applies the temperature to the pen logits.
* :func:`sample_vae` -- sketch-rnn VAE semantics: start token
  ``[0, 0, 1, 0, 0]``, temperature on mixture and pen, sigma scaled by the
  temperature, optional greedy mode, ``z`` from N(0, I) or given.

Device sampler (:class:`GraphDecoder`): B sketches in parallel, the
N-step decode loop (decoder step -> MDN head -> ``csrc/sampler.hip``, which
writes the next input on device) captured once into a HIP graph and
replayed; finished rows emit end-of-sketch padding. No host round trip per
stroke (the reference does two ``sess.run`` transfers per stroke). HyperLSTM
decoders step through :class:`~.hyper_step.HyperStepDecoder` (state in
place, seven hand-written kernels per stroke); the reference model and
the VAE's plain ``lstm`` and ``layer_norm`` decoders have whole-sketch
decoders in :mod:`.fused` (the VAE ones are opt-in: ``vae_sample --fused``).
Many sketches at once go through :mod:`.stream`, which refills finished rows
with the next latent instead of padding them (``vae_sample --mode bulk``).
"""
from __future__ import annotations

import math
import os
import random as _random
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..models import mdn as M
from ..train.graph import capture


def _get_pi_idx(x: float, pdf: np.ndarray) -> int:
    acc = 0.0
    for i in range(pdf.size):
        acc += pdf[i]
        if acc >= x:
            return i
    return -1


def _softmax_np(v):
    v = np.asarray(v, dtype=np.float64)
    v = v - v.max()
    e = np.exp(v)
    return e / e.sum()


@torch.no_grad()
def sample_reference(model, num: int = 300, temp_mixture: float = 1.0, temp_pen: float = 1.0,
                     stop_if_eoc: bool = False, rng: Optional[np.random.RandomState] = None,
                     py_rng: Optional[_random.Random] = None, fix_pen_temperature: bool = False,
                     device=None):
    """Reference ``Model.sample``. Returns ``(strokes [n, 5], mixture_params)``."""
    rng = rng or np.random.RandomState()
    py_rng = py_rng or _random.Random()
    cfg = model.cfg
    dev = device or next(model.parameters()).device
    Mx = cfg.num_mixture
    prev_x = torch.zeros(1, 5, device=dev)
    state = model.zero_state(1, dev)
    strokes = np.zeros((num, 5), dtype=np.float32)
    params = []
    for i in range(num):
        z, next_state = model.step(prev_x, state)
        pi, mu1, mu2, s1, s2, rho, _, pen_logits = (t[0].double().cpu().numpy() for t in M.mixture_coef(z, Mx))
        pi_pdf = pi.copy()
        if i > 1:
            pi_pdf = np.log(pi_pdf) / temp_mixture
            pi_pdf -= pi_pdf.max()
            pi_pdf = np.exp(pi_pdf)
        pi_pdf /= pi_pdf.sum()
        idx = _get_pi_idx(py_rng.random(), pi_pdf)
        pen = pen_logits.copy()
        if i > 1:
            if fix_pen_temperature:
                pen = pen / temp_pen
            else:
                pi_pdf /= temp_pen  # reference bug: rescales pi, pen temperature has no effect
        pen_pdf = _softmax_np(pen)
        pen_idx = _get_pi_idx(py_rng.random(), pen_pdf)
        eos, eoc, cont = (1, 0, 0) if pen_idx == 0 else (0, 1, 0) if pen_idx == 1 else (0, 0, 1)
        cov = [[s1[idx] ** 2, rho[idx] * s1[idx] * s2[idx]], [rho[idx] * s1[idx] * s2[idx], s2[idx] ** 2]]
        x1, x2 = rng.multivariate_normal([mu1[idx], mu2[idx]], cov, 1)[0]
        strokes[i] = [x1, x2, eos, eoc, cont]
        params.append([pi_pdf, mu1, mu2, s1, s2, rho, pen_pdf])
        if stop_if_eoc and eoc == 1:
            strokes = strokes[: i + 1]
            break
        prev_x = torch.tensor([[x1, x2, eos, eoc, cont]], dtype=torch.float32, device=dev)
        state = next_state
    strokes[:, 0:2] *= cfg.data_scale
    return strokes, params


def _adjust_temp(pdf: np.ndarray, temp: float) -> np.ndarray:
    p = np.log(pdf) / temp
    p -= p.max()
    p = np.exp(p)
    return p / p.sum()


@torch.no_grad()
def sample_vae(model, seq_len: int = 250, temperature: float = 1.0, greedy: bool = False,
               z: Optional[torch.Tensor] = None, label: Optional[int] = None,
               rng: Optional[np.random.RandomState] = None, py_rng: Optional[_random.Random] = None,
               prefix=None):
    """One sketch from the VAE decoder. Returns ``(strokes5 [seq_len, 5], params)``
    in the magenta layout (convert with ``data.strokes.to_normal_strokes``).
    ``prefix [P, 5]`` (P <= seq_len, no end-of-sketch row) completes a
    sketch: it is fed as the first P strokes, then the decoder samples."""
    rng = rng or np.random.RandomState()
    py_rng = py_rng or _random.Random()
    cfg = model.cfg
    dev = next(model.parameters()).device
    if cfg.conditional and z is None:
        z = torch.as_tensor(rng.randn(1, cfg.z_size), dtype=torch.float32, device=dev)
    lab = torch.tensor([label], device=dev) if (label is not None and cfg.num_classes > 0) else None
    zc = model.condition(z if cfg.conditional else None, lab, 1, dev)
    state = model.initial_state(zc, 1, dev)
    prev_x = torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0]], device=dev)
    strokes = np.zeros((seq_len, 5), dtype=np.float32)
    params = []
    P = 0
    if prefix is not None:
        prefix = np.asarray(prefix, dtype=np.float32)
        if prefix.ndim != 2 or prefix.shape[1] != 5 or prefix.shape[0] > seq_len:
            raise ValueError("sample_vae: prefix must be [P, 5] with P <= seq_len")
        if (prefix[:, 4] > 0).any():
            raise ValueError("sample_vae: a prefix ends its sketch (pen state 4) inside its length")
        P = prefix.shape[0]
    for i in range(seq_len):
        zh, state = model.decode_step(prev_x, zc, state)
        pi, mu1, mu2, s1, s2, rho, pen, _ = (t[0].double().cpu().numpy() for t in M.mixture_coef(zh, cfg.num_mixture))
        if i < P:      # a given stroke: no draw (the random streams advance only on sampled strokes)
            strokes[i] = prefix[i]
            params.append([pi, mu1, mu2, s1, s2, rho, pen])
            prev_x = torch.as_tensor(prefix[i:i + 1], dtype=torch.float32, device=dev)
            continue
        if greedy:
            idx, pidx = int(np.argmax(pi)), int(np.argmax(pen))
            x1, x2 = mu1[idx], mu2[idx]
        else:
            idx = _get_pi_idx(py_rng.random(), _adjust_temp(pi, temperature))
            pidx = _get_pi_idx(py_rng.random(), _adjust_temp(pen, temperature))
            sa, sb = s1[idx] * temperature, s2[idx] * temperature
            cov = [[sa * sa, rho[idx] * sa * sb], [rho[idx] * sa * sb, sb * sb]]
            x1, x2 = rng.multivariate_normal([mu1[idx], mu2[idx]], cov, 1)[0]
        row = [x1, x2, 0.0, 0.0, 0.0]
        row[2 + pidx] = 1.0
        strokes[i] = row
        params.append([pi, mu1, mu2, s1, s2, rho, pen])
        prev_x = torch.tensor([row], dtype=torch.float32, device=dev)
    return strokes, params


# =====================================================================================
# device sampler + HIP graph decode
# =====================================================================================
_SAMPLE_STREAM = 0x5A3D
# GraphDecoder steps VAE decoders with the in-place step decoders
# (sample/hyper_step.py) where they apply; False: the generic decode_step.
STEP_DECODER = os.environ.get("SKR_STEP_DECODER", "1") != "0"


def check_prefix(name: str, prefix: torch.Tensor, prefix_len, B: int, N: int, dev):
    """Validate the stroke prefixes of a ``run(prefix=, prefix_len=)`` call
    (shared by :class:`GraphDecoder` and the whole-sketch decoders of
    :mod:`.fused`): ``prefix [B, P, 5]``, ``prefix_len [B]`` in
    ``[0, min(P, steps)]`` (default P), no end-of-sketch pen state inside a
    row's length. Returns ``(prefix fp32, prefix_len int64)`` on ``dev``;
    raises ``ValueError`` in ``name``'s name."""
    prefix = torch.as_tensor(prefix).to(dev, torch.float32)
    if prefix.dim() != 3:
        raise ValueError(name + ": prefix must be [B, P, 5] and prefix_len [B]")
    P = prefix.shape[1]
    plen = (torch.full((B,), P, dtype=torch.int64, device=dev) if prefix_len is None
            else torch.as_tensor(prefix_len).to(dev, torch.int64))
    if prefix.shape[0] != B or prefix.shape[2] != 5 or plen.shape != (B,):
        raise ValueError(name + ": prefix must be [B, P, 5] and prefix_len [B]")
    if bool((plen < 0).any()) or bool((plen > min(P, N)).any()):
        raise ValueError(name + ": prefix_len must lie in [0, min(P, steps)]")
    inside = torch.arange(P, device=dev)[None, :] < plen[:, None]
    if bool((inside & (prefix[:, :, 4] > 0)).any()):
        raise ValueError(name + ": a prefix ends its sketch (pen state 4) inside its length")
    return prefix, plen


def check_temperature(name: str, temperature, B: int, dev) -> torch.Tensor:
    """Validate the ``temperature=`` of a ``run()`` call (shared by
    :class:`GraphDecoder` and the whole-sketch decoders of :mod:`.fused`): a
    float, or a vector of ``B`` values, one per row; every value finite and
    greater than 0 (greedy decoding is the ``greedy`` flag, not a temperature
    of 0). Returns an fp32 ``[B]`` tensor on ``dev``; raises ``ValueError`` in
    ``name``'s name."""
    try:
        t = torch.as_tensor(temperature).to(dev, torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(name + ": temperature must be a float or a vector of %d floats" % B) from None
    if t.dim() == 0:
        t = t.expand(B)
    if t.shape != (B,):
        raise ValueError(name + ": temperature must be a float or a vector of %d floats, one per row" % B)
    if not bool(torch.isfinite(t).all()) or not bool((t > 0).all()):
        raise ValueError(name + ": temperatures must be finite and greater than 0 (greedy decoding is the greedy "
                                "flag)")
    return t.contiguous()


def mdn_sample_torch(zh: torch.Tensor, M_: int, mode: int, temp, greedy: bool, fix_pen: bool,
                     seed, step: int, out_row: torch.Tensor, next_x: torch.Tensor, done: torch.Tensor,
                     params: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None,
                     nforced: Optional[torch.Tensor] = None, row0: int = 0) -> None:
    """PyTorch transcription of ``csrc/sampler.hip`` (same hash random
    numbers, same draws): the CPU path of :class:`GraphDecoder` and the
    oracle the kernel is tested against.

    ``forced [B, 5]`` with ``nforced [B]``: a row with ``step < nforced[b]``
    emits ``forced[b]`` bit for bit instead of its draw, as ``out_row`` and as
    ``next_x``, takes its finished state from that row's stop column and
    never emits padding (``csrc/mdn_sample.h``). ``params`` keeps describing
    the draw.

    ``temp`` is a float, or an fp32 ``[B]`` tensor of per-row temperatures:
    row b then uses ``temp[b]`` wherever the scalar is used, with the
    reciprocal taken in fp32 per row as the kernel takes it (the scalar form
    keeps its Python-float reciprocal).

    ``row0``: the hash row of local row 0 (row b draws the noise of row
    ``row0 + b``; everything else stays indexed by the local row)."""
    from ..models.cells import hash_uniform
    B = zh.shape[0]
    z = zh.float()
    u = hash_uniform(seed, _SAMPLE_STREAM, step, (B, 4), device=z.device, offset=4 * int(row0))
    use_t = mode == 1 or step > 1
    if torch.is_tensor(temp):      # per row: 1 / temps and temps broadcast over the row's columns, in fp32
        tv = temp.to(z.device, torch.float32).reshape(B)
        inv_t, temp = (1.0 / tv).unsqueeze(-1), tv
    else:
        inv_t = 1.0 / temp
    logits = z[:, 3:3 + M_] * (inv_t if use_t else 1.0)
    pi = torch.softmax(logits, -1)
    ar = torch.arange(B, device=z.device)
    if greedy:
        idx = pi.argmax(-1)
    else:
        hit = torch.cumsum(pi, -1) >= u[:, 0:1]
        idx = torch.where(hit.any(-1), hit.float().argmax(-1), torch.full_like(ar, M_ - 1))
    pt = inv_t if (mode == 1 or (fix_pen and step > 1)) else 1.0
    pp = torch.softmax(z[:, 0:3] * pt, -1)
    if greedy:
        pidx = pp.argmax(-1)
    else:
        hit = torch.cumsum(pp, -1) >= u[:, 1:2]
        pidx = torch.where(hit.any(-1), hit.float().argmax(-1), torch.full_like(ar, 2))
    col = lambda k: z[ar, 3 + k * M_ + idx]  # noqa: E731
    mu1, mu2, s1, s2, rho = col(1), col(2), torch.exp(col(3)), torch.exp(col(4)), torch.tanh(col(5))
    if mode == 1:
        s1, s2 = s1 * temp, s2 * temp
    x1, x2 = mu1, mu2
    if not greedy:
        r = torch.sqrt(-2.0 * torch.log(torch.clamp(u[:, 2], min=1e-12)))
        n1, n2 = r * torch.cos(2 * math.pi * u[:, 3]), r * torch.sin(2 * math.pi * u[:, 3])
        x1 = mu1 + s1 * n1
        x2 = mu2 + s2 * (rho * n1 + torch.sqrt(torch.clamp(1 - rho * rho, min=0.0)) * n2)
    row = torch.zeros(B, 5, device=z.device)
    row[:, 0], row[:, 1] = x1, x2
    row[ar, 2 + pidx] = 1.0
    stop_col = 4 if mode == 1 else 3
    pad = torch.zeros(B, 5, device=z.device)
    pad[:, stop_col] = 1.0
    stop = pidx + 2 == stop_col
    emit = torch.where((done != 0).unsqueeze(-1), pad, row)
    if nforced is not None:    # a select: nothing of the draw (NaN included) reaches a forced row
        on = step < nforced.to(z.device).long()
        fr = forced.to(z.device, torch.float32)
        row = torch.where(on.unsqueeze(-1), fr, row)
        emit = torch.where(on.unsqueeze(-1), fr, emit)
        stop = torch.where(on, fr[:, stop_col] > 0, stop)
    out_row.copy_(emit)
    next_x.copy_(row)
    done.copy_(torch.where(stop, torch.ones_like(done), done))
    if params is not None:
        params.copy_(torch.stack([idx.float(), pidx.float(), s1, s2], -1))


def mdn_sample_device(zh: torch.Tensor, M_: int, mode: int, temp, greedy: bool, fix_pen: bool,
                      seed: torch.Tensor, step: int, out_row: torch.Tensor, next_x: torch.Tensor,
                      done: torch.Tensor, params: Optional[torch.Tensor] = None,
                      forced: Optional[torch.Tensor] = None, nforced: Optional[torch.Tensor] = None,
                      row0: int = 0, row_base: Optional[torch.Tensor] = None) -> None:
    """``csrc/sampler.hip`` on a GPU tensor, :func:`mdn_sample_torch` elsewhere.
    ``forced [B, 5]`` (any row stride) with ``nforced [B]`` int32: rows with
    ``step < nforced[b]`` emit ``forced[b]`` instead of their draw. ``temp``: a
    float, or an fp32 ``[B]`` tensor of per-row temperatures. The hash row of
    local row 0 is ``row0`` plus the int32 device word ``row_base`` (a captured
    launch then serves any block of a longer job list)."""
    if torch.is_tensor(temp) and (temp.dtype != torch.float32 or temp.shape != (zh.shape[0],)):
        raise ValueError("mdn_sample_device: per-row temperatures must be an fp32 [B] tensor")
    if (forced is None) != (nforced is None):
        raise ValueError("mdn_sample_device: forced and nforced go together")
    if zh.device.type != "cuda":
        return mdn_sample_torch(zh, M_, mode, temp, greedy, fix_pen, seed, step, out_row, next_x, done, params,
                                forced, nforced, row0 + (int(row_base) if row_base is not None else 0))
    assert zh.dtype == torch.float32 and zh.stride(1) == 1 and zh.shape[1] >= 3 + 6 * M_
    assert out_row.dtype == torch.float32 and out_row.stride(-1) == 1 and out_row.shape[0] == zh.shape[0]
    assert next_x.shape == (zh.shape[0], 5) and next_x.stride(-1) == 1
    assert done.dtype == torch.int32 and done.numel() == zh.shape[0] and seed.dtype == torch.int64
    from ..utils import native
    lib = native.require_hip()
    B = zh.shape[0]
    if nforced is not None:
        assert forced.dtype == torch.float32 and forced.shape == (B, 5) and forced.stride(1) == 1
        assert nforced.dtype == torch.int32 and nforced.shape == (B,) and nforced.stride(0) == 1
    # one entry point for every combination (the others forward to it); a strided temperature view is copied,
    # the kernel indexes temps[b]
    temps = temp.contiguous() if torch.is_tensor(temp) else None
    assert temps is None or temps.device == zh.device
    assert row_base is None or (row_base.dtype == torch.int32 and row_base.numel() == 1 and row_base.is_cuda)
    rc = lib.lib.skr_mdn_sample_rows(
        zh.data_ptr(), zh.stride(0), B, M_, mode, 1.0 if temps is not None else temp, int(greedy), int(fix_pen),
        seed.data_ptr(), step, int(row0), out_row.data_ptr(), out_row.stride(0), next_x.data_ptr(),
        next_x.stride(0), done.data_ptr(), params.data_ptr() if params is not None else None,
        forced.data_ptr() if nforced is not None else None, forced.stride(0) if nforced is not None else 0,
        nforced.data_ptr() if nforced is not None else None, temps.data_ptr() if temps is not None else None,
        row_base.data_ptr() if row_base is not None else None, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("skr_mdn_sample_rows failed (%d)" % rc)


class GraphDecoder:
    """Batched autoregressive decode captured in HIP graphs.

    ``model`` is a :class:`~sketch_rnn_amd.models.reference.SketchRNN` (mode
    ``reference``) or :class:`~sketch_rnn_amd.models.vae.SketchVAE` (mode
    ``vae``). ``run()`` returns ``strokes [B, N, 5]`` (offsets in model
    units; reference mode multiplies by ``data_scale``) plus the per-row
    number of valid steps.

    The N steps are captured as consecutive chunks of ``chunk`` steps, one
    graph each (one memory pool). After each chunk the host reads whether
    every row has drawn its end-of-sketch pen state; if so the remaining
    chunks are skipped and their output rows are filled with the padding
    row the sampler would have emitted (reference: model.py:254-257, the
    ``stop_if_eoc`` break). The emitted sketches are identical to the
    full-length decode: finished rows only ever emit padding, and the
    sampler's noise is keyed by (seed, step, row), not by a running state.
    ``steps_run`` records how many decode steps the last ``run()`` executed.
    """

    CHUNK = 25               # steps per captured graph (one host read of the all-done flag per chunk)

    def __init__(self, model, batch: int, steps: int, temperature: float = 1.0, greedy: bool = False,
                 fix_pen_temperature: bool = False, use_graph: bool = True, chunk: Optional[int] = None,
                 early_exit: bool = True, fp8: bool = False):
        self.model = model
        self.kind = "vae" if hasattr(model, "encoder") else "reference"
        self.B, self.N = batch, steps
        self.temp, self.greedy, self.fix_pen = float(temperature), bool(greedy), bool(fix_pen_temperature)
        dev = next(model.parameters()).device
        self.dev = dev
        cfg = model.cfg
        self.Mx = cfg.num_mixture
        self.mode = 1 if self.kind == "vae" else 0
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.out = torch.zeros(batch, steps, 5, device=dev)
        self.done = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.x0 = torch.zeros(batch, 5, device=dev)
        # per-row temperatures: static like the prefix buffers below, read by every sampler call of every
        # step path, so run(temperature=) never causes a recapture
        self.temps = torch.full((batch,), self.temp, dtype=torch.float32, device=dev)
        if self.kind == "vae":
            self.x0[:, 2] = 1.0
            self.z = torch.zeros(batch, max(cfg.z_size, 1), device=dev)
            self.labels = torch.zeros(batch, dtype=torch.int64, device=dev)
            # stroke prefixes (sketch completion): static, so the captured graphs always carry them and a
            # prefix never causes a recapture; nforced all zero = a plain decode
            self.prefix = torch.zeros(batch, steps, 5, device=dev)
            self.nforced = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.graphs = None
        self.use_graph = use_graph and dev.type == "cuda"
        c = int(chunk or self.CHUNK)
        self.ranges = [(t, min(t + c, steps)) for t in range(0, steps, c)] if steps > 0 else []
        self.early_exit = bool(early_exit)
        self.fp8 = bool(fp8)   # MX-fp8 h W_h in the HyperLSTM step decoders (BASELINE config 5)
        self.steps_run = 0
        # hash row of row 0 (run(row0=)): a device word every sampler call reads, so it never causes a recapture
        self.row_base = torch.zeros(1, dtype=torch.int32, device=dev)
        self._carry = {}     # tensors handed from one chunk to the next (state, next input, zc)

    _MAX_CHUNKS = 8          # concurrent 128-row step decoders (one HIP stream each)

    def _steppers(self):
        """Lean in-place HyperLSTM step decoders (``sample/hyper_step.py``), one
        per chunk of <= 128 rows, when the model qualifies; else None.

        Chunks run CONCURRENTLY, one stream each (captured as parallel graph
        branches): each stroke's chain is latency-bound, so a second chain
        fills the idle CUs. Only chunk 0's main cell uses the clustered
        LayerNorm exchange (co-resident spin-waits); the others keep every
        row in one workgroup, so no two spin-waiting launches ever compete
        for residency."""
        if self.kind != "vae" or self.dev.type != "cuda" or not STEP_DECODER:
            return None
        from .hyper_step import HyperStepDecoder, hyper_step_ok, wide_ok
        if self.B > 128 and self.B % 128 == 0 and self.B <= 1024 and wide_ok(self.model):
            chunks = [(0, self.B)]   # one wide decoder: 128-row blocks inside each launch
        else:
            chunks = [(r0, min(128, self.B - r0)) for r0 in range(0, self.B, 128)]
        if len(chunks) > self._MAX_CHUNKS or not all(hyper_step_ok(self.model, n) for _, n in chunks):
            return None
        if getattr(self, "_stp", None) is None:
            # chunk 0 runs on whatever stream is current at decode time (None)
            self._stp = [(r0, n, HyperStepDecoder(self.model, n, self.dev, cluster=(i == 0), fp8=self.fp8),
                          None if i == 0 else torch.cuda.Stream(device=self.dev))
                         for i, (r0, n) in enumerate(chunks)]
        return self._stp

    @torch.no_grad()
    def _decode_steppers(self, stp, t0, t1):
        import ctypes
        from ..utils import native
        lib = native.require_hip().lib
        model, B, N = self.model, self.B, self.N
        cfg = model.cfg
        ld_out, ld_pre = self.out.stride(0), self.prefix.stride(0)
        main = torch.cuda.current_stream(self.dev)
        stp = [(r0, n, st, main if stream is None else stream) for r0, n, st, stream in stp]
        cy = self._carry
        if t0 == 0:
            lab = self.labels if cfg.num_classes > 0 else None
            cy["zc"] = zc = model.condition(self.z if cfg.conditional else None, lab, B, self.dev)
            cy["state"] = model.initial_state(zc, B, self.dev)
            cy["x0"] = self.x0.clone()
            for _, _, st, _ in stp:              # weight operands on the parent stream
                st.prepare()
        zc, state, x0 = cy["zc"], cy["state"], cy["x0"]
        for _, _, _, stream in stp:              # fork: inputs above are ready
            if stream != main:
                stream.wait_stream(main)
        for i, (r0, n, st, stream) in enumerate(stp):
            if st.fused:       # four launches per stroke (hyper_step.py module docstring)
                with torch.cuda.stream(stream):
                    if t0 == 0:
                        st.begin(zc[r0:r0 + n] if zc is not None else None, [s[r0:r0 + n] for s in state],
                                 x0=x0[r0:r0 + n])
                    done = self.done[r0:r0 + n]
                    for t in range(t0, t1):
                        smp = None if t == 0 else st.sample_args(
                            t - 1, r0, self.out[r0:r0 + n, t - 1], done, self.seed, self.Mx, self.mode, self.temp,
                            self.greedy, self.fix_pen, forced=self.prefix[r0:r0 + n, t - 1],
                            nforced=self.nforced[r0:r0 + n], temps=self.temps[r0:r0 + n])
                        if smp is not None:
                            smp.first_row = self.row_base.data_ptr()     # run(row0=): a device word
                        st.step_fused(t, smp)
                    if t1 == N:
                        st.head()          # the last stroke: head + sampler
                        rc = lib.skr_mdn_sample_slabs_rows(
                            st.ZS.data_ptr(), 128, st.S_o, n * 128, st._w["bo"].data_ptr(), n, self.Mx, self.mode,
                            self.temp, int(self.greedy), int(self.fix_pen), self.seed.data_ptr(), N - 1,
                            r0,
                            self.out[r0, N - 1].data_ptr(), ld_out, st.X.data_ptr(), 5, done.data_ptr(),
                            self.prefix[r0, N - 1].data_ptr(), ld_pre, self.nforced[r0:].data_ptr(),
                            self.temps[r0:].data_ptr(), self.row_base.data_ptr(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                        if rc != 0:
                            raise RuntimeError("skr_mdn_sample_slabs_rows failed (%d)" % rc)
                continue
            with torch.cuda.stream(stream):
                if t0 == 0:
                    st.begin(zc[r0:r0 + n] if zc is not None else None, [s[r0:r0 + n] for s in state])
                    cy["x%d" % i] = x0[r0:r0 + n].contiguous()
                x = cy["x%d" % i]
                for t in range(t0, t1):
                    nx = torch.empty(n, 5, device=self.dev)

                    def sample(zs, ldz, nslab, slab, bias, r0=r0, n=n, t=t, nx=nx):
                        rc = lib.skr_mdn_sample_slabs_rows(
                            zs.data_ptr(), ldz, nslab, slab, bias.data_ptr(), n, self.Mx, self.mode, self.temp,
                            int(self.greedy), int(self.fix_pen), self.seed.data_ptr(), t, r0,
                            self.out[r0, t].data_ptr(), ld_out, nx.data_ptr(), 5, self.done[r0:].data_ptr(),
                            self.prefix[r0, t].data_ptr(), ld_pre, self.nforced[r0:].data_ptr(),
                            self.temps[r0:].data_ptr(), self.row_base.data_ptr(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                        if rc != 0:
                            raise RuntimeError("skr_mdn_sample_slabs_rows failed (%d)" % rc)
                    st.step(x, t, sample)
                    x = nx
                cy["x%d" % i] = x
        for _, _, _, stream in stp:
            if stream != main:
                main.wait_stream(stream)          # join

    @torch.no_grad()
    def _decode(self, t0: int, t1: int):
        """Decode steps [t0, t1); t0 == 0 starts a sketch (state, done flags)."""
        model, B = self.model, self.B
        if t0 == 0:
            self.done.zero_()
        stp = self._steppers()
        if stp is not None:
            fused = {st.fused for _, _, st, _ in stp}
            # fused step decoders draw stroke t inside step t + 1's launch: after
            # steps [t0, t1) the done flags cover strokes < t1 - 1
            self._lag = 1 if fused == {True} else (0 if fused == {False} else None)
            return self._decode_steppers(stp, t0, t1)
        self._lag = 0
        cy = self._carry
        if t0 == 0:
            cy["x"] = self.x0.clone()
            if self.kind == "vae":
                cfg = model.cfg
                lab = self.labels if cfg.num_classes > 0 else None
                cy["zc"] = model.condition(self.z if cfg.conditional else None, lab, B, self.dev)
                cy["state"] = model.initial_state(cy["zc"], B, self.dev)
            else:
                cy["zc"] = None
                cy["state"] = model.zero_state(B, self.dev)
        x, zc, state = cy["x"], cy["zc"], cy["state"]
        for t in range(t0, t1):
            if self.kind == "vae":
                zh, state = model.decode_step(x, zc, state)
            else:
                zh, state = model.step(x, state)
            nx = torch.empty(B, 5, device=self.dev)
            forced = (self.prefix[:, t], self.nforced) if self.kind == "vae" else (None, None)
            mdn_sample_device(zh.contiguous(), self.Mx, self.mode, self.temps, self.greedy, self.fix_pen, self.seed, t,
                              self.out[:, t], nx, self.done, None, *forced, row_base=self.row_base)
            x = nx
        cy["x"], cy["state"] = x, state

    def _exit_after(self, t1: int) -> bool:
        return self.early_exit and self._lag is not None and t1 < self.N and bool(self.done.all())

    def _pad_from(self, t: int):
        """Rows of steps [t, N) as the sampler emits them for finished rows."""
        if t < self.N:
            self.out[:, t:].zero_()
            self.out[:, t:, 4 if self.kind == "vae" else 3] = 1.0

    @torch.no_grad()
    def run(self, seed: int = 0, z: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
            prefix: Optional[torch.Tensor] = None, prefix_len: Optional[torch.Tensor] = None,
            temperature=None, row0: int = 0):
        """Returns ``(strokes [B, N, 5], lengths [B])``.

        ``row0``: row b draws the sampler noise of row ``row0 + b`` (a block of
        a longer job list keeps its rows' noise, :mod:`.stream`). It fills a
        device word the captured graphs read, so it never causes a recapture.

        ``temperature``: a float, or a vector of B values (row b samples at
        ``temperature[b]``), for this run only; None is the constructor's
        value. It fills a static buffer the captured graphs read, so a
        temperature never causes a recapture.

        ``prefix [B, P, 5]`` with ``prefix_len [B]`` (default P for every row;
        VAE models only) completes sketches: stroke t of row b is
        ``prefix[b, t]`` for ``t < prefix_len[b]`` and the decoder continues
        from there (the contract of the whole-sketch decoders in
        :mod:`.fused`). The prefix is copied into static buffers the captured
        graphs read, so it never causes a recapture, and a later run without
        one is a plain decode."""
        if temperature is None:
            self.temps.fill_(self.temp)
        else:
            self.temps.copy_(check_temperature("GraphDecoder.run", temperature, self.B, self.dev))
        if prefix is not None or prefix_len is not None:
            if self.kind != "vae":
                raise ValueError("GraphDecoder.run: stroke prefixes need a VAE model")
            if prefix is None:
                raise ValueError("GraphDecoder.run: prefix_len without a prefix")
            prefix, plen = check_prefix("GraphDecoder.run", prefix, prefix_len, self.B, self.N, self.dev)
            Pn = min(prefix.shape[1], self.N)
            self.prefix[:, :Pn].copy_(prefix[:, :Pn])
            self.nforced.copy_(plen)
        elif self.kind == "vae":
            self.nforced.zero_()
        if z is not None:
            self.z.copy_(z)
        elif self.kind == "vae":
            g = torch.Generator(device=self.dev).manual_seed(int(seed))
            self.z.copy_(torch.randn(self.z.shape, device=self.dev, generator=g))
        if labels is not None:
            self.labels.copy_(labels)
        self.seed.fill_(int(seed))
        if int(row0) < 0 or int(row0) + self.B >= 2 ** 30:     # (the hash indexes element 4 * row + k in 32 bits)
            raise ValueError("GraphDecoder.run: row0 must be >= 0 and row0 + batch below 2^30")
        self.row_base.fill_(int(row0))
        ran = self.N
        if self.use_graph:
            # the graphs hold inference-cached weight copies (bf16): re-capture after a weight update
            from ..ops import gemm
            sig = (gemm.WEIGHTS_EPOCH[0],) + tuple(p._version for p in self.model.parameters())
            if self.graphs is not None and sig != self._sig:
                self.graphs = None
            self._sig = sig
            if self.graphs is None:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for t0, t1 in self.ranges:
                        self._decode(t0, t1)
                torch.cuda.current_stream().wait_stream(s)
                self.graphs, pool = [], None
                for t0, t1 in self.ranges:
                    g = torch.cuda.CUDAGraph()
                    with capture(g, pool=pool):
                        self._decode(t0, t1)
                    pool = g.pool() if pool is None else pool
                    self.graphs.append(g)
            for (t0, t1), g in zip(self.ranges, self.graphs):
                g.replay()
                ran = t1
                if self._exit_after(t1):   # one host read per chunk
                    break
        else:
            for t0, t1 in self.ranges:
                self._decode(t0, t1)
                ran = t1
                if self._exit_after(t1):
                    break
        if ran < self.N:
            self._pad_from(ran - self._lag)   # strokes the skipped launches would have drawn: all padding
        self.steps_run = ran
        strokes = self.out.clone()
        stop_col = 4 if self.kind == "vae" else 3
        hits = strokes[:, :, stop_col] > 0
        lengths = torch.where(hits.any(1), hits.float().argmax(1) + 1, torch.full_like(hits[:, 0], self.N,
                                                                                      dtype=torch.long))
        if self.kind == "reference":
            strokes[:, :, 0:2] *= self.model.cfg.data_scale
        return strokes, lengths
