#!/usr/bin/env python3
"""Generation throughput: temperature-sampled decode of the VAE decoder.

``--impl fused`` times the whole-sketch kernel (``fused_vae_decoder``: plain
``lstm`` and ``layer_norm`` decoders) in place of ``GraphDecoder``, falling
back to it with a printed reason for a model or device the kernels do not
take; both report the same fields.

Compares (a) the HIP-graph batched decoder (``GraphDecoder``: decoder step
kernels + MDN head + device sampler kernel, captured in chunks of steps with
an all-done exit after each chunk) against (b) the reference-style host loop
(one sketch at a time, one device round trip per stroke). Prints one JSON
line with

* ``valid_strokes_per_s`` -- sum of the sampled sketch lengths / wall time
  (the strokes a user gets; padding after a row's end-of-sketch excluded);
* ``decode_positions_per_s`` -- batch x decode steps actually run / wall time
  (row-steps the decoder computed, padding rows included);
* ``steps_run`` -- decode steps per sketch batch after the early exit.

``--impl stream --jobs J [--slots S] [--chunk C]`` times bulk generation
(``sample.stream.StreamDecoder``: S decoder rows, finished rows refilled with
the next of J latents) and reports the same fields plus ``occupancy`` (valid
strokes per computed row-step). With ``--jobs J`` the ``graph`` arm loops
``GraphDecoder.run`` over the same J latents in batches of ``--batch``, so the
two arms deliver the same number of sketches. ``--impl`` takes a
comma-separated list (``graph,stream,graph,stream``): the arms run in that
order in one process on one model, one JSON line each; ``--chunk`` takes a
list too, every stream arm running once per value.

``--train-steps N`` first trains the model N steps on synthetic sketches
(random-init models end their sketches after a handful of strokes, which
makes every throughput look like padding).

``--prefix_len P`` (sketch completion, both ``--impl`` arms) feeds a synthetic
P-stroke pen-down prefix to every row; the decoder continues from it.

``--temperatures T0,T1,...`` (both ``--impl`` arms) decodes with a
temperature per row, the listed values spread over the rows in turn
(``run(temperature=)``); the decoder is still built at ``--temperature``.

usage: python scripts/bench_sample.py [--config vae_large] [--batch 256] [--steps 250] [--train-steps 0]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vae_large")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--host-steps", type=int, default=50, help="strokes timed for the host-loop comparator")
    ap.add_argument("--train-steps", type=int, default=0, help="train this many steps first (synthetic data)")
    ap.add_argument("--no-early-exit", action="store_true")
    ap.add_argument("--fp8", action="store_true", help="MX-fp8 h W_h in the HyperLSTM step decoder (BASELINE config 5)")
    ap.add_argument("--impl", default="graph",
                    help="graph: GraphDecoder; fused: the whole-sketch kernel (fused_vae_decoder: plain lstm and "
                         "layer_norm decoders); stream: StreamDecoder over --jobs latents; a comma-separated list "
                         "runs its arms in order in one process")
    ap.add_argument("--jobs", type=int, default=0,
                    help="latents to decode per repetition (stream; graph: looped in batches of --batch)")
    ap.add_argument("--slots", type=int, default=0, help="stream: decoder rows (default --batch)")
    ap.add_argument("--chunk", default=None,
                    help="stream: decode steps per replayed graph (comma-separated: one run per value)")
    ap.add_argument("--prefix_len", type=int, default=0,
                    help="feed a synthetic prefix of this many strokes to every row (sketch completion)")
    ap.add_argument("--temperatures", default=None,
                    help="comma-separated temperatures spread over the rows in turn (per-row temperature)")
    a = ap.parse_args()
    if not 0 <= a.prefix_len <= a.steps:
        ap.error("--prefix_len must lie in [0, --steps]")
    arms = a.impl.split(",")
    if not all(x in ("graph", "fused", "stream") for x in arms):
        ap.error("--impl: graph, fused, stream, or a comma-separated list of them")
    if "stream" in arms and (a.jobs < 1 or a.prefix_len or a.fp8):
        ap.error("--impl stream needs --jobs >= 1 and takes neither --prefix_len nor --fp8")
    if len(arms) > 1 or a.jobs > 0:
        if "fused" in arms or a.prefix_len or a.temperatures:
            ap.error("--jobs and lists of arms take graph and stream, without --prefix_len and --temperatures")
    chunks = [int(c) for c in a.chunk.split(",")] if a.chunk else [None]
    import numpy as np
    import torch
    from sketch_rnn_amd import ops
    from sketch_rnn_amd.config import PRESETS
    from sketch_rnn_amd.models.vae import SketchVAE
    from sketch_rnn_amd.sample.sampler import GraphDecoder, sample_vae

    ops.set_backend("hip")
    ops.set_compute_dtype(a.dtype)
    cfg = PRESETS[a.config].replace(max_seq_len=a.steps)
    train_cost = None
    if a.train_steps > 0:
        from sketch_rnn_amd.data.dataset import StrokeDataset
        from sketch_rnn_amd.data.synthetic import synthetic_corpus
        from sketch_rnn_amd.train.trainer import VAETrainer
        tcfg = cfg.replace(batch_size=100, save_every=0)
        strokes, labels = synthetic_corpus(4000, seed=1234, max_len=a.steps, n_classes=max(cfg.num_classes, 1))
        ds = StrokeDataset(strokes, tcfg.batch_size, a.steps, labels=labels, seed=7)
        ds.normalize()
        tr = VAETrainer(tcfg, ds, None, None, device="cuda", save_dir="/tmp/skr_bench_sample", log=lambda s: None,
                        compute_dtype=a.dtype)
        for _ in range(a.train_steps):
            out = tr.train_step(*tr.batch_to_device(ds.random_batch()))
        train_cost = float(out["cost"])
        model = tr.model.eval()
    else:
        model = SketchVAE(cfg, seed=0).cuda().eval()
    pre = {}
    if a.prefix_len > 0:       # pen-down strokes of the data's scale (unit offsets)
        p5 = torch.zeros(a.batch, a.prefix_len, 5, device="cuda")
        p5[..., :2] = torch.randn(a.batch, a.prefix_len, 2, device="cuda",
                                  generator=torch.Generator(device="cuda").manual_seed(0)) * 0.5
        p5[..., 2] = 1.0
        pre = dict(prefix=p5)
    if a.temperatures is not None:
        tv = torch.tensor([float(t) for t in a.temperatures.split(",")], device="cuda")
        pre["temperature"] = tv[torch.arange(a.batch, device="cuda") % tv.numel()]
    if len(arms) > 1 or a.jobs > 0:
        return bulk_arms(a, arms, chunks, model, train_cost)
    dec, impl = None, a.impl
    if a.impl == "fused":
        from sketch_rnn_amd.sample.fused import NotCoResident, fused_vae_decoder
        try:
            dec = fused_vae_decoder(model, a.batch, a.steps, a.temperature, early_exit=not a.no_early_exit)
            dec.run(seed=0, **pre)
        except (ValueError, NotCoResident) as e:
            print("--impl fused: %s; using the graph decoder" % e, file=sys.stderr)
            dec, impl = None, "graph"
    if dec is None:
        dec = GraphDecoder(model, a.batch, a.steps, a.temperature, early_exit=not a.no_early_exit, fp8=a.fp8)
    dec.run(seed=0, **pre)  # capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total_len = total_pos = 0
    for r in range(a.reps):
        s, lens = dec.run(seed=r + 1, **pre)
        total_len += int(lens.sum())
        total_pos += a.batch * dec.steps_run
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dt = wall / a.reps
    # host loop comparator (reference-style: one sketch, one round trip per stroke)
    t0 = time.perf_counter()
    sample_vae(model, a.host_steps, a.temperature, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    hdt = time.perf_counter() - t0
    host_sps = a.host_steps / hdt
    valid_sps = total_len / wall
    print(json.dumps({"metric": "sampled valid strokes/sec (temperature %.2f)" % a.temperature, "config": a.config,
                      "impl": impl, "dtype": a.dtype, "fp8_gemm": bool(a.fp8), "batch": a.batch, "steps": a.steps, "train_steps": a.train_steps,
                      "train_cost": train_cost, "early_exit": not a.no_early_exit, "prefix_len": a.prefix_len,
                      "temperatures": a.temperatures,
                      "valid_strokes_per_s": round(valid_sps, 1),
                      "decode_positions_per_s": round(total_pos / wall, 1),
                      "steps_run": total_pos / a.batch / a.reps,
                      "ms_per_sketch_batch": round(1000 * dt, 3),
                      "ms_per_decode_step": round(1000 * wall / (total_pos / a.batch), 4),
                      "host_loop_strokes_per_s": round(host_sps, 1),
                      "speedup_valid_vs_host": round(valid_sps / host_sps, 1),
                      "mean_len": total_len / a.batch / a.reps}), flush=True)


def bulk_arms(a, arms, chunks, model, train_cost):
    """The arms of a job list, in order, on one model: ``graph`` loops
    GraphDecoder.run over the latents in batches of --batch, ``stream`` hands
    them to one StreamDecoder of --slots rows. One JSON line per run."""
    import torch
    from sketch_rnn_amd.sample.sampler import GraphDecoder
    from sketch_rnn_amd.sample.stream import StreamDecoder
    J = a.jobs if a.jobs > 0 else a.batch
    slots = a.slots or a.batch
    z = torch.randn(J, model.cfg.z_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    decs = {}
    for arm in arms:
        for chunk in (chunks if arm == "stream" else [None]):
            key = (arm, chunk)
            if key not in decs:
                if arm == "stream":
                    decs[key] = StreamDecoder(model, slots, a.steps, a.temperature, chunk=chunk)
                    decs[key].run(z, seed=0)          # capture
                else:
                    decs[key] = GraphDecoder(model, a.batch, a.steps, a.temperature, early_exit=not a.no_early_exit)
                    decs[key].run(seed=0, z=z[:a.batch])
            dec = decs[key]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            total_len = total_pos = steps = 0
            for r in range(a.reps):
                if arm == "stream":
                    _, lens = dec.run(z, seed=r + 1)
                    total_len += int(lens.sum())
                    total_pos += dec.slot_steps
                    steps += dec.steps_run
                else:
                    for j0 in range(0, J - a.batch + 1, a.batch):
                        _, lens = dec.run(seed=r + 1, z=z[j0:j0 + a.batch])
                        total_len += int(lens.sum())
                        total_pos += a.batch * dec.steps_run
                        steps += dec.steps_run
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            done = J if arm == "stream" else J // a.batch * a.batch
            print(json.dumps({"metric": "sampled valid strokes/sec (temperature %.2f)" % a.temperature,
                              "config": a.config, "impl": arm, "path": getattr(dec, "impl", "graph"),
                              "dtype": a.dtype, "jobs": done, "batch": a.batch if arm == "graph" else slots,
                              "chunk": getattr(dec, "chunk", None) if arm == "stream" else None,
                              "steps": a.steps, "train_steps": a.train_steps, "train_cost": train_cost,
                              "valid_strokes_per_s": round(total_len / wall, 1),
                              "decode_positions_per_s": round(total_pos / wall, 1),
                              "steps_run": steps / a.reps,
                              "occupancy": round(total_len / total_pos, 4) if total_pos else 0.0,
                              "ms_per_job_list": round(1000 * wall / a.reps, 3),
                              "ms_per_decode_step": round(1000 * wall / max(steps, 1), 4),
                              "mean_len": total_len / done / a.reps}), flush=True)


if __name__ == "__main__":
    main()
