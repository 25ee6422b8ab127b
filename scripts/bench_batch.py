#!/usr/bin/env python3
"""Time batch assembly on the device (csrc/batch.hip, ``--device_data``)
against the host path (``StrokeDataset.random_batch`` behind the prefetch
thread) on one GPU.

* **per batch**, vae_large's shape (B = 100, Nmax = 250, f = 0.15, prob =
  0.1), at a corpus of ``--sketches`` synthetic sketches and at that corpus
  tiled to about ``--large`` sketches (the same sketches repeated: the large
  corpus is there for the host's O(corpus) permutation). Host arm:
  ``random_batch`` + pin + host-to-device copy, which is what
  ``Prefetcher._stage`` and ``batch_to_device`` do, by the host clock, the best
  of the windows. Device arm: ``ops.batch.assemble`` into preallocated outputs,
  device events over windows of at least ``--window`` seconds. The arms
  alternate host, device, host, device ... in one process after a warm-up.
* **whole step**, vae_small and vae_large in bf16 from one captured graph,
  ``--steps`` steps per run: ``StrokeDataset`` + prefetch against the device
  dataset, alternated prefetch, device, prefetch, device in one process after a
  warm-up run of each; host clock around ``VAETrainer.train`` with the final
  checkpoint write taken out, closed by a device synchronisation.

Every part runs in a child process of its own under ``timeout -k 10``; the
first part that fails ends the run. Writes ``bench_batch.jsonl`` and a
``README.md`` into ``--out``.
Usage: ``python scripts/bench_batch.py [--out profiles/r18/batch]``
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, NMAX, F, PROB = 100, 250, 0.15, 0.1


def _emit(path, rec):
    print(json.dumps(rec), flush=True)
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")


def part_batch(a) -> int:
    import numpy as np
    import torch
    from sketch_rnn_amd.data.dataset import StrokeDataset
    from sketch_rnn_amd.data.device_dataset import DeviceStrokeDataset
    from sketch_rnn_amd.data.synthetic import synthetic_corpus
    from sketch_rnn_amd.utils import native
    native.require_hip()
    dev = torch.device("cuda:0")
    strokes, labels = synthetic_corpus(a.sketches, seed=0, max_len=NMAX)
    host = StrokeDataset(strokes, B, NMAX, random_scale_factor=F, augment_stroke_prob=PROB, labels=labels)
    host.normalize()
    tiles = max(1, a.tile)
    if tiles > 1:       # the same sketches again: the lists are tiled, not regenerated
        host.strokes = host.strokes * tiles
        host.labels = np.tile(host.labels, tiles)
    dd = DeviceStrokeDataset.from_dataset(host, dev, seed=0)
    S = len(host)
    assert len(dd) == S
    out = dd.random_batch(0)

    def host_window(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            s, l, c = host.random_batch()
            staged = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in (s, l, c)]
            keep = [t.to(dev, non_blocking=True) for t in staged]
        torch.cuda.synchronize()
        del keep
        return (time.perf_counter() - t0) / n

    step = [1]

    def dev_window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            dd.random_batch(step[0], out=out)
            step[0] += 1
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    # warm-up and calibration
    host_window(2)
    dev_window(20)
    n_host = max(5, int(math.ceil(a.window / max(host_window(2), 1e-7))))
    n_dev = max(20, int(math.ceil(a.window / max(dev_window(20), 1e-8))))
    hw, dw = [], []
    for _ in range(a.rounds):
        hw.append(host_window(n_host))
        dw.append(dev_window(n_dev))
    t0 = time.perf_counter()
    for _ in range(5):
        host.rng.permutation(S)[:B]
    perm = (time.perf_counter() - t0) / 5
    mean = sum(dw) / len(dw)
    _emit(a.records, dict(part="batch", sketches=S, tiles=tiles, points=int(dd.corpus.offsets[-1]), B=B, Nmax=NMAX,
                          random_scale_factor=F, augment_stroke_prob=PROB,
                          host_ms=min(hw) * 1e3, host_windows_s=hw, host_batches_per_window=n_host,
                          host_permutation_ms=perm * 1e3,
                          device_ms=mean * 1e3, device_min_ms=min(dw) * 1e3, device_windows_s=dw,
                          device_batches_per_window=n_dev, device_spread=(max(dw) - min(dw)) / mean,
                          host_over_device=min(hw) / mean,
                          device=torch.cuda.get_device_name(0), lib=native.hip_lib_stamp()))
    return 0


def part_step(a) -> int:
    import dataclasses
    import torch
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.config import PRESETS
    from sketch_rnn_amd.data.device_dataset import DeviceStrokeDataset
    from sketch_rnn_amd.train.trainer import VAETrainer
    from sketch_rnn_amd.utils import native
    native.require_hip()
    dev = "cuda:0"
    cfg = dataclasses.replace(PRESETS[a.preset], save_every=0)
    (train, _, _), _ = make_datasets(cfg, None, a.sketches)
    tmp = tempfile.mkdtemp(prefix="bench_batch_")

    def trainer(ds):
        tr = VAETrainer(cfg, ds, None, None, device=dev, save_dir=tmp, use_graph=True, log=lambda s: None,
                        compute_dtype="bf16")
        tr.save = lambda: None              # the final checkpoint write is not part of a step
        return tr

    arms = {"prefetch": trainer(train),
            "device": trainer(DeviceStrokeDataset.from_dataset(train, dev, seed=cfg.seed))}

    def run(tr, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train(num_steps=tr.step + n, log_every=10 ** 9)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for tr in arms.values():                # capture and warm-up
        run(tr, a.warmup)
    runs = {k: [] for k in arms}
    for _ in range(2):
        for k, tr in arms.items():
            runs[k].append(run(tr, a.steps))
    pf, dv = runs["prefetch"], runs["device"]
    own = abs(pf[0] - pf[1])
    diff = sum(dv) / 2 - sum(pf) / 2
    _emit(a.records, dict(part="step", preset=a.preset, sketches=len(train), steps=a.steps, warmup=a.warmup,
                          dtype="bf16", B=cfg.batch_size, Nmax=cfg.max_seq_len,
                          prefetch_ms_per_step=[t * 1e3 for t in pf], device_ms_per_step=[t * 1e3 for t in dv],
                          prefetch_own_difference_ms=own * 1e3, device_minus_prefetch_ms=diff * 1e3,
                          device_slower_than_the_bar=bool(diff > own),
                          device=torch.cuda.get_device_name(0), lib=native.hip_lib_stamp()))
    return 0


def _readme(records, a):
    lines = ["# Batch assembly on the device against the host path",
             "",
             "Written by `scripts/bench_batch.py`; every number below is in `bench_batch.jsonl`.",
             "",
             "## Per batch (B = %d, Nmax = %d, f = %.2f, prob = %.1f)" % (B, NMAX, F, PROB),
             "",
             "Host: `StrokeDataset.random_batch` + pin + host-to-device copy by the host clock, the best of %d"
             % a.rounds,
             "windows. Device: `ops.batch.assemble` into preallocated outputs, device events, the mean of %d windows"
             % a.rounds,
             "of at least %.1f s (`spread` is (max - min) / mean). The arms alternate in one process after a warm-up."
             % a.window,
             "The large corpus is the small one tiled; `permutation` is `rng.permutation(S)[:B]` alone.",
             "",
             "| sketches | host ms / batch | of which permutation ms | device ms / batch (spread) | host / device |",
             "|---|---|---|---|---|"]
    for r in records:
        if r["part"] == "batch":
            lines.append("| %d | %.3f | %.3f | %.4f (%.1f %%) | %.0f |" % (
                r["sketches"], r["host_ms"], r["host_permutation_ms"], r["device_ms"], 100 * r["device_spread"],
                r["host_over_device"]))
    lines += ["",
              "## Whole step (bf16, one captured graph, %d steps per run)" % a.steps,
              "",
              "`StrokeDataset` + prefetch thread against the device dataset, alternated prefetch, device, prefetch,",
              "device in one process after a warm-up run of each; host clock, closed by a device synchronisation.",
              "The bar: the device arm may not be slower than the prefetch arm by more than the difference between",
              "the prefetch arm's own two runs.",
              "",
              "| preset | sketches | prefetch ms / step (2 runs) | device ms / step (2 runs) | device - prefetch ms | "
              "prefetch's own difference ms | slower than the bar |",
              "|---|---|---|---|---|---|---|"]
    for r in records:
        if r["part"] == "step":
            lines.append("| %s | %d | %.3f, %.3f | %.3f, %.3f | %+.3f | %.3f | %s |" % (
                r["preset"], r["sketches"], r["prefetch_ms_per_step"][0], r["prefetch_ms_per_step"][1],
                r["device_ms_per_step"][0], r["device_ms_per_step"][1], r["device_minus_prefetch_ms"],
                r["prefetch_own_difference_ms"], "yes" if r["device_slower_than_the_bar"] else "no"))
    lines += ["",
              "Not measured: more than one GPU, a real QuickDraw pack, the assembly launch captured into the step",
              "graph, and the whole step at the large corpus (its host arm would sit behind the permutation above).",
              ""]
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "batch"))
    ap.add_argument("--sketches", type=int, default=20000)
    ap.add_argument("--large", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--part-timeout", type=int, default=420, help="seconds each part may take")
    ap.add_argument("--skip-steps", action="store_true", help="per-batch parts only")
    # a child's arguments
    ap.add_argument("--part", choices=["batch", "step"], default=None)
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--preset", default="vae_small")
    ap.add_argument("--records", default=None)
    a = ap.parse_args(argv)
    if a.part == "batch":
        return part_batch(a)
    if a.part == "step":
        return part_step(a)
    os.makedirs(a.out, exist_ok=True)
    fd, rec_path = tempfile.mkstemp(prefix="bench_batch_", suffix=".jsonl")
    os.close(fd)
    common = ["--sketches", str(a.sketches), "--rounds", str(a.rounds), "--window", str(a.window),
              "--steps", str(a.steps), "--warmup", str(a.warmup), "--records", rec_path]
    parts = [["--part", "batch"], ["--part", "batch", "--tile", str(max(1, round(a.large / a.sketches)))]]
    if not a.skip_steps:
        parts += [["--part", "step", "--preset", "vae_small"], ["--part", "step", "--preset", "vae_large"]]
    rc = 0
    for p in parts:             # one process per part, each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(a.part_timeout), sys.executable, os.path.abspath(__file__)] + p + common
        rc = subprocess.call(cmd)
        if rc != 0:
            print("part %s failed (%d): stopping" % (" ".join(p), rc), file=sys.stderr)
            break
    with open(rec_path) as f:
        records = [json.loads(line) for line in f if line.strip()]
    os.unlink(rec_path)
    with open(os.path.join(a.out, "bench_batch.jsonl"), "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(_readme(records, a))
    return rc


if __name__ == "__main__":
    sys.exit(main())
