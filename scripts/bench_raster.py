#!/usr/bin/env python3
"""Time the rasteriser kernels (csrc/raster.hip) against the PyTorch
transcription of the same definition (``ops.raster.rasterize_torch`` in fp32)
on one GPU.

Both arms run in one process on the same device, alternated A B A B; every
timed window is bracketed by device events, follows a warm-up call and holds
at least ``--window`` seconds of work (the repeat count comes from a
calibration call). Shapes: B in {128, 1024} x S in {64, 256}, N = 250, the
synthetic corpus; at the largest shape the kernel also runs with ``CULL`` off.

The segment-distance count of a call is ``S * S * (drawn segments of the
batch)``: what a walk over every drawn segment evaluates per pixel. It is
computed from the shapes and lengths, not measured; the culled kernel
evaluates fewer and is credited with the same count, so its rate is an
effective one.

Writes ``bench_raster.jsonl`` and a ``README.md`` table into ``--out``.
Usage: ``python scripts/bench_raster.py [--out profiles/r14/raster] [--rounds 3]``
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "raster"))
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per arm, alternated")
    ap.add_argument("--window", type=float, default=0.2, help="least seconds of work per timed window")
    ap.add_argument("--batches", default="128,1024")
    ap.add_argument("--sizes", default="64,256")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from sketch_rnn_amd.data.synthetic import synthetic_corpus
    from sketch_rnn_amd.ops import raster as R
    from sketch_rnn_amd.utils import native
    native.require_hip()
    dev = torch.device("cuda:0")
    N = 250
    R._TORCH_BUDGET = 1 << 26      # larger temporaries, fewer launches: the transcription at its best
    batches = [int(v) for v in a.batches.split(",")]
    sizes = [int(v) for v in a.sizes.split(",")]
    sk, _ = synthetic_corpus(max(batches), seed=0, max_len=N)
    x_all = np.zeros((len(sk), N, 3), np.float32)
    for i, s in enumerate(sk):
        x_all[i, :len(s)] = s
    len_all = np.asarray([len(s) for s in sk], np.int64)
    # drawn segments: 1 <= t < L with lift[t-1] < 0.5
    drawn_all = np.asarray([int((s[:len(s) - 1, 2] < 0.5).sum()) if len(s) > 1 else 0 for s in sk], np.int64)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    def arm_kernel(x, L, S, out, cull):
        def run():
            R.CULL = cull
            R.rasterize_hip(x, L, size=S, out=out)
        return run

    def arm_torch(x, L, S, out):
        return lambda: R.rasterize_torch(x, L, size=S, out=out, dtype=torch.float32)

    os.makedirs(a.out, exist_ok=True)
    records = []
    for B in batches:
        x = torch.as_tensor(x_all[:B], device=dev)
        L = torch.as_tensor(len_all[:B], device=dev)
        for S in sizes:
            out_k = torch.empty(B, S, S, device=dev)
            out_t = torch.empty(B, S, S, device=dev)
            arms = {"kernel": arm_kernel(x, L, S, out_k, True), "torch_fp32": arm_torch(x, L, S, out_t)}
            if B == max(batches) and S == max(sizes):
                arms["kernel_nocull"] = arm_kernel(x, L, S, out_k, False)
            evals = int(S) * int(S) * int(drawn_all[:B].sum())
            reps, times = {}, {k: [] for k in arms}
            for k, fn in arms.items():       # warm-up, then a calibration call
                fn()
                torch.cuda.synchronize()
                reps[k] = max(1, int(math.ceil(a.window / max(timed(fn, 1), 1e-7))))
            for _ in range(a.rounds):        # A B (C) A B (C) ...
                for k, fn in arms.items():
                    times[k].append(timed(fn, reps[k]))
            R.CULL = True
            err = float((out_k - out_t).abs().max())
            for k in arms:
                t = times[k]
                mean = sum(t) / len(t)
                records.append(dict(arm=k, B=B, N=N, S=S, width=1.0, reps_per_window=reps[k], windows_s=t,
                                    mean_s=mean, spread=(max(t) - min(t)) / mean, segment_distance_evals=evals,
                                    evals_per_s=evals / mean, mean_drawn_segments=float(drawn_all[:B].mean()),
                                    max_abs_diff_kernel_vs_torch=err,
                                    device=torch.cuda.get_device_name(0), lib=native.hip_lib_stamp()))
                print(json.dumps(records[-1]), flush=True)
    with open(os.path.join(a.out, "bench_raster.jsonl"), "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    by = {(r["arm"], r["B"], r["S"]): r for r in records}
    lines = ["# Rasteriser: kernel against the PyTorch transcription",
             "",
             "Written by `scripts/bench_raster.py` (device events, warm-up, windows of at least %.1f s, arms alternated"
             % a.window,
             "in one process, %d windows per arm). N = 250, width 1, the synthetic corpus. `spread` is" % a.rounds,
             "(max - min) / mean over the windows of one arm. `evals/s` credits every arm with",
             "S * S * (drawn segments of the batch) point-segment distances per call, computed from the shapes.",
             "",
             "| B | S | kernel ms (spread) | torch fp32 ms (spread) | torch / kernel | kernel evals/s | verdict |",
             "|---|---|---|---|---|---|---|"]
    for B in batches:
        for S in sizes:
            k, t = by[("kernel", B, S)], by[("torch_fp32", B, S)]
            ratio = t["mean_s"] / k["mean_s"]
            lines.append("| %d | %d | %.4f (%.1f %%) | %.3f (%.1f %%) | %.1f | %.3g | %s |" % (
                B, S, k["mean_s"] * 1e3, 100 * k["spread"], t["mean_s"] * 1e3, 100 * t["spread"], ratio,
                k["evals_per_s"], "the kernel is faster" if ratio > 1 else "the kernel does NOT beat the transcription"))
    nc = by.get(("kernel_nocull", max(batches), max(sizes)))
    if nc:
        k = by[("kernel", max(batches), max(sizes))]
        lines += ["", "`CULL = False` at B = %d, S = %d: %.4f ms (spread %.1f %%), %.3g evals/s actually evaluated; "
                  "culling is worth %.2fx." % (nc["B"], nc["S"], nc["mean_s"] * 1e3, 100 * nc["spread"],
                                               nc["evals_per_s"], nc["mean_s"] / k["mean_s"])]
    lines += ["", "Largest |kernel - torch fp32| over all shapes: %.3g." % max(
        r["max_abs_diff_kernel_vs_torch"] for r in records), ""]
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
