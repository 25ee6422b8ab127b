#!/usr/bin/env python3
"""Time the RDP kernel (csrc/simplify.hip) against the host reference of the
same definition (``ops.simplify.simplify_reference``) on one GPU.

Shapes, all at epsilon = 2: the synthetic corpus at B = 1024, N = 250, and
``synthetic_raw_corpus`` at B = 1024, N = 2048 without and with ``max_len =
250``.

* **kernel**: device events around ``simplify_hip`` on resident tensors; every
  timed window follows a warm-up call and holds at least ``--window`` seconds
  of work (the repeat count comes from a calibration call); ``--rounds``
  windows, ``spread`` is (max - min) / mean over them.
* **kernel, end to end**: host clock around host tensors -> device ->
  ``simplify`` -> host, the best of three.
* **host reference**: host clock, one thread, on the first ``--ref`` sketches of
  the same batch, scaled to the batch by the count of sketches; it is what a
  user has without the kernel.
* **corpus**: ``data.quickdraw.simplify_corpus`` on ``--corpus`` raw sketches
  with ``max_len = 250`` by the host clock, against the reference on every
  ``--corpus-ref-stride``-th sketch of the same list, scaled by the count.

The rounds per sketch are the levels of the recursion the kernel reports.
Writes ``bench_simplify.jsonl`` and a ``README.md`` table into ``--out``.
Usage: ``python scripts/bench_simplify.py [--out profiles/r15/simplify]``
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "simplify"))
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per shape")
    ap.add_argument("--window", type=float, default=0.2, help="least seconds of work per timed window")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ref", type=int, default=64, help="sketches of each batch the host reference runs")
    ap.add_argument("--corpus", type=int, default=20000, help="raw sketches of the end-to-end run; 0 skips it")
    ap.add_argument("--corpus-ref-stride", type=int, default=40)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from sketch_rnn_amd.data.quickdraw import simplify_corpus
    from sketch_rnn_amd.data.synthetic import synthetic_corpus, synthetic_raw_corpus
    from sketch_rnn_amd.ops import simplify as S
    from sketch_rnn_amd.utils import native
    native.require_hip()
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    B, EPS = a.batch, 2.0

    def pad(sk, N):
        x = np.zeros((len(sk), N, 3), np.float32)
        for i, s in enumerate(sk):
            x[i, :len(s)] = s
        return torch.from_numpy(x), torch.tensor([len(s) for s in sk], dtype=torch.int64)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    raw = synthetic_raw_corpus(max(B, a.corpus), seed=0)
    shapes = [("synthetic", pad(synthetic_corpus(B, seed=0, max_len=250)[0], 250), None),
              ("raw", pad(raw[:B], 2048), None),
              ("raw_fit", pad(raw[:B], 2048), 250)]
    os.makedirs(a.out, exist_ok=True)
    common = dict(epsilon=EPS, device=torch.cuda.get_device_name(0), lib=native.hip_lib_stamp())
    records = []
    for name, (x, L), max_len in shapes:
        N = x.shape[1]
        xd, Ld = x.to(dev), L.to(dev)
        rounds = torch.zeros(B, dtype=torch.int32, device=dev)
        out, n, used = S.simplify_hip(xd, Ld, EPS, max_len, rounds=rounds)      # warm-up
        torch.cuda.synchronize()
        run = lambda: S.simplify_hip(xd, Ld, EPS, max_len)
        reps = max(1, int(math.ceil(a.window / max(timed(run, 1), 1e-7))))
        t = [timed(run, reps) for _ in range(a.rounds)]
        mean = sum(t) / len(t)
        e2e = []
        for _ in range(3):
            t0 = time.perf_counter()
            o, k, u = S.simplify(x.to(dev), L.to(dev), EPS, max_len)
            o, k, u = o.cpu(), k.cpu(), u.cpu()
            e2e.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ro, rn, ru = S.simplify_reference(x[:a.ref], L[:a.ref], EPS, max_len)
        t_ref = time.perf_counter() - t0
        same = bool(torch.equal(o[:a.ref], ro) and torch.equal(k[:a.ref], rn) and torch.equal(u[:a.ref], ru))
        points = int(L.sum())
        rec = dict(shape=name, B=B, N=N, max_len=max_len, points=points, mean_len=points / B,
                   mean_new_len=float(n.float().mean()), fitted=int((used > EPS).sum()),
                   kernel_ms=mean * 1e3, kernel_windows_s=t, reps_per_window=reps, spread=(max(t) - min(t)) / mean,
                   kernel_points_per_s=points / mean,
                   rounds_mean=float(rounds.float().mean()), rounds_max=int(rounds.max()),
                   kernel_e2e_host_clock_s=min(e2e), kernel_e2e_all_s=e2e,
                   reference_sketches=a.ref, reference_host_clock_s=t_ref, reference_threads=1,
                   reference_scaled_to_batch_s=t_ref * B / a.ref,
                   reference_points_per_s=int(L[:a.ref].sum()) / t_ref,
                   kernel_equals_reference_on_subset=same,
                   e2e_speedup_over_reference=t_ref * B / a.ref / min(e2e), **common)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.corpus:
        sk = raw[:a.corpus]
        simplify_corpus(sk[:B], EPS, 250, batch=B, device=dev)                 # warm-up
        t0 = time.perf_counter()
        out, used, dropped = simplify_corpus(sk, EPS, 250, batch=B, device=dev)
        t_k = time.perf_counter() - t0
        sub = list(range(0, len(sk), a.corpus_ref_stride))
        t0 = time.perf_counter()
        same = True
        for i in sub:       # one sketch per call: no padding to a longer neighbour
            x, L = pad([sk[i]], len(sk[i]))
            ro, rn, _ = S.simplify_reference(x, L, EPS, 250)
            same = same and np.array_equal(ro[0, :int(rn[0])].numpy(), out[i])
        t_ref = time.perf_counter() - t0
        points = int(sum(len(s) for s in sk))
        rec = dict(shape="corpus", sketches=len(sk), points=points, max_len=250, batch=B,
                   mean_new_len=float(np.mean([len(s) for s in out])), dropped=len(dropped),
                   fitted=int((used > EPS).sum()),
                   simplify_corpus_host_clock_s=t_k, simplify_corpus_points_per_s=points / t_k,
                   reference_sketches=len(sub), reference_host_clock_s=t_ref, reference_threads=1,
                   reference_scaled_to_corpus_s=t_ref * len(sk) / len(sub),
                   kernel_equals_reference_on_subset=bool(same),
                   e2e_speedup_over_reference=t_ref * len(sk) / len(sub) / t_k, **common)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    with open(os.path.join(a.out, "bench_simplify.jsonl"), "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    lines = ["# RDP simplification: kernel against the host reference",
             "",
             "Written by `scripts/bench_simplify.py`. Kernel: device events, warm-up, %d windows of at least %.1f s,"
             % (a.rounds, a.window),
             "`spread` is (max - min) / mean over them. End to end: host clock around host tensors -> device ->",
             "`simplify` -> host, the best of three. Reference: host clock, one thread, on %d sketches of the batch,"
             % a.ref,
             "scaled to the batch by the count of sketches. epsilon = 2.",
             "",
             "| shape | B | N | max_len | kernel ms (spread) | points/s | rounds mean / max | end to end s | "
             "reference s (scaled) | reference / end to end |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in records:
        if r["shape"] == "corpus":
            continue
        lines.append("| %s | %d | %d | %s | %.3f (%.1f %%) | %.3g | %.1f / %d | %.4f | %.2f | %.0f |" % (
            r["shape"], r["B"], r["N"], r["max_len"], r["kernel_ms"], 100 * r["spread"], r["kernel_points_per_s"],
            r["rounds_mean"], r["rounds_max"], r["kernel_e2e_host_clock_s"], r["reference_scaled_to_batch_s"],
            r["e2e_speedup_over_reference"]))
    for r in records:
        if r["shape"] == "corpus":
            lines += ["", "`simplify_corpus` on %d raw sketches (%d points, max_len 250, batches of %d): %.2f s by the "
                      "host clock; the reference on %d of them took %.2f s, %.0f s scaled to the list: %.0fx."
                      % (r["sketches"], r["points"], r["batch"], r["simplify_corpus_host_clock_s"],
                         r["reference_sketches"], r["reference_host_clock_s"], r["reference_scaled_to_corpus_s"],
                         r["e2e_speedup_over_reference"])]
    lines.append("")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
