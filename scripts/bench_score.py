#!/usr/bin/env python3
"""Per-sketch scoring against the scalar evaluation loop, on one GPU.

For each preset (synthetic test split, bf16, the preset's batch size) the
same batches go through

* A: ``VAETrainer.evaluate`` -- ``loss(train=False)`` over every padded row,
  one host read per scalar;
* B: ``VAETrainer.evaluate_sketches`` -- ``SketchVAE.score`` decoded up to
  each batch's longest sketch, the fused score kernel, one copy per batch;

alternating A B A B ... in one process (wall time around a device
synchronise, ms per batch, median over the repeats). The head alone is timed
on one full-length batch of decoder outputs with device events over
``--calls`` back-to-back calls: ``ops.mdn_head_score`` (csrc/mdn_score.hip +
its finish kernel) against the ``gemm.linear`` + ``ops.mdn_loss`` pair that
evaluation runs under ``no_grad``. One JSON line per preset goes to ``--out``.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="vae_large,vae_small")
    ap.add_argument("--synthetic", type=int, default=4000)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default="profiles/r9/score/score_bench.jsonl")
    a = ap.parse_args()
    import numpy as np
    import torch
    from sketch_rnn_amd import ops
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.config import PRESETS
    from sketch_rnn_amd.ops import gemm
    from sketch_rnn_amd.train.trainer import VAETrainer
    from sketch_rnn_amd.utils import native
    cuda = a.device.startswith("cuda")

    def sync():
        if cuda:
            torch.cuda.synchronize()

    def wall(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for name in a.presets.split(","):
            # evaluation-mode config: loss(train=False) then masks the pen term as the score does
            cfg = dataclasses.replace(PRESETS[name], is_training=False)
            (train, valid, test), _ = make_datasets(cfg, None, a.synthetic)
            tr = VAETrainer(cfg, train, valid, test, device=a.device, use_graph=False, compute_dtype=a.dtype,
                            log=lambda s: None)
            tr.model.eval()
            nb = test.num_batches
            for _ in range(2):   # warm-up: every batch shape of both arms
                tr.evaluate(test)
                tr.evaluate_sketches(test)
            ta, tb = [], []
            for _ in range(a.reps):
                ms, ev = wall(lambda: tr.evaluate(test))
                ta.append(ms / nb)
                ms, sk = wall(lambda: tr.evaluate_sketches(test))
                tb.append(ms / nb)
            lens = np.concatenate([test.get_batch(b)[1] for b in range(nb)])
            # the two arms agree on the number they share: r_cost of evaluate (its own eps) is a
            # mean over Nmax * B rows; evaluate_sketches scores at z = mu, so only unconditional models match exactly
            rec = {"preset": name, "dtype": a.dtype, "batch_size": cfg.batch_size, "batches": nb,
                   "sketches": int(len(lens)), "max_seq_len": cfg.max_seq_len,
                   "real_row_fraction": float(lens.sum()) / (len(lens) * cfg.max_seq_len),
                   "longest_per_batch": [int(test.get_batch(b)[1].max()) for b in range(nb)],
                   "evaluate_ms_per_batch": statistics.median(ta), "evaluate_ms_all": ta,
                   "evaluate_sketches_ms_per_batch": statistics.median(tb), "evaluate_sketches_ms_all": tb,
                   "evaluate_r_cost": ev["r_cost"],
                   "sketches_nll_per_padded_row": float(sk["nll"].sum()) / (len(lens) * cfg.max_seq_len),
                   "lib": native.hip_lib_stamp() if cuda else None}
            if cuda:
                m = tr.model
                s, l, c = tr.batch_to_device(test.get_batch(nb - 1))
                with torch.no_grad():
                    sT = s.transpose(0, 1).contiguous()
                    T, B = sT.shape[0] - 1, sT.shape[1]
                    out = torch.randn(T, B, cfg.dec_rnn_size, device=a.device) * 0.5
                    lp = out.to(torch.bfloat16)
                    tgt = sT[1:]
                    Tc = int(l.max())

                    def pair():
                        z = gemm.linear(out.reshape(-1, out.shape[-1]), m.output_w, m.output_b)
                        return ops.mdn_loss(z, tgt.reshape(-1, 5), cfg.num_mixture, mode="magenta", is_training=False)

                    variants = {
                        "linear_plus_mdn_loss_full": pair,
                        "score_full_fp32_rows": lambda: ops.mdn_head_score(out, m.output_w, m.output_b, tgt, l,
                                                                           cfg.num_mixture),
                        "score_full_bf16_rows": lambda: ops.mdn_head_score(out, m.output_w, m.output_b, tgt, l,
                                                                           cfg.num_mixture, x_lp=lp),
                        "score_trimmed_bf16_rows": lambda: ops.mdn_head_score(out[:Tc], m.output_w, m.output_b,
                                                                              tgt[:Tc], l, cfg.num_mixture,
                                                                              x_lp=lp[:Tc]),
                    }
                    head = {}
                    for _ in range(2):      # alternate the variants, keep each one's best repeat
                        for k, fn in variants.items():
                            for _ in range(5):
                                fn()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            torch.cuda.synchronize()
                            e0.record()
                            for _ in range(a.calls):
                                fn()
                            e1.record()
                            torch.cuda.synchronize()
                            head.setdefault(k, []).append(e0.elapsed_time(e1) / a.calls)
                rec["head_call_ms"] = {k: min(v) for k, v in head.items()}
                rec["head_call_ms_all"] = head
                rec["head_shape"] = {"T": T, "B": B, "Hd": cfg.dec_rnn_size, "M": cfg.num_mixture, "T_trimmed": Tc}
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec))
            del tr
    return 0


if __name__ == "__main__":
    sys.exit(main())
