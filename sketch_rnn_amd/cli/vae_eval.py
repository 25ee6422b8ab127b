"""``python -m sketch_rnn_amd.cli.vae_eval`` -- per-sketch likelihood of a
trained VAE on a held-out split, and the paired comparison of two checkpoints.

``--save_dir A`` is scored on the ``test`` (or ``valid``) split of ``--data``
/ ``--synthetic N``, built as ``cli.vae_train`` builds it and normalised by
the scale stored in ``A/data.json`` when present. Prints the number of
sketches and the NLL per sketch and per point with standard errors; with
``--samples K`` also the K-sample ELBO and the IWAE-K bound. ``--out`` gets
the per-sketch arrays (``.npz``).

``--compare_dir B`` scores B on the same sketches with the same noise and
prints the paired mean difference (B - A) of the NLL per point with its
normal-approximation 95 % interval ``mean +- 1.96 sd / sqrt(n)``, absolute
and relative to A: the interval shrinks with the number of sketches, so it
resolves differences that unpaired per-seed means cannot. B's arrays go
into the ``.npz`` with a ``b_`` prefix.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def load_split(cfg, data_path, synthetic, split, save_dir):
    """``(dataset, scale)``: the split as ``cli.vae_train.make_datasets``
    builds it, normalised by ``save_dir/data.json``'s scale when that file
    exists (else by the scale recomputed from the training split)."""
    from ..data.dataset import StrokeDataset
    from .vae_train import make_datasets
    scale = None
    path = os.path.join(save_dir, "data.json")
    if os.path.exists(path):
        with open(path) as f:
            scale = json.load(f).get("scale_factor")
    if scale is None:
        (_, valid, test), scale = make_datasets(cfg, data_path, synthetic)
        return {"valid": valid, "test": test}[split], scale
    if data_path:
        from ..data.quickdraw import load_pack
        splits = load_pack(data_path)
        if split not in splits:
            return None, scale
        s, l = splits[split]
    else:
        from ..data.synthetic import synthetic_corpus
        n = synthetic or 2000
        s, l = synthetic_corpus(n, seed=cfg.seed, max_len=cfg.max_seq_len, n_classes=max(cfg.num_classes, 1))
        k = max(n // 10, cfg.batch_size)   # make_datasets: valid = [:k], test = [k:2k]
        lo = 0 if split == "valid" else k
        s, l = s[lo:lo + k], l[lo:lo + k]
    ds = StrokeDataset(s, cfg.batch_size, cfg.max_seq_len, labels=l)
    ds.normalize(scale)
    return ds, scale


def mean_se(x):
    x = np.asarray(x, np.float64)
    return float(x.mean()), (float(x.std(ddof=1) / np.sqrt(len(x))) if len(x) > 1 else 0.0)


def score_dir(save_dir, dataset, a, device):
    from ..ckpt import checkpoint as ckpt
    from ..config import load_json
    from ..train.trainer import VAETrainer
    cfg = load_json(os.path.join(save_dir, "config.json"))
    tr = VAETrainer(cfg, None, None, dataset, device=device, save_dir=save_dir, use_graph=False,
                    compute_dtype=a.dtype, log=lambda s: None)
    path = ckpt.latest_checkpoint(save_dir)
    if path:
        ckpt.load_checkpoint(path, tr.model)
    tr.model.eval()
    return tr.evaluate_sketches(dataset, max_batches=a.max_batches, samples=a.samples, seed=a.seed)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="per-sketch likelihood scores of a trained sketch-rnn VAE")
    p.add_argument("--save_dir", default="save/vae")
    p.add_argument("--compare_dir", default=None, help="second checkpoint, scored on the same sketches and noise")
    p.add_argument("--data", default=None, help="sketch pack (.npz) with train/valid/test splits")
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--split", choices=["test", "valid"], default="test")
    p.add_argument("--samples", type=int, default=0, help="K >= 1: K-sample ELBO and IWAE-K (conditional models)")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--device", default=None)
    p.add_argument("--max_batches", type=int, default=None)
    p.add_argument("--out", default="scores.npz")
    a = p.parse_args(argv)
    import torch
    from ..config import load_json
    from ..parallel import dp
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    cfg = load_json(os.path.join(a.save_dir, "config.json"))
    dataset, scale = load_split(cfg, a.data, a.synthetic, a.split, a.save_dir)
    if dataset is None or dataset.num_batches == 0:
        print("no full batch in the %s split" % a.split)
        return 1
    res = score_dir(a.save_dir, dataset, a, device)
    n = len(res["nll"])
    pts = np.maximum(res["points"], 1)
    lines = ["%d sketches (%s split, scale %.6g, %d points)" % (n, a.split, scale, int(res["points"].sum())),
             "NLL per sketch %.4f +- %.4f" % mean_se(res["nll"]),
             "NLL per point  %.5f +- %.5f" % mean_se(res["nll"] / pts)]
    if a.samples >= 1:
        lines.append("ELBO (K=%d) %.4f +- %.4f" % ((a.samples,) + mean_se(res["elbo"])))
        lines.append("IWAE-%d %.4f +- %.4f" % ((a.samples,) + mean_se(res["iwae"])))
    arrays = dict(res)
    if a.compare_dir:
        other = score_dir(a.compare_dir, dataset, a, device)
        arrays.update({"b_" + k: v for k, v in other.items()})
        pa, pb = res["nll"] / pts, other["nll"] / pts
        m, se = mean_se(pb - pa)
        base = float(pa.mean())
        lines.append("B: NLL per point %.5f +- %.5f" % mean_se(pb))
        lines.append("paired difference B - A of NLL per point: %+.6f +- %.6f (95%%)" % (m, 1.96 * se))
        lines.append("relative to A: %+.4f %% +- %.4f %%" % (100.0 * m / base, 100.0 * 1.96 * se / abs(base)))
    if dp.rank() == 0:
        for line in lines:
            print(line)
        if a.out:
            np.savez(a.out, **arrays)
            print("wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
