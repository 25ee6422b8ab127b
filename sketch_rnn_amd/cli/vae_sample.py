"""``python -m sketch_rnn_amd.cli.vae_sample`` -- generate from a trained VAE.

Modes: ``random`` (z ~ N(0, I), or the unconditional decoder), ``class``
(class-conditional z for ``--label``), ``interpolate`` (spherical
interpolation between two random latents), and two modes that read
sketches from a dataset (``--data`` / ``--synthetic`` / ``--split`` as in
``cli.vae_eval``, ``--offset`` for the first sketch):

* ``reconstruct`` -- encode each of ``--n`` sketches and decode it again:
  ``z`` is the encoder's ``mu`` (``--sample_z``: ``mu + sigma * eps``), the
  class label is the sketch's. The grid holds each original followed by its
  reconstruction. Needs a conditional model.
* ``complete`` -- feed the first ``ceil(prefix_frac * len)`` strokes of each
  sketch (at most ``len - 1``) to the decoder and let it finish the drawing,
  ``--completions K`` times per sketch. ``--z_from`` picks the latent of a
  conditional model: the encoded ``prefix`` (default), the encoded ``full``
  sketch, or the ``prior``. The grid holds each prefix followed by its K
  completions.

``--temperatures 0.1,0.4,0.7,1.0`` (modes ``random``, ``class`` and
``reconstruct``) decodes each of the ``--n`` latents once per listed
temperature, all in one batch with a temperature per row, and lays the grid
out with one line per latent and the temperatures as its columns (after the
original in ``reconstruct``).

``--mode bulk --n J --slots S [--chunk C] --out_pack FILE`` generates J
sketches from latents drawn as in ``random`` and writes them as a sketch
pack (``data.quickdraw.save_pack``, split ``train``, stroke-3 in model units
cut at each decoded length) instead of a grid. It decodes through
``sample.stream.StreamDecoder``: S decoder rows, a finished row taking the
next latent instead of padding until the longest sketch of its batch ends
(on a GPU with the four-launch HyperLSTM stroke; blocks of S through the
graph decoder elsewhere; the recycling path is bf16, so on a GPU bulk mode
computes in bf16 unless ``--dtype fp32`` is given). Super-batches of at most 16384 sketches bound the
memory. Prints one JSON line: ``steps_run``, ``slot_steps``,
``valid_strokes``, ``occupancy`` (valid strokes per computed row-step).

Writes a stroke-3 SVG grid. ``--png PATH`` writes the same grid (the same
sketches, order and columns) as a PNG of ``--png_size`` pixels per sketch,
rasterised on the model's device by ``ops.raster.rasterize``. ``--mode
reconstruct --raster_iou`` rasterises each original in its fitted frame and
its reconstructions in that same frame, prints the mean
``render.raster.soft_iou`` per decoded column and writes the per-sketch
values to ``<out>.iou.json``; with ``--device_sampler`` on a GPU the decoded
``[rows, N, 5]`` tensor is rasterised where it lies.
``--device_sampler`` decodes the whole grid in parallel through the
HIP-graph decoder; with ``--fused`` a plain ``lstm`` or ``layer_norm``
decoder of size 256 or 512 runs through its whole-sketch kernel
(``sample.fused.fused_vae_decoder``) instead, and anything those do not take
falls back to the graph decoder. The two dataset modes run on the host
sampler, the graph decoder (``--device_sampler``, on any device) and the
whole-sketch kernels alike.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np


BULK_SUPER = 16384     # --mode bulk: jobs per StreamDecoder.run (the per-job constants are held for a whole run)


def slerp(p0, p1, t):
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    omega = np.arccos(np.clip(np.dot(p0 / np.linalg.norm(p0), p1 / np.linalg.norm(p1)), -1, 1))
    so = np.sin(omega)
    if so < 1e-8:
        return (1.0 - t) * p0 + t * p1
    return np.sin((1.0 - t) * omega) / so * p0 + np.sin(t * omega) / so * p1


def _bulk(a, model, cfg, zs, labels, device, dtype) -> int:
    """``--mode bulk``: the latents through StreamDecoder in super-batches, the pack, the JSON line."""
    import json
    import torch
    from ..data.quickdraw import save_pack
    from ..data.strokes import to_normal_strokes
    from ..sample.stream import StreamDecoder
    dec = StreamDecoder(model, a.slots, cfg.max_seq_len, a.temperature, a.greedy, chunk=a.chunk)
    total = {"steps_run": 0, "slot_steps": 0, "valid_strokes": 0}
    sketches = []
    for j0 in range(0, a.n, BULK_SUPER):
        zt = torch.as_tensor(zs[j0:j0 + BULK_SUPER], dtype=torch.float32, device=device)
        s, lens = dec.run(zt, labels=torch.as_tensor(labels[j0:j0 + BULK_SUPER], device=device), seed=a.seed,
                          first_row=j0)
        s, lens = s.cpu().numpy(), lens.cpu().numpy()
        sketches.extend(to_normal_strokes(x[:n]) for x, n in zip(s, lens))
        for k in total:
            total[k] += getattr(dec, k)
    save_pack(a.out_pack, {"train": (sketches, labels)})
    total["occupancy"] = total["valid_strokes"] / total["slot_steps"] if total["slot_steps"] else 0.0
    print(json.dumps(dict(mode="bulk", impl=dec.impl, dtype=dtype, n=a.n, slots=a.slots, chunk=dec.chunk, **total)))
    return 0


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--save_dir", default="save/vae")
    p.add_argument("--out", default="vae_samples.svg")
    p.add_argument("--mode", choices=["random", "class", "interpolate", "reconstruct", "complete", "bulk"],
                   default="random")
    p.add_argument("--n", type=int, default=10)
    p.add_argument("--label", type=int, default=0)
    p.add_argument("--temperature", type=float, default=0.5)
    p.add_argument("--temperatures", default=None,
                   help="random / class / reconstruct: comma-separated temperatures; every latent is decoded once "
                        "per value in one batch, one grid line per latent (replaces --temperature)")
    p.add_argument("--greedy", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default=None)
    p.add_argument("--device_sampler", action="store_true")
    p.add_argument("--fp8", action="store_true",
                   help="device sampler: h W_h of the HyperLSTM decoder as an MX-fp8 GEMM (BASELINE config 5; "
                        "pays at >= 1024 sketches per call)")
    p.add_argument("--fused", action="store_true",
                   help="device sampler: decode plain lstm and layer_norm decoders (size 256 with <= 32 mixtures, 512 "
                        "with <= 20) with their whole-sketch kernel instead of the graph decoder (needs "
                        "--device_sampler). Measured on vae_small (lstm): faster than the graph decoder for --n 1 to "
                        "672 (2.7x at 128), slower at 1024. Measured on vae_layernorm: faster for --n 1, 128 (1.9x) "
                        "and 448 (1.05x), slower at 1024 (0.55x); one launch takes 224 rows at size 512 and larger "
                        "grids run as successive launches, so expect it to lose from 3 launches (--n > 448) on")
    p.add_argument("--data", default=None, help="reconstruct / complete: sketch pack (.npz) with train/valid/test "
                                                "splits")
    p.add_argument("--synthetic", type=int, default=0, help="reconstruct / complete: synthetic corpus of this size")
    p.add_argument("--split", choices=["test", "valid"], default="test")
    p.add_argument("--offset", type=int, default=0, help="reconstruct / complete: index of the first sketch")
    p.add_argument("--sample_z", action="store_true",
                   help="encoded latents are mu + sigma * eps instead of mu")
    p.add_argument("--prefix_frac", type=float, default=0.5,
                   help="complete: the share of each sketch's strokes given to the decoder")
    p.add_argument("--completions", type=int, default=1, help="complete: endings generated per prefix")
    p.add_argument("--z_from", choices=["prefix", "full", "prior"], default="prefix",
                   help="complete: latent of a conditional model (encode the prefix, the whole sketch, or draw it)")
    p.add_argument("--png", default=None, metavar="PATH",
                   help="also write the grid as a PNG: the same sketches in the same order and columns as the SVG, "
                        "rasterised on the model's device")
    p.add_argument("--png_size", type=int, default=64, help="--png / --raster_iou: pixels per sketch edge")
    p.add_argument("--png_width", type=float, default=1.0, help="--png / --raster_iou: stroke width in pixels")
    p.add_argument("--raster_iou", action="store_true",
                   help="reconstruct: rasterise each original in its fitted frame and its reconstructions in the "
                        "same frame, print the mean soft IoU per decoded column and write the per-sketch values "
                        "to <out>.iou.json")
    p.add_argument("--slots", type=int, default=128, help="bulk: decoder rows kept busy")
    p.add_argument("--chunk", type=int, default=None, help="bulk: decode steps between two refills of finished rows")
    p.add_argument("--out_pack", default=None, metavar="FILE", help="bulk: the sketch pack (.npz) to write")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default=None,
                   help="bulk: compute dtype of the decode (default bf16 on a GPU, where the recycling path of "
                        "StreamDecoder needs it; fp32 elsewhere)")
    a = p.parse_args(argv)
    if a.mode == "bulk":
        if not a.out_pack:
            p.error("--mode bulk needs --out_pack")
        if a.n < 0 or a.slots < 1 or (a.chunk is not None and a.chunk < 1):
            p.error("--mode bulk needs --n >= 0, --slots >= 1 and --chunk >= 1")
        if a.temperatures is not None or a.fused or a.fp8 or a.png or a.raster_iou:
            p.error("--mode bulk takes none of --temperatures, --fused, --fp8, --png, --raster_iou")
    if a.fused and not a.device_sampler:
        p.error("--fused needs --device_sampler")
    if a.raster_iou and a.mode != "reconstruct":
        p.error("--raster_iou works in the mode reconstruct")
    if (a.png or a.raster_iou) and not (1 <= a.png_size <= 512 and math.isfinite(a.png_width) and a.png_width > 0
                                        and a.png_size > 4):
        p.error("--png_size must be in 5..512 and --png_width greater than 0")
    from_data = a.mode in ("reconstruct", "complete")
    temps = None
    if a.temperatures is not None:
        if a.mode not in ("random", "class", "reconstruct"):
            p.error("--temperatures works in the modes random, class and reconstruct")
        try:
            temps = [float(t) for t in a.temperatures.split(",")]
        except ValueError:
            p.error("--temperatures must be comma-separated numbers")
        if not all(math.isfinite(t) and t > 0 for t in temps):
            p.error("--temperatures must be finite and greater than 0")
    if a.mode == "complete" and (a.completions < 1 or not 0.0 <= a.prefix_frac <= 1.0):
        p.error("--completions must be >= 1 and --prefix_frac in [0, 1]")
    import torch
    from ..ckpt import checkpoint as ckpt
    from ..config import load_json
    from ..data.strokes import to_normal_strokes
    from ..models.vae import SketchVAE
    from ..render.svg import grid_strokes3
    from ..sample.sampler import GraphDecoder, sample_vae
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    cfg = load_json(os.path.join(a.save_dir, "config.json"))
    model = SketchVAE(cfg).to(device)
    path = ckpt.latest_checkpoint(a.save_dir)
    if path:
        ckpt.load_checkpoint(path, model)
    model.eval()
    rng = np.random.RandomState(a.seed)
    zs = rng.randn(a.n, cfg.z_size)
    if a.mode == "interpolate":
        z0, z1 = rng.randn(cfg.z_size), rng.randn(cfg.z_size)
        zs = np.stack([slerp(z0, z1, t) for t in np.linspace(0, 1, a.n)])
    labels = np.full(a.n, a.label if a.mode == "class" else 0)
    N = cfg.max_seq_len
    if a.mode == "bulk":
        from .. import ops
        # the recycling path is the bf16 four-launch stroke: a GPU run takes bf16 unless told otherwise
        dtype, saved = a.dtype or ("bf16" if device.startswith("cuda") else "fp32"), ops.get_compute_dtype()
        ops.set_compute_dtype(dtype)
        try:
            return _bulk(a, model, cfg, zs, labels, device, dtype)
        finally:
            ops.set_compute_dtype(saved)
    prefix = plen = shown = None      # complete: [rows, P, 5] stroke-5 prefixes and their lengths; shown: data sketches
    group = 1                         # decoded sketches per shown one
    if from_data:
        from ..data.strokes import pad_batch_magenta
        from .vae_eval import load_split
        if a.mode == "reconstruct" and not cfg.conditional:
            print("--mode reconstruct needs a conditional model (an encoder and a latent)", file=sys.stderr)
            return 2
        ds, _ = load_split(cfg, a.data, a.synthetic, a.split, a.save_dir)
        if ds is None or len(ds) < a.offset + a.n or a.offset < 0:
            print("the %s split has no sketches [%d, %d)" % (a.split, a.offset, a.offset + a.n), file=sys.stderr)
            return 1
        data = [np.asarray(x, np.float32) for x in ds.strokes[a.offset:a.offset + a.n]]
        labels = np.asarray(ds.labels[a.offset:a.offset + a.n], dtype=np.int64)

        def encode(sk):
            """Latents of stroke-3 sketches: mu, or mu + sigma * eps with --sample_z."""
            x = torch.as_tensor(pad_batch_magenta(sk, N), device=device)
            lens = torch.as_tensor([len(x_) for x_ in sk], dtype=torch.int64, device=device)
            with torch.no_grad():
                mu, presig = (t.float().cpu().numpy() for t in model.encode(x, lens))
            return mu + np.exp(presig / 2.0) * rng.randn(*mu.shape) if a.sample_z else mu

        shown = data
        if a.mode == "reconstruct":
            zs = encode(data)
        else:
            group = a.completions
            k = [min(int(math.ceil(a.prefix_frac * len(x))), len(x) - 1) for x in data]
            shown = [x[:k_] for x, k_ in zip(data, k)]
            P = max(max(k), 1)
            pre = pad_batch_magenta(shown, P)[:, 1:]        # stroke-5 rows (no start token), padded past each length
            if cfg.conditional and a.z_from != "prior":
                # a prefix of no strokes has nothing to encode: its latent is the prior mean
                src = data if a.z_from == "full" else [x if len(x) else np.zeros((1, 3), np.float32) for x in shown]
                zs = encode(src)
                if a.z_from == "prefix":
                    zs[[i for i, k_ in enumerate(k) if k_ == 0]] = 0.0
            zs = np.repeat(zs, group, axis=0)
            if a.z_from == "prior":
                zs = rng.randn(a.n * group, cfg.z_size)
            labels = np.repeat(labels, group)
            prefix, plen = np.repeat(pre, group, axis=0), np.repeat(np.asarray(k, np.int64), group)
    row_temps = None                  # --temperatures: row i * K + j decodes latent i at temperature j
    if temps is not None:
        group = len(temps)
        zs, labels = np.repeat(zs, group, axis=0), np.repeat(labels, group)
        row_temps = np.tile(np.asarray(temps, np.float64), a.n)
    rows = len(labels)
    sketches = []
    s_dev = None                      # the decoded [rows, N, 5] tensor where a GPU device sampler left it
    if a.fused and not device.startswith("cuda"):
        print("--fused: no GPU device, sampling on the host")
    if a.device_sampler and (device.startswith("cuda") or from_data or temps is not None):
        zt, lt = torch.as_tensor(zs, dtype=torch.float32, device=device), torch.as_tensor(labels, device=device)
        pre_kw = {}
        if prefix is not None:
            pre_kw = dict(prefix=torch.as_tensor(prefix, device=device), prefix_len=torch.as_tensor(plen, device=device))
        if row_temps is not None:
            pre_kw.update(temperature=torch.as_tensor(row_temps, device=device))
        s = None
        if not device.startswith("cuda"):
            a.fused = False
        if a.fused:
            from ..sample.fused import NotCoResident, fused_vae_decoder
            try:
                s, _ = fused_vae_decoder(model, rows, cfg.max_seq_len, a.temperature, a.greedy).run(
                    seed=a.seed, z=zt, labels=lt, **pre_kw)
            except ValueError:
                print("--fused: needs an lstm or layer_norm decoder of size 256 (<= 32 mixtures) or 512 (<= 20); "
                      "using the graph decoder")
            except NotCoResident as e:
                print("--fused: %s; using the graph decoder" % e)
        if s is None:
            dec = GraphDecoder(model, rows, cfg.max_seq_len, a.temperature, a.greedy, fp8=a.fp8)
            s, _ = dec.run(seed=a.seed, z=zt, labels=lt, **pre_kw)
        sketches = [to_normal_strokes(x) for x in s.cpu().numpy()]
        if device.startswith("cuda"):
            s_dev = s
    else:
        for k in range(rows):
            z = torch.as_tensor(zs[k:k + 1], dtype=torch.float32, device=device)
            pre_k = None if prefix is None else prefix[k, :plen[k]]
            temp_k = a.temperature if row_temps is None else float(row_temps[k])
            s5, _ = sample_vae(model, cfg.max_seq_len, temp_k, a.greedy, z=z, label=int(labels[k]), rng=rng,
                               prefix=pre_k)
            sketches.append(to_normal_strokes(s5))
    def batch3(sk):
        """Stroke-3 lists padded into one [n, N, 3] batch on the model's device, with their lengths."""
        x = np.zeros((len(sk), max([len(x_) for x_ in sk] + [1]), 3), np.float32)
        for i, x_ in enumerate(sk):
            x[i, :len(x_)] = x_
        return (torch.as_tensor(x, device=device),
                torch.as_tensor([len(x_) for x_ in sk], dtype=torch.int64, device=device))

    if a.raster_iou:
        import json
        from ..ops.raster import rasterize
        from ..render.raster import soft_iou
        orig, frame = rasterize(*batch3(shown), size=a.png_size, width=a.png_width)
        frame = frame.repeat_interleave(group, dim=0)
        if s_dev is not None:   # the decoder's output where it lies: no host round trip
            dec, _ = rasterize(s_dev.float(), None, size=a.png_size, width=a.png_width, frame=frame)
        else:
            dec, _ = rasterize(*batch3(sketches), size=a.png_size, width=a.png_width, frame=frame)
        iou = soft_iou(orig.repeat_interleave(group, dim=0), dec).view(a.n, group).cpu()
        cols = temps if temps is not None else [a.temperature]
        print("raster IoU (%d sketches, %d px): %s" % (a.n, a.png_size, "  ".join(
            "T=%g %.4f" % (t, m) for t, m in zip(cols, iou.mean(0).tolist()))))
        with open(a.out + ".iou.json", "w") as f:
            json.dump({"size": a.png_size, "width": a.png_width, "temperatures": cols,
                       "mean": iou.mean(0).tolist(), "iou": iou.tolist()}, f)
    if shown is not None:       # each data sketch (or its prefix) followed by what was decoded from it
        sketches = [x for i, d in enumerate(shown) for x in [d] + sketches[i * group:(i + 1) * group]]
    maxcol = len(sketches) // a.n if temps is not None else 5      # --temperatures: one line per latent
    if temps is not None:
        grid_strokes3(sketches, a.out, maxcol=maxcol)
    else:
        grid_strokes3(sketches, a.out)
    if a.png:
        from ..ops.raster import rasterize
        from ..render.png import grid_png
        images, _ = rasterize(*batch3(sketches), size=a.png_size, width=a.png_width)
        grid_png(images, a.png, maxcol=maxcol)
        print("wrote %s (%d sketches, %d px each)" % (a.png, len(sketches), a.png_size))
    print("wrote %s (%d sketches)" % (a.out, len(sketches)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
