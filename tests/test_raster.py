"""The rasteriser on the CPU: the PyTorch transcription of the definition
(``ops.raster.rasterize_torch``) against hand-computed images, its select on
``lengths``, stroke-5 input, frames, argument validation; the PNG writer parsed
by hand; ``vae_sample --png`` and ``--raster_iou`` end to end."""
import dataclasses
import json
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.data.strokes import to_big_strokes
from sketch_rnn_amd.data.synthetic import synthetic_corpus
from sketch_rnn_amd.ops import raster as R
from sketch_rnn_amd.render import png as P
from sketch_rnn_amd.render.raster import soft_iou, to_uint8

ROWS = [[2.0, 2.5, 0.0], [4.0, 0.0, 1.0]]
UNIT = torch.tensor([[1.0, 0.0, 0.0]])


def _hand(rows=ROWS, L=2, **kw):
    return R.rasterize_torch(torch.tensor([rows]), torch.tensor([L]), size=8, width=1.0, **kw)


def test_hand_computed_image():
    img, frame = _hand(frame=UNIT)
    want = torch.zeros(8, 8, dtype=torch.float64)
    want[2] = torch.tensor([0, .5, 1, 1, 1, 1, .5, 0])
    assert img.dtype == torch.float64 and img.shape == (1, 8, 8)
    assert float((img[0] - want).abs().max()) <= 1e-6
    assert torch.equal(frame, UNIT.double())
    img32, _ = R.rasterize(torch.tensor([ROWS]), torch.tensor([2]), size=8, width=1.0, frame=UNIT)
    assert img32.dtype == torch.float32 and float((img32[0].double() - want).abs().max()) <= 1e-6


def test_pen_rule_and_short_lengths():
    lifted = [[2.0, 2.5, 1.0], [4.0, 0.0, 1.0]]
    assert float(_hand(lifted, frame=UNIT)[0].abs().max()) == 0.0      # lift[0] = 1: the only segment is a move
    assert float(_hand(L=1, frame=UNIT)[0].abs().max()) == 0.0         # the origin move is never drawn
    assert float(_hand(L=1)[0].abs().max()) == 0.0
    img, frame = _hand(L=0)
    assert float(img.abs().max()) == 0.0
    assert torch.equal(frame, torch.tensor([[1.0, 4.0, 4.0]], dtype=torch.float64))


def test_zero_length_segment_is_a_dot():
    # box (0, 0) .. (2, 0): scale 2, centre at (4, 4); the dot lands on the pixel corner (6, 4)
    img, frame = _hand([[2.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert torch.allclose(frame, torch.tensor([[2.0, 2.0, 4.0]], dtype=torch.float64))
    want = torch.zeros(8, 8, dtype=torch.float64)
    want[3:5, 5:7] = 1.0 - math.sqrt(0.5)
    assert float((img[0] - want).abs().max()) <= 1e-12
    assert abs(float(img.sum()) - 1.17) < 0.005


def _corpus(n=12, N=250):
    sk, _ = synthetic_corpus(64, seed=0, max_len=N)
    sk = sk[:n]
    x = np.zeros((n, N, 3), np.float32)
    for i, s in enumerate(sk):
        x[i, :len(s)] = s
    return sk, torch.tensor(x), torch.tensor([len(s) for s in sk])


@pytest.mark.parametrize("S", [28, 33])
def test_fp32_against_fp64(S):
    _, x, L = _corpus()
    a, fa = R.rasterize_torch(x, L, size=S)
    b, fb = R.rasterize_torch(x, L, size=S, dtype=torch.float32)
    assert b.dtype == torch.float32 and fb.dtype == torch.float32
    assert float((a - b.double()).abs().max()) <= 1e-4
    assert float(((a > 0).double().mean((1, 2))).min()) > 0.01   # no blank image passes
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0


def test_rows_past_length_take_part_in_nothing():
    _, x, L = _corpus(6)
    poisoned = x.clone()
    for i, n in enumerate(L.tolist()):
        poisoned[i, n:] = float("nan")
    for dtype in (torch.float32, torch.float64):
        a, fa = R.rasterize_torch(x, L, size=28, dtype=dtype)
        b, fb = R.rasterize_torch(poisoned, L, size=28, dtype=dtype)
        assert torch.equal(a, b) and torch.equal(fa, fb)


def test_stroke5_equals_stroke3_and_lengths():
    sk, x, L = _corpus(6, 250)
    x5 = torch.tensor(np.stack([to_big_strokes(s, 250) for s in sk]))
    assert torch.equal(R.stroke5_lengths(x5), L)
    a, fa = R.rasterize_torch(x, L, size=28, dtype=torch.float32)
    for lens in (None, L):
        b, fb = R.rasterize_torch(x5, lens, size=28, dtype=torch.float32)
        assert torch.equal(a, b) and torch.equal(fa, fb)


def test_stroke5_lengths_rule():
    s = torch.zeros(4, 3, 5)
    s[0, 0, 4] = 1           # end-of-sketch in row 0: length 0, not to_normal_strokes' "full length"
    s[1, 2, 4] = 1
    s[2, 1, 4] = 0.5         # > 0 counts
    s[2, 2, 4] = 1
    assert R.stroke5_lengths(s).tolist() == [0, 2, 1, 3]
    assert R.stroke5_lengths(s).dtype == torch.int64
    assert R.stroke5_lengths(torch.zeros(2, 0, 5)).tolist() == [0, 0]
    with pytest.raises(ValueError):
        R.stroke5_lengths(torch.zeros(2, 3, 3))


def test_given_frame_reproduces_the_fitted_call():
    _, x, L = _corpus(6)
    for dtype in (torch.float32, torch.float64):
        a, fa = R.rasterize_torch(x, L, size=33, width=1.5, dtype=dtype)
        b, fb = R.rasterize_torch(x, L, size=33, width=1.5, frame=fa, dtype=dtype)
        assert torch.equal(a, b) and torch.equal(fa, fb)
    a, fa = R.rasterize(x, L, size=33)
    b, _ = R.rasterize(x, L, size=33, frame=fa)
    assert torch.equal(a, b)
    out = torch.full((6, 33, 33), 7.0)
    c, _ = R.rasterize(x, L, size=33, out=out)
    assert c is out and torch.equal(out, a)


def test_given_frame_clips():
    img, _ = _hand(frame=torch.tensor([[2.0, 0.0, 0.0]]))      # (4, 5) -> (12, 5): runs off the canvas
    assert float(img[0, 4:6, 4:].min()) > 0 and float(img[0, :3].abs().max()) == 0.0


def test_value_errors():
    x, L = torch.zeros(2, 4, 3), torch.tensor([4, 2])
    bad = [
        dict(strokes=torch.zeros(2, 4, 4)), dict(strokes=torch.zeros(2, 4)), dict(strokes=torch.zeros(2, 4, 3).long()),
        dict(lengths=None),                                     # stroke-3 needs lengths
        dict(lengths=torch.tensor([4, 2, 1])), dict(lengths=torch.tensor([4.0, 2.0])),
        dict(size=0), dict(size=513), dict(size=8.0),
        dict(width=0.0), dict(width=-1.0), dict(width=float("nan")),
        dict(pad=-0.5), dict(pad=4.0, size=8), dict(pad=float("inf")),
        dict(frame=torch.ones(3, 3)), dict(frame=torch.ones(2, 2)),
        dict(frame=torch.tensor([[1.0, 0, 0], [0.0, 0, 0]])), dict(frame=torch.tensor([[1.0, 0, 0], [-1.0, 0, 0]])),
        dict(frame=torch.tensor([[1.0, 0, 0], [1.0, float("nan"), 0]])),
        dict(frame=torch.tensor([[1.0, 0, 0], [float("inf"), 0, 0]])),
        dict(out=torch.zeros(2, 8, 9)), dict(out=torch.zeros(2, 8, 8, dtype=torch.float64)),
    ]
    for kw in bad:
        args = dict(strokes=x, lengths=L, size=8)
        args.update(kw)
        for fn in (R.rasterize, R.rasterize_torch):
            if fn is R.rasterize_torch and "out" in kw and kw["out"].dtype == torch.float64:
                continue                                        # the fp64 oracle takes an fp64 out
            with pytest.raises(ValueError):
                fn(**args)
    R.rasterize(x, L, size=1, pad=0.0)                          # the smallest canvas
    R.rasterize(x, L, size=512)


def test_soft_iou_and_to_uint8():
    a = torch.zeros(3, 4, 4)
    b = torch.zeros(3, 4, 4)
    a[0, 0, :2] = 1.0
    b[0, 0, 1:3] = 0.5
    a[1, 1, 1] = 0.25
    assert torch.allclose(soft_iou(a, b), torch.tensor([0.5 / 2.5, 0.0, 1.0]))
    assert torch.equal(soft_iou(a, a), torch.ones(3))
    with pytest.raises(ValueError):
        soft_iou(a, b[:2])
    g = to_uint8(torch.tensor([[0.0, 1.0, 0.5, 2.0, -1.0]]))
    assert g.dtype == np.uint8 and g.tolist() == [[255, 0, 127, 0, 255]]


# ----------------------------------------------------------------------------
# PNG
# ----------------------------------------------------------------------------
def _read_png(path):
    """Parse by hand: signature, chunk CRCs, inflate, filter type 0 on every line."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 1 if ctype == 0 else 3
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    assert len(raw) == h * (1 + w * ch)
    lines = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
    assert not lines[:, 0].any()
    px = lines[:, 1:]
    return px.reshape(h, w) if ch == 1 else px.reshape(h, w, 3)


@pytest.mark.parametrize("shape", [(5, 7), (1, 1), (6, 4, 3)])
def test_write_png(tmp_path, shape):
    a = np.random.RandomState(0).randint(0, 256, size=shape).astype(np.uint8)
    path = str(tmp_path / "a.png")
    P.write_png(path, a)
    assert np.array_equal(_read_png(path), a)
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(path)), a)


def test_write_png_rejects():
    for a in (np.zeros((2, 2), np.float32), np.zeros((2, 2, 4), np.uint8), np.zeros((0, 2), np.uint8), np.zeros(3, np.uint8)):
        with pytest.raises(ValueError):
            P.png_bytes(a)


def test_grid_png_ragged(tmp_path):
    rng = np.random.RandomState(1)
    ink = torch.tensor(rng.rand(7, 6, 6), dtype=torch.float32)
    path = str(tmp_path / "g.png")
    grid = P.grid_png(ink, path, maxcol=3, margin=2)
    got = _read_png(path)
    assert got.shape == (3 * 10, 3 * 10) and np.array_equal(got, grid)
    want = np.full((30, 30), 255, np.uint8)
    for k in range(7):
        y, x = (k // 3) * 10 + 2, (k % 3) * 10 + 2
        want[y:y + 6, x:x + 6] = to_uint8(ink[k])
    assert np.array_equal(got, want)
    assert (got[20:, 10:] == 255).all()                       # the ragged last line stays white
    assert P.grid_png(ink[:2], None, maxcol=5, margin=0).shape == (6, 12)
    assert P.grid_png(ink[:0], None) is None


# ----------------------------------------------------------------------------
# vae_sample --png / --raster_iou
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = VAEConfig(enc_rnn_size=16, dec_rnn_size=24, z_size=8, num_mixture=3, dec_model="layer_norm",
                    enc_model="layer_norm", max_seq_len=20, batch_size=4, conditional=True, num_classes=3)
    cfg = dataclasses.replace(cfg, is_training=True)
    (train, valid, test), _ = make_datasets(cfg, None, 60)
    d = str(tmp_path_factory.mktemp("raster") / "save_c")
    tr = VAETrainer(cfg, train, valid, test, device="cpu", save_dir=d, use_graph=False, log=lambda s: None)
    tr.train(num_steps=2, prefetch=False)
    if tr.step == 2:
        tr.save()
    return d


def test_vae_sample_png(saved, tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample
    # --greedy: the host sampler's component draws are not seeded, a greedy decode repeats
    base = ["--save_dir", saved, "--device", "cpu", "--n", "7", "--seed", "4", "--greedy"]
    plain, with_png, png = str(tmp_path / "a.svg"), str(tmp_path / "b.svg"), str(tmp_path / "b.png")
    assert vae_sample.main(base + ["--out", plain]) == 0
    out_plain = capsys.readouterr().out
    assert vae_sample.main(base + ["--out", with_png, "--png", png, "--png_size", "24", "--png_width", "1.5"]) == 0
    out_png = capsys.readouterr().out
    with open(plain, "rb") as f, open(with_png, "rb") as g:
        assert f.read() == g.read()                          # the SVG does not change with --png
    assert out_plain == "wrote %s (7 sketches)\n" % plain
    assert out_png.endswith("wrote %s (7 sketches)\n" % with_png) and png in out_png
    img = _read_png(png)
    assert img.shape == (2 * (24 + 4), 5 * (24 + 4))          # 7 sketches, maxcol 5, margin 2
    assert (img[28:, 2 * 28:] == 255).all() and (img < 255).any()


def test_vae_sample_png_temperatures_grid(saved, tmp_path):
    from sketch_rnn_amd.cli import vae_sample
    png = str(tmp_path / "t.png")
    base = ["--save_dir", saved, "--device", "cpu", "--n", "2", "--temperatures", "0.2,0.5,1.0", "--device_sampler"]
    assert vae_sample.main(base + ["--out", str(tmp_path / "t.svg"), "--png", png, "--png_size", "16"]) == 0
    assert _read_png(png).shape == (2 * 20, 3 * 20)           # one line per latent
    assert vae_sample.main(base + ["--out", str(tmp_path / "u.svg")]) == 0
    with open(str(tmp_path / "t.svg"), "rb") as f, open(str(tmp_path / "u.svg"), "rb") as g:
        assert f.read() == g.read()                          # the seeded device sampler: same SVG without --png


@pytest.mark.parametrize("device_sampler", [False, True])
def test_vae_sample_raster_iou(saved, tmp_path, capsys, device_sampler):
    from sketch_rnn_amd.cli import vae_sample
    out = str(tmp_path / "r.svg")
    args = ["--save_dir", saved, "--device", "cpu", "--n", "3", "--mode", "reconstruct", "--synthetic", "60",
            "--temperatures", "0.1,1.0", "--raster_iou", "--png_size", "32", "--out", out]
    assert vae_sample.main(args + (["--device_sampler"] if device_sampler else [])) == 0
    text = capsys.readouterr().out
    assert "raster IoU" in text and "T=0.1" in text and "T=1" in text
    with open(out + ".iou.json") as f:
        rec = json.load(f)
    iou = np.asarray(rec["iou"])
    assert iou.shape == (3, 2) and rec["temperatures"] == [0.1, 1.0] and rec["size"] == 32
    assert ((iou >= 0) & (iou <= 1)).all()
    assert np.allclose(rec["mean"], iou.mean(0))
    assert os.path.exists(out)


def test_vae_sample_raster_flags_rejected(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample
    base = ["--save_dir", str(tmp_path), "--device", "cpu", "--n", "2"]
    for extra, word in ((["--raster_iou"], "--raster_iou"), (["--png", "x.png", "--png_size", "4"], "--png_size"),
                        (["--png", "x.png", "--png_width", "0"], "--png_size")):
        with pytest.raises(SystemExit) as e:
            vae_sample.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
