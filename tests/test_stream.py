"""Bulk generation on the CPU: ``StreamDecoder`` (blocks of ``slots`` jobs
through ``GraphDecoder``) against one plain ``GraphDecoder`` over all jobs,
``first_row``, ``GraphDecoder.run(row0=)``, validation, and ``vae_sample
--mode bulk``."""
import json
import os

import numpy as np
import pytest
import torch

from sketch_rnn_amd.config import RefConfig, VAEConfig, save_json
from sketch_rnn_amd.data.quickdraw import load_pack
from sketch_rnn_amd.data.strokes import to_normal_strokes
from sketch_rnn_amd.models.reference import SketchRNN
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.sample.stream import StreamDecoder

N, SLOTS, TEMP = 24, 8, 0.5


def _cfg(dec_model="hyper"):
    return VAEConfig(enc_rnn_size=32, dec_rnn_size=64, z_size=16, dec_model=dec_model, hyper_num_units=32,
                     hyper_embedding_size=8, num_classes=0, max_seq_len=N)


def _model(dec_model="hyper", seed=0):
    cfg = _cfg(dec_model)
    m = SketchVAE(cfg, seed=seed).eval()
    with torch.no_grad():    # fewer end-of-sketch draws: a spread of lengths inside N
        m.output_b[2] -= 1.0
    return cfg, m


def _z(cfg, J, seed=1):
    return torch.randn(J, cfg.z_size, generator=torch.Generator().manual_seed(seed))


def _temps(J):
    return torch.tensor([0.25, 0.5, 1.0])[torch.arange(J) % 3]


@pytest.mark.parametrize("dec_model", ["hyper", "lstm"])
@pytest.mark.parametrize("J", [0, 1, 8, 37])
@pytest.mark.parametrize("per_job", [False, True])
def test_stream_equals_plain_decoder(dec_model, J, per_job):
    cfg, m = _model(dec_model)
    z = _z(cfg, J)
    temp = _temps(J) if per_job else 0.7
    dec = StreamDecoder(m, SLOTS, N, TEMP)
    assert dec.impl == "blocks"
    s, l = dec.run(z, temperature=temp, seed=3)
    assert s.shape == (J, N, 5) and l.shape == (J,)
    if J == 0:
        assert dec.steps_run == dec.slot_steps == dec.valid_strokes == 0 and dec.occupancy == 0.0
        return
    s0, l0 = SM.GraphDecoder(m, J, N, TEMP).run(seed=3, z=z, temperature=temp)
    assert torch.equal(s, s0) and torch.equal(l, l0)
    if J == 37:
        assert int((l0 < N).sum()) >= 8 and int(l0.max()) > 5, l0    # the lengths vary: rows end on their own
    assert dec.valid_strokes == int(l0.sum())
    assert dec.slot_steps == SLOTS * dec.steps_run and dec.steps_run > 0
    assert dec.occupancy == dec.valid_strokes / dec.slot_steps
    assert dec.counters()["occupancy"] == dec.occupancy
    # default temperature: the constructor's
    s1, _ = dec.run(z, seed=3)
    s2, _ = SM.GraphDecoder(m, J, N, TEMP).run(seed=3, z=z)
    assert torch.equal(s1, s2)


def test_stream_does_not_depend_on_slots_or_chunk():
    cfg, m = _model()
    z = _z(cfg, 37)
    ref = StreamDecoder(m, SLOTS, N, TEMP).run(z, seed=5)
    for slots, chunk in ((5, None), (37, 4), (64, 7)):
        got = StreamDecoder(m, slots, N, TEMP, chunk=chunk).run(z, seed=5)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])


def test_first_row_splits_a_run():
    cfg, m = _model()
    z, t = _z(cfg, 37), _temps(37)
    dec = StreamDecoder(m, SLOTS, N, TEMP)
    s, l = dec.run(z, temperature=t, seed=9)
    for cut in (8, 13):
        sa, la = dec.run(z[:cut], temperature=t[:cut], seed=9)
        sb, lb = dec.run(z[cut:], temperature=t[cut:], seed=9, first_row=cut)
        assert torch.equal(torch.cat([sa, sb]), s) and torch.equal(torch.cat([la, lb]), l)
    sb, _ = dec.run(z[13:], temperature=t[13:], seed=9)          # without it the noise rows differ
    assert not torch.equal(sb, s[13:])


@pytest.mark.parametrize("kind", ["hyper", "lstm", "reference"])
def test_graph_decoder_row0_default(kind):
    if kind == "reference":
        m = SketchRNN(RefConfig(rnn_size=32, num_mixture=5, seq_length=N), seed=0).eval()
        kw = {}
    else:
        cfg, m = _model(kind)
        kw = dict(z=_z(cfg, 12))
    a = SM.GraphDecoder(m, 12, N, TEMP).run(seed=2, **kw)
    b = SM.GraphDecoder(m, 12, N, TEMP).run(seed=2, row0=0, **kw)
    c = SM.GraphDecoder(m, 12, N, TEMP).run(seed=2, row0=5, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])
    if kind != "reference":      # rows 5.. of a run are rows 0.. of a run with row0 = 5
        d = SM.GraphDecoder(m, 7, N, TEMP).run(seed=2, z=kw["z"][5:], row0=5)
        assert torch.equal(d[0], a[0][5:]) and torch.equal(d[1], a[1][5:])
    for bad in (-1, 2 ** 30 - 12):           # 4 * row + k is a 32-bit index
        with pytest.raises(ValueError):
            SM.GraphDecoder(m, 12, N, TEMP).run(seed=2, row0=bad, **kw)


def test_mdn_sample_torch_row0():
    B, M = 9, 5
    z = torch.randn(B, 3 + 6 * M, generator=torch.Generator().manual_seed(0)) * 2

    def run(zz, **kw):
        n = zz.shape[0]
        out, nx, done = torch.zeros(n, 5), torch.zeros(n, 5), torch.zeros(n, dtype=torch.int32)
        SM.mdn_sample_torch(zz, M, 1, 0.5, False, False, 7, 3, out, nx, done, **kw)
        return out, nx, done
    full, tail, plain = run(z), run(z[4:], row0=4), run(z[4:])
    for a, b in zip(full, tail):
        assert torch.equal(a[4:], b)
    assert not torch.equal(full[0][4:], plain[0])
    # a far row costs what a near one costs (only rows row0 .. row0 + B are hashed), up to the 32-bit limit
    from sketch_rnn_amd.models.cells import hash_uniform
    far = 2 ** 30 - 1 - B
    u = hash_uniform(7, 0x5A3D, 3, (B, 4), offset=4 * far)
    assert u.shape == (B, 4) and bool(((u >= 0) & (u < 1)).all())
    assert torch.equal(hash_uniform(7, 0x5A3D, 3, (6 + B, 4))[6:], hash_uniform(7, 0x5A3D, 3, (B, 4), offset=24))
    run(z, row0=far)


def test_stream_value_errors():
    cfg, m = _model()
    z = _z(cfg, 5)
    ref = SketchRNN(RefConfig(rnn_size=32, num_mixture=5, seq_length=N), seed=0).eval()
    for bad in (lambda: StreamDecoder(ref, SLOTS, N),
                lambda: StreamDecoder(m, 0, N),
                lambda: StreamDecoder(m, SLOTS, 0),
                lambda: StreamDecoder(m, SLOTS, N, chunk=0),
                lambda: StreamDecoder(m, SLOTS, N, temperature=0.0),
                lambda: StreamDecoder(m, SLOTS, N, fp8=True)):
        with pytest.raises(ValueError):
            bad()
    dec = StreamDecoder(m, SLOTS, N, TEMP)
    pre = torch.zeros(5, 3, 5)
    pre[..., 2] = 1.0
    for kw in (dict(z=z[0]), dict(z=torch.zeros(5, cfg.z_size + 1)), dict(z=z, labels=torch.zeros(4, dtype=torch.long)),
               dict(z=z, temperature=torch.ones(4)), dict(z=z, temperature=0.0),
               dict(z=z, temperature=torch.tensor([1.0, 1.0, float("nan"), 1.0, 1.0])),
               dict(z=z, first_row=-1), dict(z=z, first_row=2 ** 30),
               dict(z=z, prefix=pre), dict(z=z, prefix=pre, prefix_len=torch.full((5,), 2)),
               dict(z=z, prefix_len=torch.full((5,), 2))):
        with pytest.raises(ValueError):
            dec.run(**kw)
    s, l = dec.run(z)            # and the decoder still works after them
    assert s.shape == (5, N, 5)


def test_vae_sample_cli_bulk(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample
    cfg = _cfg()
    d = str(tmp_path / "save")
    os.makedirs(d)
    save_json(cfg, os.path.join(d, "config.json"))
    pack = str(tmp_path / "bulk.npz")
    args = ["--save_dir", d, "--device", "cpu", "--mode", "bulk", "--n", "37", "--slots", "8", "--seed", "4",
            "--temperature", "0.5", "--out_pack", pack]
    assert vae_sample.main(args) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    sk, labels = load_pack(pack)["train"]
    assert len(sk) == 37 and len(labels) == 37
    # the API on the same latents
    m = SketchVAE(cfg).eval()
    z = torch.as_tensor(np.random.RandomState(4).randn(37, cfg.z_size), dtype=torch.float32)
    dec = StreamDecoder(m, 8, N, 0.5)
    s, l = dec.run(z, seed=4)
    for a, x, n in zip(sk, s.numpy(), l.numpy()):
        b = to_normal_strokes(x[:n])
        assert a.shape == b.shape and np.array_equal(a, b)
    assert line["impl"] == "blocks" and line["n"] == 37 and line["slots"] == 8 and line["dtype"] == "fp32"
    for k in ("steps_run", "slot_steps", "valid_strokes", "occupancy"):
        assert line[k] == getattr(dec, k), k
    # a smaller super-batch passes first_row on: the same pack
    vae_sample.BULK_SUPER, saved = 16, vae_sample.BULK_SUPER
    try:
        pack2 = str(tmp_path / "bulk2.npz")
        assert vae_sample.main(args[:-1] + [pack2, "--chunk", "6"]) == 0
    finally:
        vae_sample.BULK_SUPER = saved
    sk2, _ = load_pack(pack2)["train"]
    assert all(np.array_equal(a, b) for a, b in zip(sk, sk2)) and len(sk2) == 37
    for bad in (["--mode", "bulk", "--n", "4"], ["--mode", "bulk", "--out_pack", pack, "--slots", "0"],
                ["--mode", "bulk", "--out_pack", pack, "--temperatures", "0.5,1.0"]):
        with pytest.raises(SystemExit):
            vae_sample.main(["--save_dir", d, "--device", "cpu"] + bad)
