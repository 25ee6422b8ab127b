"""Sketch completion and reconstruction on the CPU: forced strokes in the
sampler's PyTorch transcription, stroke prefixes through ``GraphDecoder`` and
``sample_vae``, their validation, and the ``vae_sample`` modes ``reconstruct``
and ``complete``."""
import dataclasses
import os
import random

import numpy as np
import pytest
import torch

from sketch_rnn_amd.config import RefConfig, VAEConfig
from sketch_rnn_amd.models.reference import SketchRNN
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import sampler as SM

N, B, TEMP = 48, 12, 0.5


def _model(dec_model, seed=0):
    cfg = VAEConfig(enc_rnn_size=32, dec_rnn_size=64, z_size=16, dec_model=dec_model, hyper_num_units=32,
                    hyper_embedding_size=8, num_classes=0, max_seq_len=N)
    m = SketchVAE(cfg, seed=seed).eval()
    with torch.no_grad():    # p3 ~ 6 % per stroke at temperature 0.5: sketches long enough to complete
        m.output_b[2] -= 1.0
    return cfg, m


def _z(cfg, seed=1):
    return torch.randn(B, cfg.z_size, generator=torch.Generator().manual_seed(seed))


def _prefix(P=9, seed=2):
    """[B, P, 5] pen-down / pen-up strokes, and mixed lengths with 0 and P."""
    g = torch.Generator().manual_seed(seed)
    pre = torch.zeros(B, P, 5)
    pre[..., :2] = torch.randn(B, P, 2, generator=g) * 0.5
    pen = torch.randint(0, 2, (B, P), generator=g)
    pre.view(-1, 5)[torch.arange(B * P), 2 + pen.view(-1)] = 1.0
    plen = torch.tensor([0, P, 1, 4, P, 0, 7, 2, P - 1, 3, 5, 6])
    return pre, plen


def _not_vacuous(lengths, n=N):
    """At least a quarter of the rows are worth completing, and at least a
    quarter end on their own."""
    assert (lengths >= 8).float().mean().item() >= 0.25, lengths
    assert (lengths < n).float().mean().item() >= 0.25, lengths


@pytest.mark.parametrize("mode,greedy,step", [(1, False, 0), (1, False, 3), (0, False, 5), (1, True, 2)])
def test_mdn_sample_torch_forced(mode, greedy, step):
    Bn, M = 64, 5
    g = torch.Generator().manual_seed(step)
    z = torch.randn(Bn, 3 + 6 * M, generator=g) * 2
    done0 = (torch.rand(Bn, generator=g) < 0.3).to(torch.int32)
    forced = torch.randn(Bn, 5, generator=g)
    stop_col = 4 if mode == 1 else 3
    forced[:, 2:] = 0.0
    forced[torch.arange(Bn), 2 + torch.randint(0, 3, (Bn,), generator=g)] = 1.0
    nforced = torch.tensor([0, step, step + 1, 10 ** 6], dtype=torch.int32).repeat(Bn // 4)
    on = step < nforced
    assert bool(on.any()) and bool((~on).any()) and bool((on & (done0 != 0)).any())
    assert bool((forced[on][:, stop_col] > 0).any()) and bool((forced[on][:, stop_col] == 0).any())
    seed = torch.tensor([7], dtype=torch.int64)

    def call(zz, **kw):
        out, nx, pr, done = torch.zeros(Bn, 5), torch.zeros(Bn, 5), torch.zeros(Bn, 4), done0.clone()
        SM.mdn_sample_torch(zz, M, mode, TEMP, greedy, False, seed, step, out, nx, done, pr, **kw)
        return out, nx, done, pr

    o0, n0, d0, p0 = call(z)
    o1, n1, d1, p1 = call(z, forced=forced, nforced=nforced)
    assert torch.equal(o1[on], forced[on]) and torch.equal(n1[on], forced[on])
    assert torch.equal(d1[on], ((done0[on] != 0) | (forced[on][:, stop_col] > 0)).to(torch.int32))
    assert torch.equal(o1[~on], o0[~on]) and torch.equal(n1[~on], n0[~on]) and torch.equal(d1[~on], d0[~on])
    assert torch.equal(p1, p0)                         # params keep describing the draw
    zn = z.clone()
    zn[on] = float("nan")                              # a select: nothing of a forced row's head output leaks
    o2, n2, d2, _ = call(zn, forced=forced, nforced=nforced)
    assert torch.equal(o2, o1) and torch.equal(n2, n1) and torch.equal(d2, d1)
    # mdn_sample_device off the GPU is the same function
    out, nx, done = torch.zeros(Bn, 5), torch.zeros(Bn, 5), done0.clone()
    SM.mdn_sample_device(z, M, mode, TEMP, greedy, False, seed, step, out, nx, done, None, forced, nforced)
    assert torch.equal(out, o1) and torch.equal(nx, n1) and torch.equal(done, d1)


def _oracle(m, cfg, z, seed, pre, plen):
    """Explicit loop over ``decode_step`` fed [S0, prefix], continued with the
    plain sampler at the same (seed, step)."""
    zc = m.condition(z if cfg.conditional else None, None, B, "cpu")
    state = m.initial_state(zc, B, "cpu")
    x = torch.zeros(B, 5)
    x[:, 2] = 1.0
    out, done = torch.zeros(B, N, 5), torch.zeros(B, dtype=torch.int32)
    sd = torch.tensor([seed], dtype=torch.int64)
    with torch.no_grad():
        for t in range(N):
            zh, state = m.decode_step(x, zc, state)
            before, nx = done.clone(), torch.zeros(B, 5)
            SM.mdn_sample_torch(zh, cfg.num_mixture, 1, TEMP, False, False, sd, t, out[:, t], nx, done)
            given = t < plen
            if t < pre.shape[1]:
                out[given, t] = pre[given, t]
                nx[given] = pre[given, t]
            done[given] = before[given]
            x = nx
    hits = out[:, :, 4] > 0
    return out, torch.where(hits.any(1), hits.float().argmax(1) + 1, torch.full((B,), N))


@pytest.mark.parametrize("dec_model", ["lstm", "layer_norm", "hyper"])
def test_graph_decoder_prefix_cpu(dec_model):
    cfg, m = _model(dec_model)
    z = _z(cfg)
    pre, plen = _prefix()
    dec = SM.GraphDecoder(m, batch=B, steps=N, temperature=TEMP)
    s0, l0 = dec.run(seed=3, z=z)
    _not_vacuous(l0)
    s1, l1 = dec.run(seed=3, z=z, prefix=pre, prefix_len=plen)
    for b in range(B):                                                   # (a)
        assert torch.equal(s1[b, :plen[b]], pre[b, :plen[b]]), b
        assert int(l1[b]) > int(plen[b])
    _not_vacuous(l1)
    assert not torch.equal(s1, s0)
    sz, lz = dec.run(seed=3, z=z, prefix=pre, prefix_len=torch.zeros(B, dtype=torch.int64))   # (b)
    assert torch.equal(sz, s0) and torch.equal(lz, l0)
    sp, lp = dec.run(seed=3, z=z)                                        # a prefix does not stick
    assert torch.equal(sp, s0) and torch.equal(lp, l0)
    so, lo = _oracle(m, cfg, z, 3, pre, plen)                            # (c)
    assert torch.equal(s1, so) and torch.equal(l1, lo)
    sf, lf = dec.run(seed=3, z=z, prefix=pre[:, :4])                     # prefix_len defaults to P
    assert torch.equal(sf[:, :4], pre[:, :4])
    # (d) a row's own leading strokes as its prefix change nothing: the noise is keyed by (seed, step, row)
    k = torch.stack([torch.zeros_like(l0), torch.ones_like(l0), l0 // 2, l0 - 1])[torch.arange(B) % 4, torch.arange(B)]
    k = torch.minimum(k, l0 - 1)
    assert bool((k > 1).any())
    ss, ls = dec.run(seed=3, z=z, prefix=s0[:, :int(k.max())], prefix_len=k)
    assert torch.equal(ss, s0) and torch.equal(ls, l0)


def test_prefix_validation():
    cfg, m = _model("lstm")
    dec = SM.GraphDecoder(m, batch=B, steps=N, temperature=TEMP)
    pre, plen = _prefix()
    P = pre.shape[1]
    bad = [dict(prefix=pre[:-1]), dict(prefix=pre[:, :, :4]), dict(prefix=pre, prefix_len=plen[:-1]),
           dict(prefix=pre[0]), dict(prefix=pre, prefix_len=plen + 1), dict(prefix=pre, prefix_len=plen - 1),
           dict(prefix_len=plen)]
    ends = pre.clone()
    ends[3, 2] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0])
    bad.append(dict(prefix=ends, prefix_len=plen))            # row 3 has length 4: p3 inside it
    for kw in bad:
        with pytest.raises(ValueError):
            dec.run(seed=0, **kw)
    ends[3, 2] = pre[3, 2]
    ends[3, 4] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0])      # p3 past the row's length is not read
    dec.run(seed=0, prefix=ends, prefix_len=plen)
    long = torch.zeros(B, N + 3, 5)
    long[..., 2] = 1.0
    with pytest.raises(ValueError):
        dec.run(seed=0, prefix=long)                          # default length P > steps
    s, _ = dec.run(seed=0, prefix=long, prefix_len=torch.full((B,), N))
    assert torch.equal(s, long[:, :N])
    ref = SM.GraphDecoder(SketchRNN(RefConfig(rnn_size=32, num_mixture=4), seed=0), batch=B, steps=8)
    with pytest.raises(ValueError):
        ref.run(seed=0, prefix=pre[:, :4])
    ref.run(seed=0)
    assert P == 9


def test_sample_vae_prefix():
    cfg, m = _model("layer_norm")
    pre = _prefix()[0][0].numpy()
    z = _z(cfg)[:1]
    s, params = SM.sample_vae(m, N, TEMP, z=z, rng=np.random.RandomState(0), prefix=pre)
    assert s.shape == (N, 5) and len(params) == N
    assert np.array_equal(s[:len(pre)], pre)
    assert np.all(s[len(pre):, 2:].sum(1) == 1)
    s0, _ = SM.sample_vae(m, N, TEMP, z=z, rng=np.random.RandomState(0), py_rng=random.Random(0), prefix=pre[:0])
    s1, _ = SM.sample_vae(m, N, TEMP, z=z, rng=np.random.RandomState(0), py_rng=random.Random(0))
    assert np.array_equal(s0, s1)
    end = pre.copy()
    end[2] = [0, 0, 0, 0, 1]
    for bad in (end, pre[:, :4], np.zeros((N + 1, 5), np.float32)):
        with pytest.raises(ValueError):
            SM.sample_vae(m, N, TEMP, z=z, prefix=bad)


def _saved(tmp_path, conditional=True):
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = VAEConfig(enc_rnn_size=16, dec_rnn_size=24, z_size=8, num_mixture=3, dec_model="layer_norm",
                    enc_model="layer_norm", max_seq_len=20, batch_size=4, conditional=conditional, num_classes=3)
    cfg = dataclasses.replace(cfg, is_training=True)
    (train, valid, test), _ = make_datasets(cfg, None, 60)
    d = str(tmp_path / ("save_c" if conditional else "save_u"))
    tr = VAETrainer(cfg, train, valid, test, device="cpu", save_dir=d, use_graph=False, log=lambda s: None)
    tr.train(num_steps=2, prefetch=False)
    if tr.step == 2:
        tr.save()
    return d


@pytest.mark.parametrize("device_sampler", [False, True])
def test_vae_sample_cli_reconstruct_complete(tmp_path, capsys, device_sampler):
    from sketch_rnn_amd.cli import vae_sample
    d = _saved(tmp_path)
    n, K = 3, 2
    base = ["--save_dir", d, "--synthetic", "60", "--device", "cpu", "--n", str(n), "--offset", "1"]
    base += ["--device_sampler"] if device_sampler else []
    out = str(tmp_path / "rec.svg")
    assert vae_sample.main(base + ["--mode", "reconstruct", "--out", out]) == 0
    assert "(%d sketches)" % (2 * n) in capsys.readouterr().out
    assert vae_sample.main(base + ["--mode", "reconstruct", "--sample_z", "--out", out]) == 0
    capsys.readouterr()
    for z_from in ("prefix", "full", "prior"):
        out = str(tmp_path / ("cmp_%s.svg" % z_from))
        args = base + ["--mode", "complete", "--completions", str(K), "--z_from", z_from, "--out", out]
        assert vae_sample.main(args) == 0
        assert "(%d sketches)" % (n * (1 + K)) in capsys.readouterr().out
        assert open(out).read().count("<path") >= n * K


def test_vae_sample_cli_grid_holds_data_then_decodes(tmp_path, monkeypatch):
    """The grids' contents: ``reconstruct`` lays out [original, decode] pairs and
    ``complete`` [prefix, K decodes that begin with the prefix]."""
    from sketch_rnn_amd.cli import vae_eval, vae_sample
    from sketch_rnn_amd.config import load_json
    from sketch_rnn_amd.render import svg
    d = _saved(tmp_path)
    cfg = load_json(os.path.join(d, "config.json"))
    ds, _ = vae_eval.load_split(cfg, None, 60, "test", d)
    got = {}
    monkeypatch.setattr(svg, "grid_strokes3", lambda sk, path, **kw: got.update(sk=[np.asarray(x) for x in sk]))
    n, K = 4, 3
    base = ["--save_dir", d, "--synthetic", "60", "--device", "cpu", "--n", str(n), "--offset", "2"]
    assert vae_sample.main(base + ["--mode", "reconstruct", "--device_sampler"]) == 0
    assert len(got["sk"]) == 2 * n
    for i in range(n):
        assert np.array_equal(got["sk"][2 * i], ds.strokes[2 + i])
    for dev in ([], ["--device_sampler"]):
        assert vae_sample.main(base + dev + ["--mode", "complete", "--completions", str(K), "--prefix_frac", "0.4"]) == 0
        assert len(got["sk"]) == n * (1 + K)
        for i in range(n):
            full = ds.strokes[2 + i]
            k = min(int(np.ceil(0.4 * len(full))), len(full) - 1)
            pre = got["sk"][i * (1 + K)]
            assert np.array_equal(pre, full[:k])
            for c in got["sk"][i * (1 + K) + 1:(i + 1) * (1 + K)]:
                assert len(c) >= k and np.array_equal(c[:k], pre)


def test_vae_sample_cli_reconstruct_needs_conditional(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample
    d = _saved(tmp_path, conditional=False)
    base = ["--save_dir", d, "--synthetic", "60", "--device", "cpu", "--n", "2", "--out", str(tmp_path / "x.svg")]
    assert vae_sample.main(base + ["--mode", "reconstruct"]) != 0
    assert "conditional" in capsys.readouterr().err
    assert vae_sample.main(base + ["--mode", "complete", "--completions", "2"]) == 0     # the decoder alone completes
    assert "(6 sketches)" in capsys.readouterr().out
