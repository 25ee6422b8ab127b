"""Per-sketch likelihood scoring on the CPU: ``ops.mdn_head_score`` against a
per-sketch loop over ``mdn_loss_torch``, the masked-row select, the identity
that ties ``SketchVAE.score`` to ``loss(train=False)["r_cost"]``, the IWAE
bound and the ``vae_eval`` command line."""
import dataclasses

import numpy as np
import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import PRESETS, VAEConfig
from sketch_rnn_amd.models.mdn import mdn_loss_torch
from sketch_rnn_amd.models.vae import SketchVAE

T, B, HD, M = 7, 5, 24, 4
LENGTHS = [1, 3, 7, 7, 4]


def _head(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, HD, generator=g) * 0.5
    W = torch.randn(HD, 3 + 6 * M, generator=g) / HD ** 0.5
    b = 0.1 * torch.randn(3 + 6 * M, generator=g)
    t = torch.zeros(T, B, 5)
    t[..., :2] = torch.randn(T, B, 2, generator=g) * 0.7
    pen = torch.randint(0, 2, (T, B), generator=g)
    t.view(-1, 5)[torch.arange(T * B), 2 + pen.view(-1)] = 1.0
    lengths = torch.tensor(LENGTHS)
    # a well-formed batch: rows at t >= len are end-of-sketch padding (0, 0, 0, 0, 1)
    t[torch.arange(T).unsqueeze(1) >= lengths.unsqueeze(0)] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0])
    return x, W, b, t, lengths


def _loop(x, W, b, t, lengths, include_end):
    """Sketch b sliced to its len rows (p3 = 0 there, so the eval mask 1 - p3
    is 1), mdn_loss_torch (a mean) times len; the end row (p3 = 1) through
    is_training=True, whose pen term is the unmasked cross-entropy."""
    shape, pen = [], []
    for k, n in enumerate(lengths.tolist()):
        z = x[:n, k] @ W + b
        _, s, p = mdn_loss_torch(z, t[:n, k], M, mode="magenta", is_training=False)
        s, p = s * n, p * n
        if include_end and n < T:
            _, _, pe = mdn_loss_torch((x[n, k] @ W + b)[None], t[n:n + 1, k], M, mode="magenta", is_training=True)
            p = p + pe
        shape.append(s)
        pen.append(p)
    return torch.stack(shape), torch.stack(pen)


@pytest.mark.parametrize("include_end", [False, True])
def test_head_score_matches_per_sketch_loop(include_end):
    x, W, b, t, lengths = _head()
    shape, pen = ops.mdn_head_score(x, W, b, t, lengths, M, include_end=include_end)
    rs, rp = _loop(x, W, b, t, lengths, include_end)
    assert shape.shape == (B,) and pen.shape == (B,)
    assert torch.allclose(shape, rs, rtol=1e-5, atol=0), (shape, rs)
    assert torch.allclose(pen, rp, rtol=1e-5, atol=0), (pen, rp)
    if include_end:   # len == T: no end row; shorter sketches gained one positive term
        s0, p0 = ops.mdn_head_score(x, W, b, t, lengths, M, include_end=False)
        assert torch.equal(s0, shape)
        full = lengths == T
        assert torch.equal(p0[full], pen[full]) and bool((pen[~full] > p0[~full]).all())


@pytest.mark.parametrize("include_end", [False, True])
def test_head_score_ignores_masked_rows(include_end):
    x, W, b, t, lengths = _head(1)
    ref = ops.mdn_head_score(x, W, b, t, lengths, M, include_end=include_end)
    tt = torch.arange(T).unsqueeze(1)
    dead = tt >= (lengths + (1 if include_end else 0)).unsqueeze(0)
    assert bool(dead.any())
    xn, tn = x.clone(), t.clone()
    xn[dead] = float("nan")
    tn[dead] = float("nan")
    got = ops.mdn_head_score(xn, W, b, tn, lengths, M, include_end=include_end)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all())


def test_head_score_has_no_autograd():
    x, W, b, t, lengths = _head()
    with pytest.raises(RuntimeError):
        ops.mdn_head_score(x, W.requires_grad_(), b, t, lengths, M)
    with torch.no_grad():
        ops.mdn_head_score(x, W, b, t, lengths, M)


# loss(train=False) masks the pen term only for an evaluation-mode config
# (is_training=False): that is the r_cost the identity speaks of
_SMALL = dict(max_seq_len=20, batch_size=4, is_training=False)
CONFIGS = {
    "plumbing": dataclasses.replace(PRESETS["plumbing"], **_SMALL),
    "layer_norm": VAEConfig(enc_rnn_size=16, dec_rnn_size=24, z_size=8, num_mixture=3, dec_model="layer_norm",
                            enc_model="layer_norm", **_SMALL),
    "hyper": VAEConfig(enc_rnn_size=16, dec_rnn_size=24, z_size=8, num_mixture=3, dec_model="hyper",
                       hyper_num_units=12, hyper_embedding_size=4, num_classes=3, **_SMALL),
}


def _batch(cfg, idx=0):
    from sketch_rnn_amd.data.dataset import StrokeDataset
    from sketch_rnn_amd.data.synthetic import synthetic_corpus
    # sketches shorter than max_seq_len: every batch has padding after its longest sketch
    s, l = synthetic_corpus(16, seed=3, max_len=cfg.max_seq_len - 4, n_classes=max(cfg.num_classes, 1))
    ds = StrokeDataset(s, cfg.batch_size, cfg.max_seq_len, labels=l)
    ds.normalize()
    x, lens, lab = ds.get_batch(idx)
    return torch.as_tensor(x), torch.as_tensor(lens), torch.as_tensor(lab)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_score_identity_with_eval_loss_and_max_len(name):
    cfg = CONFIGS[name]
    m = SketchVAE(cfg, seed=0).eval()
    x, lens, lab = _batch(cfg)
    lab = lab if cfg.num_classes else None
    Nmax = x.shape[1] - 1
    assert int(lens.max()) < Nmax   # the batch is padded: max_len really cuts steps
    e = torch.randn(cfg.batch_size, cfg.z_size, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = float(m.loss(x, lens, lab, train=False, eps=e)["r_cost"])
    kw = dict(eps=e[None], include_end=False) if cfg.conditional else {}
    out = m.score(x, lens, lab, **kw)
    got = float(out["nll"].sum()) / (Nmax * cfg.batch_size)
    assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    assert torch.equal(out["points"], lens)
    assert torch.allclose(out["nll"], out["shape"] + out["pen"])
    cut = m.score(x, lens, lab, max_len=int(lens.max()), **kw)
    for k in ("shape", "pen", "nll"):
        assert torch.allclose(cut[k], out[k], rtol=1e-6, atol=0), k
    # the end row lies one step past the longest sketch: max_len keeps it
    kw["include_end"] = True
    a, c = m.score(x, lens, lab, **kw), m.score(x, lens, lab, max_len=int(lens.max()), **kw)
    assert torch.allclose(a["pen"], c["pen"], rtol=1e-6, atol=0)
    assert torch.equal(a["points"], lens + 1) and torch.equal(c["points"], lens + 1)
    assert bool((a["pen"] > out["pen"]).all()) and torch.allclose(a["shape"], out["shape"], rtol=1e-6, atol=0)


def test_score_iwae():
    cfg = CONFIGS["layer_norm"]
    m = SketchVAE(cfg, seed=1).eval()
    with torch.no_grad():   # the 0.001-scale initial latent heads give sigma ~ 1, mu ~ 0: make q informative
        m.encoder.mu_w.mul_(300.0)
        m.encoder.sig_w.mul_(300.0)
    x, lens, lab = _batch(cfg)
    one = m.score(x, lens, samples=1, seed=3)
    assert torch.allclose(one["iwae"], one["elbo"], rtol=1e-6, atol=1e-6)
    k8 = m.score(x, lens, samples=8, seed=3)
    assert set(k8) == {"shape", "pen", "nll", "points", "elbo", "iwae", "kl"}
    assert bool((k8["iwae"] >= k8["elbo"]).all())
    assert bool((k8["iwae"] > k8["elbo"]).any())
    assert bool((k8["kl"] >= 0).all())
    assert torch.equal(k8["points"], lens + (lens < x.shape[1] - 1).long())   # include_end defaults to True here
    again = m.score(x, lens, samples=8, seed=3)
    other = m.score(x, lens, samples=8, seed=4)
    for k in k8:
        assert torch.equal(k8[k], again[k]), k
    assert not torch.equal(k8["iwae"], other["iwae"])
    # the ELBO's definition: mean_k of -nll_k - (log q - log p); its KL part is a
    # Monte-Carlo estimate of the analytic sum-over-dimensions KL
    mu, presig = m.encode(x, lens)
    assert torch.allclose(k8["kl"], -0.5 * (1 + presig - mu * mu - presig.exp()).sum(-1), rtol=1e-5, atol=1e-6)
    # given noise: eps = 0 puts every sample at z = mu, where log q - log p is analytic
    z0 = m.score(x, lens, eps=torch.zeros(2, cfg.batch_size, cfg.z_size), include_end=False)
    mean = m.score(x, lens)
    assert torch.allclose(z0["nll"], mean["nll"], rtol=1e-5, atol=0)
    want = -mean["nll"] - 0.5 * (mu * mu).sum(-1) + 0.5 * presig.sum(-1)
    assert torch.allclose(z0["elbo"], want, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        SketchVAE(CONFIGS["plumbing"], seed=0).score(*_batch(CONFIGS["plumbing"])[:2], samples=1)


def test_vae_eval_cli(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_eval
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = dataclasses.replace(CONFIGS["layer_norm"], is_training=True)
    (train, valid, test), scale = make_datasets(cfg, None, 60)
    d = str(tmp_path / "save")
    tr = VAETrainer(cfg, train, valid, test, device="cpu", save_dir=d, use_graph=False, log=lambda s: None)
    tr.train(num_steps=2, prefetch=False)
    if tr.step == 2:
        tr.save()
    # the trainer's own array API, and the r_cost identity through evaluate's noise
    arr = tr.evaluate_sketches(test)
    n = test.num_batches * cfg.batch_size
    assert set(arr) == {"shape", "pen", "nll", "points"} and all(len(v) == n for v in arr.values())
    assert arr["points"].dtype == np.int64 and np.all(arr["points"] >= 1)
    out = str(tmp_path / "scores.npz")
    args = ["--save_dir", d, "--synthetic", "60", "--device", "cpu", "--dtype", "fp32", "--out", out]
    assert vae_eval.main(args) == 0
    txt = capsys.readouterr().out
    assert txt.startswith("%d sketches" % n) and "NLL per sketch" in txt and "NLL per point" in txt
    z = np.load(out)
    assert sorted(z.files) == ["nll", "pen", "points", "shape"] and all(len(z[k]) == n for k in z.files)
    assert np.allclose(z["nll"], arr["nll"], rtol=1e-6)      # the checkpoint round trip scores the same
    assert vae_eval.main(args + ["--compare_dir", d, "--samples", "2"]) == 0
    txt = capsys.readouterr().out
    assert "ELBO (K=2)" in txt and "IWAE-2" in txt
    assert "paired difference B - A of NLL per point: +0.000000 +- 0.000000" in txt
    z = np.load(out)
    assert {"iwae", "elbo", "kl", "b_nll", "b_iwae"} <= set(z.files) and len(z["b_nll"]) == n
    assert np.array_equal(z["nll"], z["b_nll"])
