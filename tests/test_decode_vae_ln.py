"""Fused whole-sketch decoder for LayerNorm-LSTM VAE decoders
(sketch_rnn_amd/sample/fused.py FusedLNVAEDecoder, csrc/decode_vae_ln.hip),
the parts that need no GPU: which models are eligible, the PyTorch
transcription of the kernel's step (bf16 operands, per-16-unit-block
statistics partials combined in block order) against the fp32 step oracle,
and ``vae_sample --fused`` without a device.

``make_model`` / ``make_latent`` / ``make_inputs`` / ``step_oracle`` /
``transcription_forced`` are also what tests/test_decode_vae_ln_gpu.py runs
the kernel against.
"""
import os

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import RefConfig, VAEConfig, save_json
from sketch_rnn_amd.models.reference import SketchRNN
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample.fused import (fused_vae_kind, fused_vae_ln_ok, fused_vae_ok,
                                         ln_decode_step_transcription)


def _vae(**kw):
    kw.setdefault("enc_rnn_size", 8)
    kw.setdefault("z_size", 4)
    return SketchVAE(VAEConfig(**kw), seed=0)


@pytest.mark.parametrize("kw", [
    dict(dec_rnn_size=512, num_mixture=20),                                        # conditional (vae_layernorm)
    dict(dec_rnn_size=256, num_mixture=20, conditional=False),
    dict(dec_rnn_size=512, num_mixture=20, num_classes=3, class_embed="add"),
    dict(dec_rnn_size=512, num_mixture=20, num_classes=3, class_embed="concat"),
    dict(dec_rnn_size=256, num_mixture=32),
])
def test_fused_vae_ln_ok_accepts(kw):
    m = _vae(dec_model="layer_norm", **kw)
    assert fused_vae_ln_ok(m)
    assert not fused_vae_ok(m)          # the plain decoder's predicate is unchanged


@pytest.mark.parametrize("kw", [
    dict(dec_model="lstm", dec_rnn_size=512, num_mixture=20),
    dict(dec_model="hyper", dec_rnn_size=512, num_mixture=20, hyper_num_units=16, hyper_embedding_size=4),
    dict(dec_model="layer_norm", dec_rnn_size=1024, num_mixture=20),
    dict(dec_model="layer_norm", dec_rnn_size=512, num_mixture=24),
    dict(dec_model="layer_norm", dec_rnn_size=256, num_mixture=33),
    dict(dec_model="layer_norm", dec_rnn_size=128, num_mixture=20),
])
def test_fused_vae_ln_ok_rejects(kw):
    assert not fused_vae_ln_ok(_vae(**kw))


def test_fused_vae_ln_ok_rejects_reference_model():
    assert not fused_vae_ln_ok(SketchRNN(RefConfig(rnn_size=256, num_layers=1, num_mixture=20), seed=0))


def test_fused_vae_kind():
    assert fused_vae_kind(_vae(dec_model="lstm", dec_rnn_size=512, num_mixture=20)) == "lstm"
    assert fused_vae_kind(_vae(dec_model="layer_norm", dec_rnn_size=256, num_mixture=20)) == "layer_norm"
    assert fused_vae_kind(_vae(dec_model="hyper", dec_rnn_size=512, num_mixture=20, hyper_num_units=16,
                               hyper_embedding_size=4)) is None
    assert fused_vae_kind(_vae(dec_model="layer_norm", dec_rnn_size=1024, num_mixture=20)) is None
    assert fused_vae_kind(SketchRNN(RefConfig(rnn_size=256, num_layers=1, num_mixture=20), seed=0)) is None


# ---------------------------------------------------------------------------------------
# the test model and the two references (shared with the GPU file)
# ---------------------------------------------------------------------------------------
def make_model(H, M, kind="cond", seed=3, eos_bias=0.0):
    """Random-init ``layer_norm`` VAE with the changes that make indexing
    mistakes show: ``init_w`` x30 (|h0|, |c0| ~ 0.9), ``output_b`` ~ N(0, 0.1),
    and every layer-norm gain ~ 1 + 0.3 N(0, 1) / shift ~ 0.3 N(0, 1), so each
    gate and unit has parameters of its own."""
    kw = {"cond": {}, "uncond": {"conditional": False},
          "class": {"num_classes": 3, "class_embed": "concat"}}[kind]
    m = SketchVAE(VAEConfig(dec_model="layer_norm", enc_rnn_size=64, dec_rnn_size=H, num_mixture=M, **kw), seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        if m.z_in:
            m.init_w *= 30
        m.output_b.copy_(torch.randn(m.output_b.shape, generator=g) * 0.1)
        m.output_b[2] += eos_bias          # the end-of-sketch pen logit
        for name in ("ln_gamma", "lnc_gamma"):
            p = getattr(m.dec, name)
            p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
        for name in ("ln_beta", "lnc_beta"):
            p = getattr(m.dec, name)
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return m.eval()


def make_latent(m, B, seed, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, m.cfg.z_size, generator=g).to(dev) if m.cfg.conditional else None
    labels = (torch.arange(B) % 3).to(dev) if m.cfg.num_classes > 0 else None
    return z, labels


def make_inputs(N, B, seed):
    """Fed inputs: the start token, then strokes of all three pen states."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, B, 5)
    x[..., :2] = torch.randn(N, B, 2, generator=g) * 0.6
    pen = torch.multinomial(torch.tensor([0.8, 0.15, 0.05]), N * B, replacement=True, generator=g).view(N, B)
    x[..., 2:] = torch.nn.functional.one_hot(pen, 3).float()
    x[0] = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0])
    return x


@torch.no_grad()
def step_oracle(m, xs, z, labels):
    """Head outputs ``[N, B, 3+6M]`` of the fp32 PyTorch step loop
    (``SketchVAE.decode_step``, backend ``torch``)."""
    ops.set_backend("torch")
    ops.set_compute_dtype("fp32")
    N, B, dev = xs.shape[0], xs.shape[1], xs.device
    zc = m.condition(z, labels, B, dev)
    st = m.initial_state(zc, B, dev)
    zo = []
    for t in range(N):
        zt, st = m.decode_step(xs[t], zc, st)
        zo.append(zt)
    return torch.stack(zo)


@torch.no_grad()
def transcription_forced(m, xs, z, labels):
    """The same loop through :func:`ln_decode_step_transcription`, started as
    ``FusedLNVAEDecoder`` starts the kernel (h0 rounded to bf16, c0 fp32)."""
    N, B, dev = xs.shape[0], xs.shape[1], xs.device
    zc = m.condition(z, labels, B, dev)
    h, c = m.initial_state(zc, B, dev)
    zp = zc.float() @ m.dec.W_x.detach().float()[5:] if zc is not None else None
    h, c = h.to(torch.bfloat16).float(), c.float()
    zo = []
    for t in range(N):
        zt, h, c = ln_decode_step_transcription(m, xs[t], zp, h, c)
        zo.append(zt)
    return torch.stack(zo)


def errors(a, ref):
    """(relative Frobenius error, max error, max |ref|)."""
    return ((a - ref).norm() / ref.norm()).item(), (a - ref).abs().max().item(), ref.abs().max().item()


@pytest.fixture
def _restore_ops():
    yield
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")


@pytest.mark.parametrize("H,M,kind,B", [(512, 20, "cond", 37), (256, 20, "uncond", 5), (256, 32, "cond", 8),
                                        (512, 20, "class", 6)])
def test_transcription_matches_step_oracle(H, M, kind, B, _restore_ops):
    """The kernel's arithmetic (bf16 W_h / W_out / carried h, block partials
    combined in block order, direct form) against the fp32 oracle over 30
    steps. What separates them is the bf16 rounding alone, so the plain
    decoder's bounds (rel < 1e-2, max < 5 % of max |z|) must hold with room;
    the figures printed here are what the GPU test's bounds refer to."""
    m = make_model(H, M, kind)
    N = 30
    xs = make_inputs(N, B, B * 7 + N)
    z, labels = make_latent(m, B, 11)
    zo = step_oracle(m, xs, z, labels)
    zt = transcription_forced(m, xs, z, labels)
    rel, err, top = errors(zt, zo)
    print("transcription H %d M %d %s B %d N %d: rel %.3e max %.3e of %.3e" % (H, M, kind, B, N, rel, err, top))
    assert torch.isfinite(zt).all()
    assert rel < 1e-2 and err < 0.05 * top, (rel, err, top)


def test_transcription_statistics_are_the_layer_norms(_restore_ops):
    """With fp32 operands in place of bf16 ones the transcription IS
    ``ln_lstm_pointwise``: its block-partial statistics are the row mean and
    biased variance (fp32 rounding apart)."""
    from sketch_rnn_amd.models import cells as C
    m = make_model(256, 20)
    B = 7
    g = torch.Generator().manual_seed(5)
    gates = torch.randn(B, 4 * 256, generator=g) * 2 + 0.5
    c = torch.randn(B, 256, generator=g)
    p = m.dec
    h_ref, c_ref = C.ln_lstm_pointwise(gates, c, p.ln_gamma, p.ln_beta, p.lnc_gamma, p.lnc_beta, 1.0)
    # feed `gates` through the transcription: h = 0, x = 0, zp = gates
    _, h_t, c_t = ln_decode_step_transcription(m, torch.zeros(B, 5), gates, torch.zeros(B, 256), c)
    assert torch.allclose(c_t, c_ref.detach(), rtol=1e-5, atol=1e-5)
    assert torch.allclose(h_t, h_ref.detach().to(torch.bfloat16).float(), rtol=0, atol=1e-2)


def test_vae_sample_fused_layer_norm_without_gpu(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample as cvs
    save_json(VAEConfig(dec_model="layer_norm", enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2,
                        max_seq_len=12), str(tmp_path / "config.json"))
    out = str(tmp_path / "g.svg")
    assert cvs.main(["--save_dir", str(tmp_path), "--out", out, "--n", "2", "--device", "cpu",
                     "--device_sampler", "--fused"]) == 0
    assert "--fused" in capsys.readouterr().out
    assert os.path.getsize(out) > 100
