"""Fused whole-sketch decoder for the VAE's plain LSTM decoders
(csrc/decode_vae.hip, sketch_rnn_amd/sample/fused.py FusedVAEDecoder):

* teacher-forced head outputs against the fp32 PyTorch step oracle
  (``SketchVAE.decode_step`` in a loop), bf16 tolerances: H 512 and 256,
  conditional / unconditional / class-conditional, one row block / several /
  a batch split over two launches, the widest head;
* sampled strokes against the PyTorch transcription of the sampler applied
  to the kernel's own head outputs, and the kernel re-run teacher-forced on
  its own samples reproduces those head outputs;
* launching the steps in chunks, and leaving early once every row has ended,
  change no bit of the result;
* per-row stroke prefixes (sketch completion);
* replays are deterministic and the device seed changes the draws.

The models are random-init with three changes so indexing mistakes show:
``init_w`` x30 (|h0| ~ 0.9 instead of ~0.05: a swapped h0/c0 is visible), and
the decoder and output biases N(0, 0.1) instead of zero.
"""
import functools

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.sample.fused import FusedVAEDecoder, fused_vae_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    from sketch_rnn_amd.ops.recurrent import check_cluster_errors
    torch.cuda.synchronize()
    check_cluster_errors(DEV)


@functools.lru_cache(maxsize=None)
def _model(H, M, kind="cond", seed=3, eos_bias=0.0):
    kw = {"cond": {}, "uncond": {"conditional": False},
          "class": {"num_classes": 3, "class_embed": "concat"}}[kind]
    m = SketchVAE(VAEConfig(dec_model="lstm", enc_rnn_size=64, dec_rnn_size=H, num_mixture=M, **kw), seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        if m.z_in:
            m.init_w *= 30
        m.dec.bias.copy_(torch.randn(m.dec.bias.shape, generator=g) * 0.1)
        m.output_b.copy_(torch.randn(m.output_b.shape, generator=g) * 0.1)
        m.output_b[2] += eos_bias          # the end-of-sketch pen logit
    m = m.to(DEV).eval()
    assert fused_vae_ok(m)
    return m


def _latent(m, B, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, m.cfg.z_size, generator=g).to(DEV) if m.cfg.conditional else None
    labels = (torch.arange(B) % 3).to(DEV) if m.cfg.num_classes > 0 else None
    return z, labels


def _strokes(N, B, seed):
    """[N, B, 5] pen-down / pen-up strokes (no end of sketch)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, B, 5)
    x[..., :2] = torch.randn(N, B, 2, generator=g) * 0.6
    pen = torch.multinomial(torch.tensor([0.8, 0.2]), N * B, replacement=True, generator=g).view(N, B)
    x[..., 2:4] = torch.nn.functional.one_hot(pen, 2).float()
    return x


def _inputs(N, B, seed):
    """Fed inputs: the start token, then strokes of all three pen states."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, B, 5)
    x[..., :2] = torch.randn(N, B, 2, generator=g) * 0.6
    pen = torch.multinomial(torch.tensor([0.8, 0.15, 0.05]), N * B, replacement=True, generator=g).view(N, B)
    x[..., 2:] = torch.nn.functional.one_hot(pen, 3).float()
    x[0] = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0])
    return x


@pytest.mark.parametrize("H,M,kind,B,N", [
    (512, 20, "cond", 37, 30),      # two row blocks, the second partial
    (256, 20, "uncond", 5, 12),     # MTW = 1, z_in = 0
    (512, 20, "class", 20, 10),     # labels and the wider zc
    (512, 20, "cond", None, 6),     # rows of one launch + 6: a second launch, row0
    (256, 32, "cond", 40, 20),      # widest head
])
def test_fused_vae_forced_matches_step_oracle(H, M, kind, B, N):
    m = _model(H, M, kind)
    if B is None:
        B = FusedVAEDecoder(m, 64, N).rows + 6
    dec = FusedVAEDecoder(m, B, N)
    assert B <= dec.rows or len(range(0, B, dec.rows)) == 2
    xs = _inputs(N, B, B * 7 + N).to(DEV)
    z, labels = _latent(m, B, 11)
    zk = dec.forced(xs, z=z, labels=labels)
    ops.set_backend("torch")
    ops.set_compute_dtype("fp32")
    zc = m.condition(z, labels, B, DEV)
    st = m.initial_state(zc, B, DEV)
    zo = []
    for t in range(N):
        zt, st = m.decode_step(xs[t], zc, st)
        zo.append(zt)
    zo = torch.stack(zo)
    torch.cuda.synchronize()
    err = (zk - zo).abs().max().item()
    rel = ((zk - zo).norm() / zo.norm()).item()
    print("H %d M %d %s B %d N %d: rel %.3e max %.3e of %.3e" % (H, M, kind, B, N, rel, err, zo.abs().max().item()))
    assert rel < 1e-2 and err < 0.05 * zo.abs().max().item(), (rel, err)


def test_fused_vae_samples_match_sampler_transcription():
    m = _model(512, 20)
    B, N, temp, Mx = 48, 40, 0.5, 20
    z0, _ = _latent(m, B, 12)
    strokes, lengths, z = FusedVAEDecoder(m, B, N, temperature=temp, early_exit=False).run(seed=9, z=z0,
                                                                                          return_z=True)
    seed = torch.tensor([9], dtype=torch.int64, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    xs = torch.zeros(N, B, 5, device=DEV)
    xs[0, :, 2] = 1.0
    rows = torch.zeros(N, B, 5, device=DEV)
    for t in range(N):
        out, nx = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV)
        SM.mdn_sample_torch(z[t], Mx, 1, temp, False, False, seed, t, out, nx, done)
        rows[t] = out
        if t + 1 < N:
            xs[t + 1] = nx
    ref = rows.transpose(0, 1).clone()
    same = (ref[:, :, 2:] == strokes[:, :, 2:]).all(-1)
    print("pen agreement %.5f" % same.float().mean().item())
    assert same.float().mean().item() > 0.998
    assert torch.allclose(strokes[same], ref[same], rtol=1e-4, atol=1e-3)
    # the kernel fed its own draws back: teacher-forcing it on them (as
    # re-drawn by the transcription: offsets equal to float rounding of
    # exp/log/cos) reproduces z
    zf = FusedVAEDecoder(m, B, N, temperature=temp).forced(xs, z=z0)
    ok_rows = same.all(1)
    print("rows agreeing throughout %.3f" % ok_rows.float().mean().item())
    assert ok_rows.float().mean().item() > 0.9
    assert torch.allclose(zf[:, ok_rows], z[:, ok_rows], rtol=1e-3, atol=1e-3)
    assert (lengths >= 1).all() and (lengths <= N).all()


def test_fused_vae_chunking_is_invisible():
    m = _model(512, 20)
    B, N = 40, 40
    z0, _ = _latent(m, B, 13)
    a = FusedVAEDecoder(m, B, N, temperature=0.7, chunk=16, early_exit=False).run(seed=4, z=z0, return_z=True)
    b = FusedVAEDecoder(m, B, N, temperature=0.7, chunk=40, early_exit=False).run(seed=4, z=z0, return_z=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_fused_vae_early_exit():
    m = _model(512, 20, eos_bias=6.0)
    B, N = 40, 64
    z0, _ = _latent(m, B, 14)
    dec = FusedVAEDecoder(m, B, N, temperature=1.0, chunk=16, early_exit=True)
    s, ln = dec.run(seed=5, z=z0)
    assert dec.steps_run < N, dec.steps_run
    full = FusedVAEDecoder(m, B, N, temperature=1.0, chunk=16, early_exit=False)
    sf, lf = full.run(seed=5, z=z0)
    assert full.steps_run == N
    torch.cuda.synchronize()
    assert torch.equal(s, sf) and torch.equal(ln, lf)
    pad = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0], device=DEV)
    for r in range(B):
        assert s[r, ln[r] - 1, 4] == 1 or ln[r] == N
        assert (s[r, ln[r]:] == pad).all()


def test_fused_vae_prefix():
    m = _model(256, 20)
    B, N = 24, 20
    z0, _ = _latent(m, B, 15)
    prefix = _strokes(N, B, 16).transpose(0, 1).contiguous().to(DEV)      # [B, 20, 5]
    plen = torch.tensor([0, 3, 20] * (B // 3), device=DEV)
    dec = FusedVAEDecoder(m, B, N, temperature=0.6, early_exit=False)
    s0, l0, zf0 = dec.run(seed=6, z=z0, return_z=True)
    s, ln, zf = dec.run(seed=6, z=z0, prefix=prefix, prefix_len=plen, return_z=True)
    torch.cuda.synchronize()
    free = plen == 0
    assert torch.equal(s[free], s0[free]) and torch.equal(ln[free], l0[free]) and torch.equal(zf[:, free], zf0[:, free])
    for b in range(B):
        P = int(plen[b])
        assert torch.equal(s[b, :P], prefix[b, :P])
    assert not torch.equal(s[plen == 3], s0[plen == 3])
    # a full-length prefix is teacher forcing on [S0, prefix]
    xs = torch.zeros(N, B, 5, device=DEV)
    xs[0, :, 2] = 1.0
    xs[1:] = prefix.transpose(0, 1)[: N - 1]
    zt = dec.forced(xs, z=z0)
    whole = plen == 20
    assert torch.equal(zf[:, whole], zt[:, whole])
    bad = prefix.clone()
    bad[1, 2, 2:] = torch.tensor([0.0, 0.0, 1.0], device=DEV)      # row 1 (prefix_len 3) ends at stroke 2
    with pytest.raises(ValueError):
        dec.run(seed=6, z=z0, prefix=bad, prefix_len=plen)
    bad[1, 2] = prefix[1, 2]
    bad[1, 5, 2:] = torch.tensor([0.0, 0.0, 1.0], device=DEV)      # past row 1's length: ignored
    s2, _ = dec.run(seed=6, z=z0, prefix=bad, prefix_len=plen)
    assert torch.equal(s2, s)


def test_fused_vae_deterministic_and_seeded():
    m = _model(512, 20)
    B, N = 64, 50
    z0, _ = _latent(m, B, 17)
    dec = FusedVAEDecoder(m, B, N, temperature=0.3)
    a, la = dec.run(seed=1, z=z0)
    b, lb = dec.run(seed=1, z=z0)
    c, _ = dec.run(seed=2, z=z0)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert not torch.equal(a, c)
    for r in range(B):   # finished rows emit end-of-sketch padding
        assert torch.all(a[r, la[r]:, 4] == 1)
    # z drawn from the seed, as GraphDecoder.run does
    d, _ = dec.run(seed=1)
    g = torch.Generator(device=DEV).manual_seed(1)
    e, _ = dec.run(seed=1, z=torch.randn((B, m.cfg.z_size), device=DEV, generator=g))
    assert torch.equal(d, e)


def test_fused_vae_rejects_ineligible_models():
    m = SketchVAE(VAEConfig(dec_model="layer_norm", enc_rnn_size=64, dec_rnn_size=512), seed=0).to(DEV)
    with pytest.raises(ValueError):
        FusedVAEDecoder(m, 4, 4)
