"""Fused whole-sketch decoder for LayerNorm-LSTM VAE decoders
(csrc/decode_vae_ln.hip, sketch_rnn_amd/sample/fused.py FusedLNVAEDecoder):

* teacher-forced head outputs against the fp32 PyTorch step oracle
  (``SketchVAE.decode_step`` in a loop): H 512 and 256, conditional /
  unconditional / class-conditional, one row block / several / a batch split
  over two launches, the widest head;
* rows do not see each other (the statistics exchange is per row): the same
  rows in a larger batch give the same bits;
* NaN-filling every in-launch hand-off buffer changes no bit (no read
  precedes its write);
* sampled strokes against the PyTorch transcription of the sampler applied to
  the kernel's own head outputs, and the kernel re-run teacher-forced on its
  own samples reproduces those head outputs;
* launching the steps in chunks, and leaving early once every row has ended,
  change no bit of the result;
* per-row stroke prefixes; determinism and seeding; the factory.

The model (tests/test_decode_vae_ln.py ``make_model``) is random-init with
``init_w`` x30, ``output_b`` ~ N(0, 0.1) and every layer-norm gain / shift
drawn per gate and unit, so a gate or unit mix-up shows.
"""
import functools

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import fused as F
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.sample.fused import (FusedLNVAEDecoder, FusedVAEDecoder, fused_vae_decoder, fused_vae_kind,
                                         fused_vae_ln_ok)
from test_decode_vae_ln import errors, make_inputs, make_latent, make_model, step_oracle, transcription_forced

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _restore():
    yield
    F.LN_DECODE_POISON = False
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    from sketch_rnn_amd.ops.recurrent import check_cluster_errors
    torch.cuda.synchronize()
    check_cluster_errors(DEV)


@functools.lru_cache(maxsize=None)
def _model(H, M, kind="cond", seed=3, eos_bias=0.0):
    m = make_model(H, M, kind, seed, eos_bias).to(DEV).eval()
    assert fused_vae_ln_ok(m)
    return m


def _latent(m, B, seed):
    return make_latent(m, B, seed, DEV)


def _strokes(N, B, seed):
    """[N, B, 5] pen-down / pen-up strokes (no end of sketch)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, B, 5)
    x[..., :2] = torch.randn(N, B, 2, generator=g) * 0.6
    pen = torch.multinomial(torch.tensor([0.8, 0.2]), N * B, replacement=True, generator=g).view(N, B)
    x[..., 2:4] = torch.nn.functional.one_hot(pen, 2).float()
    return x


@pytest.mark.parametrize("H,M,kind,B,N", [
    (512, 20, "cond", 37, 30),      # two row blocks, the second partial
    (256, 20, "uncond", 5, 12),     # MTW = 1, z_in = 0
    (512, 20, "class", 20, 10),     # labels and the wider zc
    (512, 20, "cond", None, 6),     # rows of one launch + 6: a second launch, row0
    (256, 32, "cond", 40, 20),      # widest head
])
def test_fused_ln_forced_matches_step_oracle(H, M, kind, B, N):
    """Bounds: the plain decoder's (relative Frobenius error < 1e-2, max error
    < 5 % of max |z|), which the kernel meets on every case.

    Measured on MI355X, kernel vs fp32 oracle | PyTorch transcription of the
    kernel's arithmetic (``ln_decode_step_transcription``) vs the same oracle
    on the same inputs (rel, max):

    ==================  ===================  ===================  =========
    case                kernel               transcription        max |z|
    ==================  ===================  ===================  =========
    512 cond  37 x 30   3.552e-3 / 1.183e-2  3.557e-3 / 1.241e-2  1.853
    256 unc.   5 x 12   5.102e-3 / 1.111e-2  5.102e-3 / 1.111e-2  1.453
    512 class 20 x 10   3.223e-3 / 6.089e-3  3.223e-3 / 6.089e-3  1.825
    512 cond 230 x  6   3.045e-3 / 6.170e-3  3.045e-3 / 6.170e-3  2.105
    256 M32   40 x 20   2.704e-3 / 4.594e-3  2.703e-3 / 4.594e-3  1.685
    ==================  ===================  ===================  =========

    The kernel is as far from the oracle as its transcription is: the error
    is the bf16 rounding of W_h, W_out and the carried h. Kernel against
    transcription: rel 5e-6 .. 6e-4.
    """
    m = _model(H, M, kind)
    if B is None:
        B = FusedLNVAEDecoder(m, 64, N).rows + 6
    dec = FusedLNVAEDecoder(m, B, N)
    assert B <= dec.rows or len(range(0, B, dec.rows)) == 2
    xs = make_inputs(N, B, B * 7 + N).to(DEV)
    z, labels = _latent(m, B, 11)
    zk = dec.forced(xs, z=z, labels=labels)
    zo = step_oracle(m, xs, z, labels)
    zt = transcription_forced(m, xs, z, labels)
    torch.cuda.synchronize()
    rel, err, top = errors(zk, zo)
    trel, terr, _ = errors(zt, zo)
    krel, kerr, _ = errors(zk, zt)
    print("H %d M %d %s B %d N %d: kernel rel %.3e max %.3e | transcription rel %.3e max %.3e | of %.3e | "
          "kernel vs transcription rel %.3e max %.3e" % (H, M, kind, B, N, rel, err, trel, terr, top, krel, kerr))
    assert torch.isfinite(zk).all()
    assert rel < 1e-2 and err < 0.05 * top, (rel, err, top)


def test_fused_ln_rows_do_not_see_each_other():
    m = _model(512, 20)
    N = 12
    xs = make_inputs(N, 40, 77).to(DEV)
    z, _ = _latent(m, 40, 21)
    za = FusedLNVAEDecoder(m, 40, N).forced(xs, z=z)
    # rows 16..23: a full 16-row tile of a 32-row block there, a partial one here
    zb = FusedLNVAEDecoder(m, 24, N).forced(xs[:, :24].contiguous(), z=z[:24].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(za).all()
    assert torch.equal(za[:, :24], zb)


def test_fused_ln_no_read_before_its_write():
    m = _model(512, 20)
    B, N = 40, 24
    z0, _ = _latent(m, B, 22)
    F.LN_DECODE_POISON = False
    a = FusedLNVAEDecoder(m, B, N, temperature=0.7, chunk=8, early_exit=False).run(seed=3, z=z0, return_z=True)
    F.LN_DECODE_POISON = True
    b = FusedLNVAEDecoder(m, B, N, temperature=0.7, chunk=8, early_exit=False).run(seed=3, z=z0, return_z=True)
    F.LN_DECODE_POISON = False
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert not torch.isnan(x.float()).any() and not torch.isnan(y.float()).any()
        assert torch.equal(x, y)


def test_fused_ln_samples_match_sampler_transcription():
    m = _model(512, 20)
    B, N, temp, Mx = 48, 40, 0.5, 20
    z0, _ = _latent(m, B, 12)
    strokes, lengths, z = FusedLNVAEDecoder(m, B, N, temperature=temp, early_exit=False).run(seed=9, z=z0,
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
    zf = FusedLNVAEDecoder(m, B, N, temperature=temp).forced(xs, z=z0)
    ok_rows = same.all(1)
    print("rows agreeing throughout %.3f" % ok_rows.float().mean().item())
    assert ok_rows.float().mean().item() > 0.9
    # Bound. The re-drawn offsets differ from the kernel's by fp32 rounding
    # (1 ulp, 2.4e-7 measured). Such a difference reaches z only where it
    # tips the bf16 rounding of a unit of h: a perturbation of one bf16 ulp
    # of that unit, at most twice the rounding error EVERY unit of h carries
    # at EVERY step against the fp32 oracle. The oracle test bounds the sum
    # of all of those at rel 1e-2 / 5 % of max |z|, so the rare tipped
    # roundings stay within the same bounds, while a wrong hand-off of x
    # (stale, shifted by a step, columns mixed) changes z at order 1. The
    # plain decoder's elementwise 1e-3 does not carry over: the gate layer
    # norm multiplies a tipped ulp by rstd * gamma (~4 here) before it
    # recurs. Measured: max 1.7e-3 (0.09 % of max |z|), rel 1.2e-4.
    rel, err, top = errors(zf[:, ok_rows], z[:, ok_rows])
    print("forced on own draws: rel %.3e max %.3e of %.3e, max stroke diff %.3e"
          % (rel, err, top, (strokes[same] - ref[same]).abs().max().item()))
    assert rel < 1e-2 and err < 0.05 * top, (rel, err, top)
    assert (lengths >= 1).all() and (lengths <= N).all()


def test_fused_ln_chunking_is_invisible():
    m = _model(512, 20)
    B, N = 40, 40
    z0, _ = _latent(m, B, 13)
    a = FusedLNVAEDecoder(m, B, N, temperature=0.7, chunk=16, early_exit=False).run(seed=4, z=z0, return_z=True)
    b = FusedLNVAEDecoder(m, B, N, temperature=0.7, chunk=40, early_exit=False).run(seed=4, z=z0, return_z=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_fused_ln_early_exit():
    m = _model(512, 20, eos_bias=6.0)
    B, N = 40, 64
    z0, _ = _latent(m, B, 14)
    dec = FusedLNVAEDecoder(m, B, N, temperature=1.0, chunk=16, early_exit=True)
    s, ln = dec.run(seed=5, z=z0)
    assert dec.steps_run < N, dec.steps_run
    full = FusedLNVAEDecoder(m, B, N, temperature=1.0, chunk=16, early_exit=False)
    sf, lf = full.run(seed=5, z=z0)
    assert full.steps_run == N
    torch.cuda.synchronize()
    assert torch.equal(s, sf) and torch.equal(ln, lf)
    pad = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0], device=DEV)
    for r in range(B):
        assert s[r, ln[r] - 1, 4] == 1 or ln[r] == N
        assert (s[r, ln[r]:] == pad).all()


def test_fused_ln_prefix():
    m = _model(256, 20)
    B, N = 24, 20
    z0, _ = _latent(m, B, 15)
    prefix = _strokes(N, B, 16).transpose(0, 1).contiguous().to(DEV)      # [B, 20, 5]
    plen = torch.tensor([0, 3, 20] * (B // 3), device=DEV)
    dec = FusedLNVAEDecoder(m, B, N, temperature=0.6, early_exit=False)
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


def test_fused_ln_deterministic_and_seeded():
    m = _model(512, 20)
    B, N = 64, 50
    z0, _ = _latent(m, B, 17)
    dec = FusedLNVAEDecoder(m, B, N, temperature=0.3)
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


def test_fused_vae_decoder_factory():
    ln = _model(256, 20)
    plain = SketchVAE(VAEConfig(dec_model="lstm", enc_rnn_size=64, dec_rnn_size=256, num_mixture=20), seed=0).to(DEV)
    hyper = SketchVAE(VAEConfig(dec_model="hyper", enc_rnn_size=64, dec_rnn_size=256, num_mixture=20,
                                hyper_num_units=16, hyper_embedding_size=4), seed=0).to(DEV)
    assert fused_vae_kind(ln) == "layer_norm" and fused_vae_kind(plain) == "lstm" and fused_vae_kind(hyper) is None
    d = fused_vae_decoder(ln, 4, 6, temperature=0.5)
    assert type(d) is FusedLNVAEDecoder
    s, lens = d.run(seed=1)
    torch.cuda.synchronize()
    assert s.shape == (4, 6, 5) and torch.isfinite(s).all()
    assert type(fused_vae_decoder(plain, 4, 6)) is FusedVAEDecoder
    with pytest.raises(ValueError):
        fused_vae_decoder(hyper, 4, 6)
    with pytest.raises(ValueError):
        FusedLNVAEDecoder(plain, 4, 6)
