"""The rounding-faithful references of tests/bf16_faithful.py, proved on the
CPU before tests/test_bf16_faithful_gpu.py holds the bf16 kernels to them.

``rounded=False`` in fp64: every scan's forward equals the torch-backend
oracle run in fp64 (``ops.lstm_sequence`` with resets and with LayerNorm,
``ops.bilstm_sequence_packed``, the 2-layer ``SketchRNN`` stack, ``Encoder``
with ``lengths``) and its hand-written backward equals autograd of that
oracle, to fp64 rounding: ``2^-53 * 2^16`` of the tensor's largest element
(sums of at most T * B * H = 1280 terms chained over T = 4 steps each way;
any wrong term is ten orders of magnitude above that).

``rounded=True``: fp32 and fp64 arithmetic agree within the bf16 noise
``max|rounded - exact|`` (they differ only where a bf16 rounding flips on a
last-bit difference), and that noise is non-zero for every quantity -- a
``rounded`` flag that does nothing fails here.
"""
import functools

import pytest
import torch

import bf16_faithful as F
from sketch_rnn_amd import ops

F64_TOL = 2.0 ** -53 * 2.0 ** 16
T, B, H = 4, 5, 64
KEEP = 0.9


@pytest.fixture(autouse=True)
def _torch_backend():
    ops.set_backend("torch")
    yield
    ops.set_backend("auto")


@functools.lru_cache(maxsize=None)
def _stack_model():
    from sketch_rnn_amd.config import RefConfig
    from sketch_rnn_amd.models.reference import SketchRNN
    return SketchRNN(RefConfig(rnn_size=H, num_layers=2, num_mixture=2, keep_prob=1.0), seed=1)


@functools.lru_cache(maxsize=None)
def _encoder():
    from sketch_rnn_amd.config import VAEConfig
    from sketch_rnn_amd.models.vae import Encoder
    cfg = VAEConfig(enc_rnn_size=H, dec_rnn_size=H, z_size=8, max_seq_len=T, batch_size=B)
    enc = Encoder(cfg, torch.Generator().manual_seed(2))
    with torch.no_grad():   # (the initial 0.001 / zero heads would leave the head gradients degenerate)
        g = torch.Generator().manual_seed(3)
        for p in (enc.mu_w, enc.sig_w, enc.mu_b, enc.sig_b, enc.fw.bias, enc.bw.bias):
            p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return enc


@functools.lru_cache(maxsize=None)
def _case(name):
    """``(oracle, scan)``: ``oracle()`` is the torch backend in fp64 with
    autograd, ``scan(dtype, rounded)`` the reference under test."""
    if name in ("lstm_reset", "ln_lstm", "bilstm"):
        nd = 2 if name == "bilstm" else 1
        inp = F.seq_inputs(T, B, H, nd, "cpu", reset=name == "lstm_reset", ln=name == "ln_lstm")
        return (lambda: F.run_seq_ops(inp, nd, KEEP, torch.float64),
                lambda dt, r: F.run_seq_scan(inp, nd, KEEP, dt, r))
    if name == "stack":
        m = _stack_model()
        inp = F.stack_inputs(m, B, T, "cpu")
        return (lambda: F.run_stack_ops(m, inp, torch.float64), lambda dt, r: F.run_stack_scan(m, inp, dt, r))
    enc = _encoder()
    inp = F.encoder_inputs(T, B, 8, [T, 1, 3, 2, T], "cpu")
    return (lambda: F.run_encoder_ops(enc, inp, torch.float64), lambda dt, r: F.run_encoder_scan(enc, inp, dt, r))


CASES = ["lstm_reset", "ln_lstm", "bilstm", "stack", "encoder"]
# the head biases' gradients are column sums of the loss weights: no recurrence, no rounding in them
NO_RECURRENCE = {"dmu_b", "dsig_b"}


def _maxabs(t):
    return float(t.detach().double().abs().max())


@pytest.mark.parametrize("name", CASES)
def test_exact_scan_equals_the_fp64_oracle_and_its_autograd(name):
    oracle, scan = _case(name)
    ref, got = oracle(), scan(torch.float64, False)
    assert set(ref) == set(got), (sorted(ref), sorted(got))
    for k in sorted(ref):
        assert ref[k].dtype == got[k].dtype == torch.float64, k
        assert ref[k].shape == got[k].shape, (k, ref[k].shape, got[k].shape)
        err, top = _maxabs(got[k] - ref[k]), _maxabs(ref[k])
        assert top > 0.0, k
        assert err <= F64_TOL * top, "%s: |scan - oracle| %.3e of %.3e" % (k, err, top)


@pytest.mark.parametrize("name", CASES)
def test_rounded_scans_agree_within_the_bf16_noise_and_the_noise_is_real(name):
    _, scan = _case(name)
    exact, r64, r32 = scan(torch.float64, False), scan(torch.float64, True), scan(torch.float32, True)
    for k in sorted(exact):
        assert r32[k].dtype == torch.float32, k
        noise = _maxabs(r64[k] - exact[k])
        if k in NO_RECURRENCE:
            assert noise == 0.0, k
            continue
        assert noise > 0.0, "%s: the rounded scan equals the exact one" % k
        diff = _maxabs(r32[k].double() - r64[k])
        assert diff <= noise, "%s: |fp32 - fp64| %.3e > bf16 noise %.3e" % (k, diff, noise)


def test_rounding_is_to_bf16():
    t = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -9, 3.0e-5], dtype=torch.float64)
    r = F.bf16(t)
    assert r.dtype == torch.float64
    assert r[0] == 1.0 and r[1] == 1.0 + 2.0 ** -7   # ties to even, 8 significant bits
    assert F.bf16(t, False) is t
