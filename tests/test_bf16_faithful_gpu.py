"""The bf16 LSTM kernels against the rounding-faithful fp64 reference.

Every quantity -- forward outputs, final states, every gradient -- is computed
three ways on the same inputs: ``q64`` (the exact scan of
tests/bf16_faithful.py in fp64), ``qb`` (the same scan in fp32 with a bf16
rounding at each point where the host code hands bf16 to a kernel; a
transcription, not the code under test) and ``qk`` (the kernels: hip
backend, bf16 compute). The rule of tests/fp64_rule.py with its margin of 4,

    max|qk - q64| <= 4 * max|qb - q64| + 4 * 2^-24 * max|q64|,

is applied slice by slice, each against its own ``max|q64|``: outputs and
``dxp`` per time step and per block of 32 rows (per direction), weight and
bias gradients per gate column group (per direction), initial / final /
reset-state quantities per row block, LayerNorm and latent-head parameter
gradients per tensor. A kernel that rounds where the table in
tests/bf16_faithful.py says it does has the transcription's error up to
roundings that flip on a last-bit difference (under 0.5 of that error on the
CPU); a wrong row, step, mask or term moves it by tens to thousands of times.
No bound here comes from what a kernel was seen to give.

``|qk - qb| / max|qb - q64|`` is recorded next to each quantity (the
``|k-b|`` rows of the report; second figure: its share of the bound) and not
asserted: it tells arithmetic noise from a rounding in another place.
The committed report: profiles/r17/bf16_faithful/ratios.txt.
"""
import functools
import math

import pytest
import torch

import bf16_faithful as F
import fp64_rule as R
from sketch_rnn_amd import ops
from sketch_rnn_amd.ops import persist, recurrent

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = 32
KEEP = 0.9


@pytest.fixture(autouse=True)
def _restore():
    saved = (persist.PERSIST_ENABLED, persist.BI_ENCODER, persist.lstm_stack, persist.bilstm_last_h,
             recurrent.LN_CHAIN, recurrent.LN_SAVES_LP, recurrent.PERSIST_LENGTHS)
    yield
    (persist.PERSIST_ENABLED, persist.BI_ENCODER, persist.lstm_stack, persist.bilstm_last_h,
     recurrent.LN_CHAIN, recurrent.LN_SAVES_LP, recurrent.PERSIST_LENGTHS) = saved
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    torch.cuda.synchronize()
    recurrent.check_cluster_errors(DEV)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    R.report("bf16 LSTM kernels vs the rounding-faithful scans (tests/bf16_faithful.py)")


def _spy(name):
    """Count the calls of ``persist.<name>`` (the fixture puts it back)."""
    calls, orig = [0], getattr(persist, name)

    def spy(*a, **k):
        calls[0] += 1
        return orig(*a, **k)
    setattr(persist, name, spy)
    return calls


# ---- the rule, slice by slice ---------------------------------------------------------------------
_GATED = ("W_x", "W_h", "bias", "dW", "db0", "db1", "dW_h0", "dW_h1", "dW_in1", "dW_x0")
_WHOLE = ("dln_gamma", "dln_beta", "dlnc_gamma", "dlnc_beta", "dmu_w", "dmu_b", "dsig_w", "dsig_b")


def _slices(key, t, B):
    """``(label, index)`` of the slices of quantity ``key`` (see the module
    docstring); ``B``: rows per direction."""
    if key in _WHOLE:
        yield "", (Ellipsis,)
    elif key.endswith(_GATED):
        n = t.shape[-1] // 4
        for d in (range(t.shape[0]) if t.dim() == 3 else [None]):
            for q in range(4):
                cols = slice(q * n, (q + 1) * n)
                yield "dir %s gate %d" % (d, q), ((d, slice(None), cols) if d is not None else (Ellipsis, cols))
    else:   # [T, nd*B, X] or [nd*B, X]: row blocks of every direction, per time step
        rows = t.shape[-2]
        assert rows % B == 0, (key, t.shape, B)
        blocks = [(g, r0) for g in range(rows // B) for r0 in range(0, B, ROWS)]
        for ts in (range(t.shape[0]) if t.dim() == 3 else [None]):
            for g, r0 in blocks:
                rs = slice(g * B + r0, g * B + min(r0 + ROWS, B))
                yield "t %s dir %d rows %d.." % (ts, g, r0), ((ts, rs) if ts is not None else (rs,))


def _check_all(case, qk, qb, q64, B):
    assert set(qk) == set(qb) == set(q64), (sorted(qk), sorted(qb), sorted(q64))
    fails = []
    for key in sorted(q64):
        k, b, r = (q[key].detach().double().cpu() for q in (qk, qb, q64))
        assert qk[key].dtype == qb[key].dtype == torch.float32 and q64[key].dtype == torch.float64, key
        assert k.shape == b.shape == r.shape, (key, k.shape, b.shape, r.shape)
        name = "%s %s" % (case, key)
        for where, idx in _slices(key, r, B):
            ks, bs, rs = k[idx], b[idx], r[idx]
            eb, top = float((bs - rs).abs().max()), float(rs.abs().max())
            dkb = float((ks - bs).abs().max())
            bound = 4.0 * eb + 4.0 * R.EPS32 * top
            R.record(name + " |k-b|", dkb / eb if eb > 0.0 else (0.0 if dkb == 0.0 else math.inf),
                     dkb / bound if bound > 0.0 else (0.0 if dkb == 0.0 else math.inf))
            try:
                R.check(name, ks, bs, rs)
            except AssertionError as e:
                fails.append("[%s] %s" % (where, e))
    assert not fails, "%d slices over the bound:\n%s" % (len(fails), "\n".join(fails))


def _three_ways(run_ops, run_scan):
    ops.set_backend("hip")
    ops.set_compute_dtype("bf16")
    qk = run_ops(torch.float32)
    torch.cuda.synchronize()
    return qk, run_scan(torch.float32, True), run_scan(torch.float64, False)


def _seq_case(case, T, B, H, nd, reset=False, ln=False):
    inp = F.seq_inputs(T, B, H, nd, DEV, reset=reset, ln=ln)
    qk, qb, q64 = _three_ways(lambda dt: F.run_seq_ops(inp, nd, KEEP, dt),
                              lambda dt, r: F.run_seq_scan(inp, nd, KEEP, dt, r))
    _check_all(case, qk, qb, q64, B)


# ---- persistent biLSTM (csrc/lstm_persist.hip, nd = 2) ----------------------------------------------
@pytest.mark.parametrize("H,B,rows", [(512, 33, 32), (512, 129, 64), (256, 1, 32), (256, 65, 32)])
def test_persistent_bilstm(H, B, rows):
    """32-row blocks with a last block of one row; 64-row blocks; one row;
    H = 256 with three blocks."""
    ops.set_compute_dtype("bf16")
    assert persist.persist_ok(H, 2, 1, B=B) and persist.block_rows(H, 2, 1, B) == rows
    calls = _spy("lstm_stack")
    _seq_case("bilstm H%d B%d" % (H, B), 7, B, H, 2)
    assert calls[0] == 1


# ---- fused encoder (models.vae.Encoder -> persist.bilstm_last_h) --------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder(H):
    from sketch_rnn_amd.config import VAEConfig
    from sketch_rnn_amd.models.vae import Encoder
    cfg = VAEConfig(enc_rnn_size=H, dec_rnn_size=H, z_size=16, max_seq_len=7, batch_size=33)
    enc = Encoder(cfg, torch.Generator().manual_seed(2))
    with torch.no_grad():   # heads and biases of ordinary size (the initial ones are 0.001 / zero)
        g = torch.Generator().manual_seed(3)
        for p in (enc.mu_w, enc.sig_w, enc.mu_b, enc.sig_b, enc.fw.bias, enc.bw.bias):
            p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return enc.to(DEV)


_T_ENC, _B_ENC = 7, 33
LENGTHS = {
    "full": [_T_ENC] * _B_ENC,
    "ones": [1] * _B_ENC,
    # rows of length 1 and T in the first block; the lone row of the second block stops after one step
    "mixed": [1, _T_ENC, 3, 1, 5, 2, _T_ENC, 6] * 4 + [1],
}


@pytest.mark.parametrize("lens", ["full", "ones", "mixed"])
@pytest.mark.parametrize("H", [256, 512])
def test_fused_encoder(H, lens):
    """``mu``, ``presig`` and every parameter gradient of the encoder as one
    node: only ``h[len - 1]`` is written, each row block stops after its
    longest row, and the input-projection gradients read the bf16 gate
    gradient."""
    enc = _encoder(H)
    inp = F.encoder_inputs(_T_ENC, _B_ENC, 16, LENGTHS[lens], DEV)
    calls = _spy("bilstm_last_h")
    qk, qb, q64 = _three_ways(lambda dt: F.run_encoder_ops(enc, inp, dt),
                              lambda dt, r: F.run_encoder_scan(enc, inp, dt, r))
    assert calls[0] == 1
    _check_all("encoder H%d %s" % (H, lens), qk, qb, q64, _B_ENC)


# ---- persistent 2-layer stack (SketchRNN.features) --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack_model():
    from sketch_rnn_amd.config import RefConfig
    from sketch_rnn_amd.models.reference import SketchRNN
    return SketchRNN(RefConfig(rnn_size=256, num_layers=2, num_mixture=4, keep_prob=1.0), seed=1).to(DEV)


@pytest.mark.parametrize("B", [1, 33])
def test_persistent_stack(B):
    """Both layers in one launch, layer 1's input product inside the
    recurrence, eoc resets at t = 0 and t = T - 1 among them."""
    m = _stack_model()
    inp = F.stack_inputs(m, B, 5, DEV)
    assert inp["x"][0, 0, 3] > 0 and inp["x"][0, 4, 3] > 0
    calls = _spy("lstm_stack")
    qk, qb, q64 = _three_ways(lambda dt: F.run_stack_ops(m, inp, dt), lambda dt, r: F.run_stack_scan(m, inp, dt, r))
    assert calls[0] == 1
    _check_all("stack B%d" % B, qk, qb, q64, B)


# ---- persistent decoder layer (ops.lstm_sequence, nd = 1, h0 / c0 with gradients) --------------------
@pytest.mark.parametrize("H", [256, 512])
def test_persistent_decoder_layer(H):
    calls = _spy("lstm_stack")
    _seq_case("decoder H%d" % H, 4, 33, H, 1)
    assert calls[0] == 1


# ---- fused per-step kernels (csrc/lstm_fused.hip) ---------------------------------------------------
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("H", [256, 512])
def test_fused_per_step(H, nd, B):
    """One launch per step each way, resets on for nd = 1 (their
    ``reset_h / reset_c`` gradients included)."""
    persist.PERSIST_ENABLED = False
    ops.set_compute_dtype("bf16")
    assert recurrent._fused_ok(H, False, torch.bfloat16)
    calls = _spy("lstm_stack")
    _seq_case("fused H%d nd%d B%d" % (H, nd, B), 3, B, H, nd, reset=nd == 1)
    assert calls[0] == 0


# ---- LayerNorm-LSTM in bf16 ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,chain", [(256, True), (512, True), (256, False), (512, False), (320, True)])
def test_ln_lstm(H, chain):
    """Chained steps (csrc/chain_step.hip), the two-launch path they are
    measured against elsewhere, and H = 320, which the chain refuses (not a
    multiple of 256), on the clustered cells. bf16 saves (LN_SAVES_LP)."""
    T = 4
    recurrent.LN_CHAIN = chain
    assert recurrent.LN_SAVES_LP
    n0, r0 = dict(recurrent.LN_CHAIN_STATS), dict(recurrent.ROW_STATS)
    _seq_case("ln H%d %s" % (H, "chain" if chain else "two-launch"), T, 33, H, 1, ln=True)
    chained = chain and H % 256 == 0
    assert recurrent.LN_CHAIN_STATS["fwd"] - n0["fwd"] == (T if chained else 0)
    assert recurrent.LN_CHAIN_STATS["bwd"] - n0["bwd"] == (T - 1 if chained else 0)
    if H == 320:
        assert recurrent.ROW_STATS["cluster"] - r0["cluster"] == 2 * T
