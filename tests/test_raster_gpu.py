"""The rasteriser kernels (csrc/raster.hip) on the GPU: images against the
fp64 transcription under the rule of tests/fp64_rule.py, the bit-identity of
culling, repeats, poisoned padding, stroke-5 input, ``out=`` and a captured
graph, and the decoder's device output against the same sketches taken
through the host."""
import functools

import numpy as np
import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.data.strokes import to_big_strokes, to_normal_strokes
from sketch_rnn_amd.data.synthetic import synthetic_corpus
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.ops import raster as R
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.utils import native

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _report():
    import fp64_rule
    yield
    fp64_rule.report("rasteriser (csrc/raster.hip)")


@pytest.fixture(autouse=True)
def _restore():
    yield
    R.CULL = True
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")


@functools.lru_cache(None)
def _sketches():
    return synthetic_corpus(64, seed=0, max_len=250)[0]


def _pad(sk, N):
    x = np.zeros((len(sk), N, 3), np.float32)
    for i, s in enumerate(sk):
        x[i, :len(s)] = s
    return torch.tensor(x), torch.tensor([len(s) for s in sk], dtype=torch.int64)


def _corpus(B, N):
    """B corpus sketches of at most N rows; below the corpus' own N the last
    one is a longer sketch cut to exactly N rows (its last segment sits at the
    table's last index)."""
    sk = [s for s in _sketches() if len(s) <= N][:B]
    if N < 250:
        sk[-1] = next(s for s in _sketches() if len(s) > N)[:N]
    assert len(sk) == B and max(len(s) for s in sk) == N
    return _pad(sk, N)


def _walk(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, generator=g)
    x[..., 2] = (torch.rand(B, N, generator=g) < 0.1).float()
    return x, torch.tensor([N] + [N - 43] * (B - 1), dtype=torch.int64)[:B]


EDGE = torch.tensor([[[9.0, 9.0, 0.0]] * 4,                                       # length 0
                     [[2.0, 2.5, 0.0], [4.0, 0.0, 1.0], [9.0, 9.0, 0.0], [9.0, 9.0, 0.0]],   # length 1
                     [[2.0, 2.5, 0.0], [4.0, 0.0, 1.0], [9.0, 9.0, 0.0], [9.0, 9.0, 0.0]]])  # length 2
EDGE2 = torch.tensor([[[2.0, 0.0, 0.0], [0.0, 0.0, 1.0], [9.0, 9.0, 0.0], [9.0, 9.0, 0.0]],  # a dot
                      [[2.0, 2.5, 1.0], [4.0, 0.0, 1.0], [9.0, 9.0, 0.0], [9.0, 9.0, 0.0]],  # lifted: blank
                      [[2.0, 2.5, 0.0], [4.0, 0.0, 0.0], [-1.0, 3.0, 1.0], [-5.0, 0.5, 1.0]]])   # length N, one move

# name: (inputs, size, width, corpus case?)
CASES = {
    "minimal": (lambda: (torch.tensor([[[3.0, 1.0, 0.0]]]), torch.tensor([1])), 8, 1.0, False),
    "edge": (lambda: (EDGE, torch.tensor([0, 1, 2])), 8, 1.0, False),
    "edge2": (lambda: (EDGE2, torch.tensor([2, 2, 4])), 8, 1.0, False),
    "wave+1": (lambda: _corpus(8, 65), 28, 1.0, True),
    "workload": (lambda: _corpus(8, 250), 64, 1.5, True),
    "odd-size": (lambda: _corpus(5, 250), 33, 1.0, True),
    "chunk2": (lambda: _walk(2, 300, seed=7), 16, 1.0, False),
}


def _three(x, L, S, width, frame=None):
    """(q64, q32, qk) images and frames of one call."""
    q64 = R.rasterize_torch(x, L, size=S, width=width, frame=frame)
    q32 = R.rasterize_torch(x, L, size=S, width=width, frame=frame, dtype=torch.float32)
    fk = None if frame is None else frame.to(DEV)
    qk = R.rasterize_hip(x.to(DEV), L.to(DEV), size=S, width=width, frame=fk)
    assert qk[0].dtype == torch.float32 and qk[0].shape == (x.shape[0], S, S) and qk[1].shape == (x.shape[0], 3)
    return q64, q32, tuple(t.cpu() for t in qk)


def _inked(q64):
    return (q64 > 0).double().mean((1, 2))


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_fp64(name):
    import fp64_rule
    make, S, width, corpus = CASES[name]
    x, L = make()
    q64, q32, qk = _three(x, L, S, width)
    if corpus:      # a blank output cannot pass
        assert float(_inked(q64[0]).min()) > 0.01
    print("%s: inked share of the fp64 images %s" % (name, [round(v, 4) for v in _inked(q64[0]).tolist()]))
    fp64_rule.check("image " + name, qk[0], q32[0], q64[0], margin=4.0)
    fp64_rule.check("frame " + name, qk[1], q32[1], q64[1], margin=4.0)
    if name == "edge":
        assert float(qk[0][:2].abs().max()) == 0.0 and float(qk[0][2].max()) > 0.5
        assert qk[1][0].tolist() == [1.0, 4.0, 4.0]
    if name == "edge2":
        assert abs(float(qk[0][0].sum()) - 1.17) < 0.005 and float(qk[0][1].abs().max()) == 0.0


def test_kernel_given_frame_clips():
    """A given frame of twice the fitted scale about the canvas centre: half the drawing is clipped."""
    import fp64_rule
    x, L = _corpus(4, 250)
    _, fit = R.rasterize_hip(x.to(DEV), L.to(DEV), size=64)
    fit = fit.cpu()
    frame = torch.stack([2 * fit[:, 0], 2 * fit[:, 1] - 32.0, 2 * fit[:, 2] - 32.0], dim=1)
    q64, q32, qk = _three(x, L, 64, 1.0, frame=frame)
    assert float(_inked(q64[0]).min()) > 0.01
    assert torch.equal(qk[1], frame)
    fp64_rule.check("image given frame", qk[0], q32[0], q64[0], margin=4.0)
    fitted64, _ = R.rasterize_torch(x, L, size=64)
    assert float((fitted64 - q64[0]).abs().max()) > 0.5          # it is another image


@pytest.mark.parametrize("B,N,S,width", [(5, 250, 33, 1.0), (8, 250, 64, 1.5)])
def test_cull_changes_no_bit(B, N, S, width):
    x, L = (t.to(DEV) for t in _corpus(B, N))
    a, fa = R.rasterize_hip(x, L, size=S, width=width)
    again, _ = R.rasterize_hip(x, L, size=S, width=width)
    R.CULL = False
    b, fb = R.rasterize_hip(x, L, size=S, width=width)
    assert torch.equal(a, again)                                  # two runs are bit-identical
    assert torch.equal(a, b) and torch.equal(fa, fb)
    assert float(a.max()) > 0.5


def test_padding_stroke5_out_and_frame():
    sk = [s for s in _sketches() if len(s) <= 100][:6]
    x, L = (t.to(DEV) for t in _pad(sk, 100))
    a, fa = R.rasterize(x, L, size=33, width=1.5)
    assert a.is_cuda and a.dtype == torch.float32
    poisoned = x.clone()
    for i, n in enumerate(L.tolist()):
        poisoned[i, n:] = float("nan")
    b, fb = R.rasterize(poisoned, L, size=33, width=1.5)
    assert torch.equal(a, b) and torch.equal(fa, fb)              # rows past lengths change nothing
    x5 = torch.tensor(np.stack([to_big_strokes(s, 100) for s in sk]), device=DEV)
    for lens in (None, L):
        c, fc = R.rasterize(x5, lens, size=33, width=1.5)
        assert torch.equal(a, c) and torch.equal(fa, fc)          # stroke-5 equals stroke-3
    out = torch.full((6, 33, 33), 7.0, device=DEV)
    d, _ = R.rasterize(x, L, size=33, width=1.5, out=out)
    assert d is out and torch.equal(out, a)                       # out= is filled in place
    e, fe = R.rasterize(x, L, size=33, width=1.5, frame=fa)
    assert torch.equal(a, e) and torch.equal(fa, fe)              # the returned frame reproduces the call
    with pytest.raises(ValueError):
        R.rasterize(x, L, size=33, frame=torch.zeros(6, 3, device=DEV))
    with pytest.raises(ValueError):
        R.rasterize_hip(x.cpu(), L.cpu(), size=33)


def test_sizes_1_and_512_and_empty():
    x, L = (t.to(DEV) for t in _corpus(2, 250))
    a, _ = R.rasterize(x, L, size=1, pad=0.0)
    assert a.shape == (2, 1, 1) and bool(torch.isfinite(a).all())
    import fp64_rule
    short = _pad([s for s in _sketches() if len(s) <= 40][:1], 40)     # 1024 tiles; few segments keep the oracle quick
    q64, q32, qk = _three(short[0], short[1], 512, 2.0)
    fp64_rule.check("image S=512", qk[0], q32[0], q64[0], margin=4.0)
    e, fe = R.rasterize(torch.zeros(2, 0, 3, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), size=8)
    assert float(e.abs().max()) == 0.0 and fe.tolist() == [[1.0, 4.0, 4.0]] * 2


def test_graph_capture_replays_the_eager_call():
    x, L = (t.to(DEV) for t in _corpus(4, 65))
    eager, feager = R.rasterize(x, L, size=28)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        R.rasterize(x, L, size=28)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        img, frame = R.rasterize(x, L, size=28)
    img.fill_(7.0)
    frame.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(img, eager) and torch.equal(frame, feager)


def test_decoder_output_rasterised_where_it_lies():
    """The GraphDecoder's device [4, 32, 5] output through ``rasterize`` equals
    the same sketches taken through the host (``to_normal_strokes``, padding),
    on the rows where the two length rules agree (all but an end-of-sketch in
    row 0)."""
    native.require_hip()
    ops.set_backend("hip")
    ops.set_compute_dtype("bf16")
    cfg = VAEConfig(enc_rnn_size=64, dec_rnn_size=256, z_size=16, dec_model="lstm", num_classes=0, max_seq_len=32)
    m = SketchVAE(cfg, seed=3).to(DEV).eval()
    with torch.no_grad():
        m.output_b[2] += -1.0          # p3 ~ 6 % per stroke at temperature 0.5: sketches of some length
    z = torch.randn(4, cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    s, _ = SM.GraphDecoder(m, batch=4, steps=32, temperature=0.5).run(seed=3, z=z)
    assert s.is_cuda and s.shape == (4, 32, 5)
    img, frame = R.rasterize(s.float())
    host = [to_normal_strokes(r) for r in s.cpu().numpy()]
    agree = R.stroke5_lengths(s).cpu() == torch.tensor([len(h) for h in host])
    assert int(agree.sum()) >= 2, agree
    x3, L3 = (t.to(DEV) for t in _pad(host, 32))
    img3, frame3 = R.rasterize(x3, L3)
    assert torch.equal(img[agree], img3[agree]) and torch.equal(frame[agree], frame3[agree])
    assert float(img[agree].max()) > 0.5
