"""Bulk generation on the GPU: the recycling path of ``StreamDecoder`` (the
slot-map sampler in csrc/decode_step.hip, the refill pair of
csrc/decode_refill.hip, the replayed chunk graph) against the plain
``GraphDecoder`` over the same jobs, bit for bit, and against itself over
slot counts, chunk lengths, graph replay and eager launches."""
import functools

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.sample import stream as ST
from sketch_rnn_amd.utils import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, TEMP, SEED = 24, 0.5, 11
JOB_T = (0.4, 0.5, 0.65)          # [j % 3]: per-job temperatures


@pytest.fixture(autouse=True)
def _mode():
    native.require_hip()
    ops.set_backend("hip")
    ops.set_compute_dtype("bf16")
    yield
    ST.POISON = False
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    from sketch_rnn_amd.ops.recurrent import check_cluster_errors
    torch.cuda.synchronize()
    check_cluster_errors(DEV)


@functools.lru_cache(maxsize=None)
def _model(bias=-1.0):
    """``_hyper256``'s shape (tests/test_sampler_gpu.py) with the end-of-sketch
    bias moved by ``bias``: -1 spreads the lengths over 1..N."""
    cfg = VAEConfig(enc_rnn_size=64, dec_rnn_size=512, z_size=32, dec_model="hyper", hyper_num_units=256,
                    hyper_embedding_size=16, num_classes=0, max_seq_len=N)
    m = SketchVAE(cfg, seed=1).to(DEV).eval()
    with torch.no_grad():
        m.output_b[2] += bias
    return m


@functools.lru_cache(maxsize=None)
def _jobs(J):
    z = torch.randn(700, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))[:J].contiguous()
    return z, torch.tensor(JOB_T, device=DEV)[torch.arange(J, device=DEV) % 3]


@functools.lru_cache(maxsize=None)
def _plain(J, per_job=True, bias=-1.0):
    """The plain decode of the first J jobs (computed once, never modified)."""
    z, t = _jobs(J)
    s, l = SM.GraphDecoder(_model(bias), J, N, TEMP).run(seed=SEED, z=z, temperature=t if per_job else None)
    torch.cuda.synchronize()
    return s, l


def _not_vacuous():
    """The inputs prove something: on the plain decoder at least 8 rows end
    within 5 strokes (slots are refilled early and often) and at least 8 run
    to N (slots end by the length limit, not by a pen state)."""
    for per_job in (True, False):
        l = _plain(128, per_job)[1]
        assert int((l <= 5).sum()) >= 8 and int((l == N).sum()) >= 8, l.tolist()


def _stream(J, slots, chunk=None, use_graph=True, per_job=True, bias=-1.0, **kw):
    z, t = _jobs(J)
    dec = ST.StreamDecoder(_model(bias), slots, N, TEMP, chunk=chunk, use_graph=use_graph)
    assert dec.impl == "recycle"
    s, l = dec.run(z, temperature=t if per_job else None, seed=SEED, **kw)
    torch.cuda.synchronize()
    return dec, s, l


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_oracle_and_counted_steps():
    _not_vacuous()
    for per_job in (True, False):
        dec, s, l = _stream(128, 8, chunk=5, per_job=per_job)
        assert _same((s, l), _plain(128, per_job))
        assert dec.valid_strokes == int(l.sum()) and dec.slot_steps == 8 * dec.steps_run
        assert dec.occupancy == dec.valid_strokes / dec.slot_steps
    # counted, not timed: fewer step launches than the same jobs in 16 plain batches of 8 with the all-done exit
    z, t = _jobs(128)
    plain = SM.GraphDecoder(_model(), 8, N, TEMP, chunk=5, use_graph=False)
    total = 0
    for j0 in range(0, 128, 8):
        _, lb = plain.run(seed=SEED, z=z[j0:j0 + 8], temperature=TEMP, row0=j0)
        total += plain.steps_run
    assert dec.steps_run < total, "stream steps_run %d, 16 plain batches of 8 %d" % (dec.steps_run, total)
    print("steps_run: stream %d, 16 plain batches of 8: %d, occupancy %.3f" % (dec.steps_run, total, dec.occupancy))


def test_schedule_invariance():
    _not_vacuous()
    _, s, l = _stream(300, 8, chunk=5)
    assert int((l <= 5).sum()) >= 8 and int((l == N).sum()) >= 8
    for slots, chunk, graph in ((32, 3, True), (128, 25, True), (8, 25, False), (128, 3, False), (32, 5, False)):
        _, s2, l2 = _stream(300, slots, chunk=chunk, use_graph=graph)
        assert _same((s, l), (s2, l2)), (slots, chunk, graph)
    assert s.shape == (300, N, 5)


def test_wide_decoder_equals_plain_wide_decode():
    _not_vacuous()
    dec, s, l = _stream(256, 256, chunk=5)
    assert _same((s, l), _plain(256))
    assert dec.steps_run <= 30        # one job per slot: N + 1 launches rounded up to the chunk


def test_wide_decoder_chunks():
    _not_vacuous()
    a = _stream(700, 256, chunk=5)
    b = _stream(700, 256, chunk=8)
    assert _same(a[1:], b[1:])
    assert int((a[2] <= 5).sum()) >= 8 and int((a[2] == N).sum()) >= 8


@pytest.mark.parametrize("J,slots", [(5, 8), (9, 8), (1, 8), (37, 32)])
def test_edges_job_counts(J, slots):
    """Fewer jobs than slots (some slots never get one), one job more than
    slots, with N = 24 no multiple of the chunk of 5."""
    _not_vacuous()
    _, s, l = _stream(J, slots, chunk=5)
    assert _same((s, l), _plain(J))


def test_edge_no_jobs():
    dec, s, l = _stream(0, 8, chunk=5)
    assert s.shape == (0, N, 5) and l.shape == (0,) and dec.steps_run == 0


@pytest.mark.parametrize("bias,length", [(-30.0, N), (30.0, 1)])
def test_edges_every_row_same_length(bias, length):
    """A model whose rows all run to N (slots end by the length limit alone),
    and one whose rows all stop at stroke 1 (every chunk refills every slot)."""
    _not_vacuous()
    ref = _plain(37, True, bias)
    assert bool((ref[1] == length).all()), ref[1].tolist()
    _, s, l = _stream(37, 8, chunk=5, bias=bias)
    assert _same((s, l), ref)


def test_poison_prefill_determinism():
    _not_vacuous()
    for J, slots in ((5, 8), (37, 8), (300, 128)):
        dec, s, l = _stream(J, slots, chunk=5)
        z, t = _jobs(J)
        again = dec.run(z, temperature=t, seed=SEED)                  # two runs of one decoder
        assert _same((s, l), again)
        dec.out.fill_(7.0)                                            # whatever the buffer held before
        assert _same((s, l), dec.run(z, temperature=t, seed=SEED))
        ST.POISON = True                                              # idle slots NaN-filled by every refill
        try:
            _, s2, l2 = _stream(J, slots, chunk=5)
            _, s3, l3 = _stream(J, slots, chunk=5, use_graph=False)
        finally:
            ST.POISON = False
        assert _same((s, l), (s2, l2)) and _same((s, l), (s3, l3))
        assert bool(torch.isfinite(s).all())


def test_first_row_and_seed_on_device():
    """``first_row`` and the seed live in device memory: one captured graph
    serves every run. The second part of a split job list, decoded with
    ``first_row``, is the plain decode of those jobs with ``row0`` (the same
    row count on both sides, so the per-job constants come from the same
    products)."""
    _not_vacuous()
    z, t = _jobs(128)
    dec, s, l = _stream(128, 8, chunk=5)
    g = dec._graph
    b = dec.run(z[50:], temperature=t[50:], seed=SEED, first_row=50)
    assert dec._graph is g
    ref = SM.GraphDecoder(_model(), 78, N, TEMP).run(seed=SEED, z=z[50:], temperature=t[50:], row0=50)
    assert _same(b, ref)
    assert int((b[1] <= 5).sum()) >= 5 and int((b[1] == N).sum()) >= 5
    assert not torch.equal(b[0], dec.run(z[50:], temperature=t[50:], seed=SEED)[0])      # the noise rows moved
    c = dec.run(z, temperature=t, seed=SEED + 1)
    assert dec._graph is g and not torch.equal(c[0], s)


def test_row0_is_a_device_word():
    """``GraphDecoder.run(row0=)`` on the stepper path replays the graphs it
    captured for another ``row0``, and gives what a decoder that never saw
    another value gives."""
    z, t = _jobs(16)
    dec = SM.GraphDecoder(_model(), 8, N, TEMP, chunk=5)
    a = dec.run(seed=SEED, z=z[:8], temperature=t[:8])
    graphs = dec.graphs
    assert graphs is not None
    b = dec.run(seed=SEED, z=z[8:], temperature=t[8:], row0=8)
    assert dec.graphs is graphs
    fresh = SM.GraphDecoder(_model(), 8, N, TEMP, chunk=5, use_graph=False).run(seed=SEED, z=z[8:], temperature=t[8:],
                                                                             row0=8)
    assert _same(b, fresh)
    assert not torch.equal(b[0], dec.run(seed=SEED, z=z[8:], temperature=t[8:])[0])
    assert _same(a, dec.run(seed=SEED, z=z[:8], temperature=t[:8], row0=0))


def test_sampler_kernels_row_base():
    """The two sampler kernels with the row offset by value, in the device
    word, and split between both: the same draws, those of rows row0.. of a
    longer launch."""
    import ctypes
    lib = native.require_hip().lib
    B, M, R = 40, 20, 37
    g = torch.Generator(device=DEV).manual_seed(5)
    z = torch.randn(R + B, 3 + 6 * M, device=DEV, generator=g) * 2
    seed = torch.tensor([9], dtype=torch.int64, device=DEV)
    word = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)       # noqa: E731

    def rows(zz, **kw):
        n = zz.shape[0]
        out, nx, done = torch.zeros(n, 5, device=DEV), torch.zeros(n, 5, device=DEV), torch.zeros(n, dtype=torch.int32,
                                                                                                   device=DEV)
        SM.mdn_sample_device(zz, M, 1, 0.5, False, False, seed, 3, out, nx, done, **kw)
        return out, nx, done
    full = rows(z)
    for kw in (dict(row0=R), dict(row_base=word(R)), dict(row0=30, row_base=word(R - 30))):
        for a, b in zip(full, rows(z[R:], **kw)):
            assert torch.equal(a[R:], b), kw
    assert not torch.equal(full[0][R:], rows(z[R:])[0])
    zs = torch.randn(2, B, 128, device=DEV, generator=g)
    bias = torch.randn(128, device=DEV, generator=g) * 0.3

    def slabs(row0, base):
        out, nx, done = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV), torch.zeros(B, dtype=torch.int32,
                                                                                                   device=DEV)
        rc = lib.skr_mdn_sample_slabs_rows(zs.data_ptr(), 128, 2, B * 128, bias.data_ptr(), B, M, 1, 0.5, 0, 0,
                                           seed.data_ptr(), 3, row0, out.data_ptr(), 5, nx.data_ptr(), 5,
                                           done.data_ptr(), None, 0, None, None,
                                           base.data_ptr() if base is not None else None,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        return out, nx, done
    ref = slabs(R, None)
    for got in (slabs(0, word(R)), slabs(30, word(R - 30))):
        assert all(torch.equal(a, b) for a, b in zip(ref, got))
    assert not torch.equal(ref[0], slabs(0, None)[0])


def test_blocks_path_on_the_gpu_replays_one_set_of_graphs():
    """A slot count the recycling path refuses: blocks through GraphDecoder,
    every block with its own row0, without a capture per block."""
    z, t = _jobs(37)
    dec = ST.StreamDecoder(_model(), 8, N, TEMP)
    dec.impl = "blocks"                       # (the same jobs through the other implementation)
    s, l = dec.run(z, temperature=t, seed=SEED)
    graphs = dec._blocks[8].graphs
    s2, l2 = dec.run(z, temperature=t, seed=SEED, first_row=0)
    assert dec._blocks[8].graphs is graphs and _same((s, l), (s2, l2))
    for j0 in (0, 8, 32):
        n = min(8, 37 - j0)
        ref = SM.GraphDecoder(_model(), n, N, TEMP, use_graph=False).run(seed=SEED, z=z[j0:j0 + n],
                                                                       temperature=t[j0:j0 + n], row0=j0)
        assert torch.equal(s[j0:j0 + n], ref[0]) and torch.equal(l[j0:j0 + n], ref[1])


def test_vae_sample_cli_bulk_recycles(tmp_path, capsys):
    """``vae_sample --mode bulk`` on the GPU takes the recycling path (bf16 is
    its default there) and writes the API's sketches."""
    import json
    import os
    import numpy as np
    from sketch_rnn_amd.cli import vae_sample
    from sketch_rnn_amd.config import save_json
    from sketch_rnn_amd.data.quickdraw import load_pack
    from sketch_rnn_amd.data.strokes import to_normal_strokes
    ops.set_compute_dtype("fp32")             # the state a fresh process starts in
    cfg = _model().cfg
    d = str(tmp_path / "save")
    os.makedirs(d)
    save_json(cfg, os.path.join(d, "config.json"))
    pack = str(tmp_path / "bulk.npz")
    args = ["--save_dir", d, "--device", DEV, "--mode", "bulk", "--n", "37", "--slots", "8", "--seed", "4",
            "--temperature", "0.5", "--out_pack", pack]
    assert vae_sample.main(args) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["impl"] == "recycle" and line["dtype"] == "bf16" and line["n"] == 37
    assert ops.get_compute_dtype() == "fp32"                       # restored
    sk, _ = load_pack(pack)["train"]
    assert len(sk) == 37
    ops.set_compute_dtype("bf16")
    m = SketchVAE(cfg).to(DEV).eval()                              # the CLI's model: the config's seed, no checkpoint
    z = torch.as_tensor(np.random.RandomState(4).randn(37, cfg.z_size), dtype=torch.float32, device=DEV)
    dec = ST.StreamDecoder(m, 8, N, 0.5)
    s, l = dec.run(z, seed=4)
    assert dec.impl == "recycle"
    for a, x, n in zip(sk, s.cpu().numpy(), l.cpu().numpy()):
        assert np.array_equal(a, to_normal_strokes(x[:n]))
    for k in ("steps_run", "slot_steps", "valid_strokes", "occupancy"):
        assert line[k] == getattr(dec, k), k
    assert vae_sample.main(args + ["--dtype", "fp32"]) == 0        # asked for: the blocks path
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["impl"] == "blocks"


def test_recycle_refusals():
    m = _model()
    with pytest.raises(ValueError):
        ST.StreamDecoder(m, 8, N, fp8=True)
    dec = ST.StreamDecoder(m, 8, N, TEMP)
    pre = torch.zeros(4, 2, 5, device=DEV)
    pre[..., 2] = 1.0
    with pytest.raises(ValueError):
        dec.run(_jobs(4)[0], prefix=pre)
    assert ST.StreamDecoder(m, 130, N, TEMP).impl == "blocks"     # a slot count the stepper refuses
