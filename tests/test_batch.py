"""Batch assembly from a concatenated corpus (sketch_rnn_amd/ops/batch.py) on
the CPU: the reference against the host dataset and against
``augment_strokes`` fed the same uniforms, bit for bit; hand cases of the drop
rule; the shuffle as a bijection per epoch; world-size invariance and
statelessness, down to a resumed trainer; ranges of the draws; the errors and
the CLI."""
import math
import os

import numpy as np
import pytest
import torch

from sketch_rnn_amd.cli import vae_train
from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.data.dataset import StrokeDataset
from sketch_rnn_amd.data.device_dataset import DeviceStrokeDataset
from sketch_rnn_amd.data.strokes import augment_strokes
from sketch_rnn_amd.data.synthetic import synthetic_corpus
from sketch_rnn_amd.ops import batch as OB
from sketch_rnn_amd.train.trainer import VAETrainer

SIZES = [1, 2, 3, 4, 5, 16, 17, 100, 1000, 4097, 70000]
NMAX = 96


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Two (strokes, lengths, labels) triples hold the same bits."""
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.fixture(scope="module")
def host_ds():
    strokes, labels = synthetic_corpus(400, seed=3, max_len=NMAX, n_classes=5)
    ds = StrokeDataset(strokes, 8, NMAX, random_scale_factor=0.15, augment_stroke_prob=0.1, labels=labels)
    ds.normalize()
    return ds


@pytest.fixture(scope="module")
def dev_ds(host_ds):
    return DeviceStrokeDataset.from_dataset(host_ds, "cpu", seed=11)


def _hand_sketches():
    pen = lambda bits: np.asarray(bits, np.float32)
    mk = lambda n, lifts: np.stack([np.arange(1, n + 1, dtype=np.float32) * 0.37,
                                    -np.arange(1, n + 1, dtype=np.float32) * 1.3, pen(lifts)], 1)
    return [
        np.zeros((0, 3), np.float32),
        mk(1, [1]),
        mk(3, [0, 0, 1]),
        mk(6, [0, 0, 0, 0, 0, 1]),                          # one pen-down stroke
        mk(12, [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1]),       # a lift resets the count
        mk(8, [0, 0, 0, 0, 0, 0, 0, 1]),
    ]


# -- host equality ----------------------------------------------------------------------
def test_reference_equals_host_dataset_without_augmentation(host_ds, dev_ds):
    idx = [0, 5, 399, 17, 17, 250, 3, 128]
    want = host_ds._from_indices(idx, augment=False)
    got = OB.assemble_reference(dev_ds.corpus, NMAX, len(idx), seed=1, step=9, indices=idx)
    assert _same(got, tuple(torch.from_numpy(np.ascontiguousarray(w)) for w in want))
    for b in (0, host_ds.num_batches - 1):
        assert _same(dev_ds.get_batch(b), tuple(torch.from_numpy(np.ascontiguousarray(w)) for w in host_ds.get_batch(b)))


def test_reference_equals_host_dataset_hand_corpus():
    sk = _hand_sketches()
    ds = StrokeDataset(sk, 3, 12, labels=[4, 0, 2, 9, 1, 7])
    dd = DeviceStrokeDataset.from_dataset(ds, "cpu")
    assert len(dd) == len(ds) == 6 and dd.num_batches == ds.num_batches == 2
    for b in range(2):
        assert _same(dd.get_batch(b), tuple(torch.from_numpy(np.ascontiguousarray(w)) for w in ds.get_batch(b)))


# -- the drop rule ------------------------------------------------------------------------
class _StubRNG:
    """Feeds ``augment_strokes`` the reference's uniforms."""

    def __init__(self, u):
        self.u, self.i = [float(v) for v in u], 0

    def rand(self):
        self.i += 1
        return self.u[self.i - 1]


@pytest.mark.parametrize("prob", [0.1, 0.5, 1.0])
def test_drop_rule_equals_augment_strokes(prob):
    strokes, _ = synthetic_corpus(300, seed=5, max_len=NMAX)
    dropped = 0
    for g, rows in enumerate(strokes):
        u = OB.drop_uniforms(7, 3, g, NMAX, len(rows))
        rng = _StubRNG(u)
        want = augment_strokes(rows, prob, rng)
        assert rng.i == len(rows)
        xy, lift = OB.assemble_one(rows, 7, 3, g, NMAX, 0.0, prob)
        assert len(xy) == len(want)
        assert np.array_equal(xy.view(np.int32), want[:, 0:2].view(np.int32))
        assert np.array_equal(lift, want[:, 2] == 1)
        dropped += len(rows) - len(xy)
    assert dropped > 0


def test_drop_hand_cases():
    sk = _hand_sketches()
    corpus = OB.make_corpus(sk, Nmax=12)
    s, l, _ = OB.assemble_reference(corpus, 12, 6, seed=0, step=0, augment_stroke_prob=1.0, indices=range(6))
    assert l.tolist() == [0, 1, 3, 4, 8, 4]
    assert s[0].tolist() == [[0, 0, 1, 0, 0]] + [[0, 0, 0, 0, 1]] * 12                    # n = 0
    assert s[1, 1].tolist() == [sk[1][0, 0], sk[1][0, 1], 0, 1, 0] and s[1, 2, 4] == 1    # n = 1
    assert torch.equal(s[2, 1:4, 0:2], torch.from_numpy(sk[2][:, 0:2]))                   # 3 points never drop
    # six pen-down points: 0, 1, 2 and 5 stay; 2 carries 3 and 4
    x = sk[3].astype(np.float64)
    assert torch.equal(s[3, 1:3, 0:2], torch.from_numpy(sk[3][0:2, 0:2]))
    assert s[3, 3, 0:2].tolist() == [float(np.float32(x[2, 0] + x[3, 0] + x[4, 0])),
                                     float(np.float32(x[2, 1] + x[3, 1] + x[4, 1]))]
    assert torch.equal(s[3, 4, 0:2], torch.from_numpy(sk[3][5, 0:2]))
    assert s[3, 1:5, 2].tolist() == [1, 1, 1, 0] and s[3, 5].tolist() == [0, 0, 0, 0, 1]
    # two strokes of 6: in each, points 3 and 4 merge into 2; the lifted point and the three after a lift stay
    lift = [bool(v) for v in s[4, 1:9, 3].tolist()]
    assert lift == [False, False, False, True, False, False, False, True]
    x = sk[4].astype(np.float64)
    assert s[4, 7, 0].item() == float(np.float32(x[8, 0] + x[9, 0] + x[10, 0]))
    assert s[4, 8, 0].item() == float(sk[4][11, 0])
    # 8 points, the last lifted: 3 .. 6 merge into 2
    x = sk[5].astype(np.float64)
    assert s[5, 3, 1].item() == float(np.float32((((x[2, 1] + x[3, 1]) + x[4, 1]) + x[5, 1]) + x[6, 1]))
    assert s[5, 4].tolist() == [sk[5][7, 0], sk[5][7, 1], 0, 1, 0]


def test_full_length_sketch():
    rows = synthetic_corpus(1, seed=1, max_len=NMAX)[0][0]
    assert len(rows) == NMAX
    corpus = OB.make_corpus([rows], Nmax=NMAX)
    s, l, _ = OB.assemble_reference(corpus, NMAX, 1, seed=0, step=0, indices=[0])
    assert l.tolist() == [NMAX] and s[0, NMAX, 4] == 0 and torch.equal(s[0, 1:, 0:2], torch.from_numpy(rows[:, 0:2]))
    s, l, _ = OB.assemble_reference(corpus, NMAX, 1, seed=0, step=0, indices=[0], augment_stroke_prob=1.0)
    n = int(l[0])
    assert n < NMAX and s[0, n + 1:, 4].eq(1).all() and s[0, 1:n + 1, 4].eq(0).all()
    assert abs(float(s[0, 1:, 0].double().sum()) - float(rows[:, 0].astype(np.float64).sum())) < 1e-3


# -- shuffle ----------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_shuffle_is_a_bijection_per_epoch(S):
    e0 = OB.shuffle_positions(5, 0, np.arange(S), S)
    assert np.array_equal(np.sort(e0), np.arange(S))
    e1 = OB.shuffle_positions(5, 1, np.arange(S), S)
    assert np.array_equal(np.sort(e1), np.arange(S))
    if S >= 16:
        assert not np.array_equal(e0, e1)
    for p in (0, S // 2, S - 1):                      # rows of a step map to (epoch, position) by q
        assert OB.shuffle_index(5, p, 0, 1, S) == e0[p]
        assert OB.shuffle_index(5, 1, p, S, S) == e1[p]


def test_batch_straddles_an_epoch_boundary():
    S, B = 17, 8
    sk = [np.asarray([[i, -i, 1]], np.float32) for i in range(S)]
    corpus = OB.make_corpus(sk, labels=np.arange(S), Nmax=4)
    seen = []
    for step in range(5):           # 40 rows: epochs 0 and 1 whole, 6 rows of epoch 2
        _, _, lab = OB.assemble_reference(corpus, 4, B, seed=2, step=step)
        seen += lab.tolist()
    assert sorted(seen[0:17]) == sorted(seen[17:34]) == list(range(17))
    assert seen[16] == OB.shuffle_positions(2, 0, [16], S)[0] and seen[17] == OB.shuffle_positions(2, 1, [0], S)[0]
    assert len(set(seen[34:40])) == 6


# -- world size and statelessness -------------------------------------------------------
def test_world_size_invariance(dev_ds):
    B = dev_ds.batch_size
    whole = dev_ds.random_batch(6, 0, 1, batch_size=4 * B)
    parts = [dev_ds.random_batch(6, r, 4) for r in range(4)]
    assert _same(tuple(torch.cat([p[i] for p in parts]) for i in range(3)), whole)
    assert int(whole[1].sum()) < int(sum(dev_ds.corpus.offsets[i + 1] - dev_ds.corpus.offsets[i] for i in (
        OB.shuffle_index(11, 6, g, 4 * B, len(dev_ds)) for g in range(4 * B))))     # something was dropped


def test_random_batch_is_a_function_of_the_step(dev_ds):
    first = {s: dev_ds.random_batch(s) for s in (0, 1, 2, 40)}
    for s in (40, 2, 0, 1, 1):
        assert _same(dev_ds.random_batch(s), first[s])
    assert not _same(first[0], first[1])
    assert not _same(dev_ds.random_batch(3, rank=1, world=2), dev_ds.random_batch(3, rank=0, world=2))
    out = (torch.full((8, NMAX + 1, 5), float("nan")), torch.full((8,), -1), torch.full((8,), -1))
    assert dev_ds.random_batch(2, out=out)[0] is out[0] and _same(out, first[2])
    assert dev_ds.state_dict() == {}


def _tiny_cfg(**kw):
    return VAEConfig(enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2, max_seq_len=24, batch_size=4,
                     save_every=0, random_scale_factor=0.15, augment_stroke_prob=0.2, seed=5, **kw)


def _tiny_sets(cfg, n=60):
    (tr, va, te), _ = vae_train.make_datasets(cfg, None, n)
    return [DeviceStrokeDataset.from_dataset(d, "cpu", seed=cfg.seed) for d in (tr, va, te)]


def _run(cfg, save_dir, steps, resume=False, losses=None):
    from sketch_rnn_amd import ops
    ops.set_backend("torch")
    try:
        tr = VAETrainer(cfg, *_tiny_sets(cfg), save_dir=save_dir, log=lambda s: None)
        if resume:
            assert tr.resume()
        step = tr.train_step

        def recording(*batch):
            out = step(*batch)
            losses.append(tuple(float(out[k]) for k in ("cost", "r_cost", "kl_cost")))
            return out
        tr.train_step = recording
        tr.train(num_steps=steps, log_every=1)
        assert tr._prefetch is None
        return tr
    finally:
        ops.set_backend("auto")


def test_resumed_trainer_repeats_the_uninterrupted_run(tmp_path):
    cfg = _tiny_cfg()
    a, b = [], []
    full = _run(cfg, str(tmp_path / "a"), 4, losses=a)
    half = _run(cfg, str(tmp_path / "b"), 2, losses=b)
    from sketch_rnn_amd.ckpt import checkpoint as ckpt
    _, extra, _ = ckpt.load_checkpoint(ckpt.latest_checkpoint(str(tmp_path / "b")), half.model, half.opt)
    assert extra["step"] == 2 and "data" not in extra          # no data RNG in the checkpoint
    rest = _run(cfg, str(tmp_path / "b"), 4, resume=True, losses=b)
    assert len(a) == 4 and a == b                    # cost, recon and kl of every step, bit for bit
    assert torch.equal(full.opt.flat, rest.opt.flat) and not torch.equal(full.opt.flat, half.opt.flat)
    ev = full.evaluate(full.valid_set, max_batches=1)
    assert math.isfinite(ev["cost"])


def _rank_worker(rank, world, port, out_dir):
    from test_dp import _init
    dp = _init(rank, world, port)
    from sketch_rnn_amd import ops
    ops.set_backend("torch")
    cfg = _tiny_cfg()
    logs = []
    for name, plan in (("full", [(4, False)]), ("split", [(2, False), (4, True)])):
        for steps, resume in plan:
            tr = VAETrainer(cfg, *_tiny_sets(cfg), save_dir=os.path.join(out_dir, name), log=logs.append)
            if resume:
                assert tr.resume()
            seen = []
            rb = tr.train_set.random_batch
            tr.train_set.random_batch = lambda *a, _rb=rb, _s=seen, **k: _s.append(_rb(*a, **k)) or _s[-1]
            tr.train(num_steps=steps, log_every=1)
            dp.barrier()
            torch.save({"flat": tr.opt.flat.clone(), "batches": [tuple(t.clone() for t in b) for b in seen]},
                       os.path.join(out_dir, "%s_%d_r%d.pt" % (name, steps, rank)))
    dp.barrier()
    torch.distributed.destroy_process_group()


def test_resume_is_exact_on_rank_1_of_2(tmp_path):
    from test_dp import _spawn
    _spawn(_rank_worker, tmp_path)
    ld = lambda n: torch.load(tmp_path / n, weights_only=True)
    full, first, second = ld("full_4_r1.pt"), ld("split_2_r1.pt"), ld("split_4_r1.pt")
    got = first["batches"] + second["batches"]
    assert len(full["batches"]) == len(got) == 4
    assert all(_same(x, y) for x, y in zip(full["batches"], got))
    assert torch.equal(full["flat"], second["flat"])
    r0 = ld("full_4_r0.pt")
    assert torch.equal(r0["flat"], full["flat"]) and not _same(r0["batches"][0], full["batches"][0])


# -- ranges -------------------------------------------------------------------------------
def test_scale_factors_and_drop_share(dev_ds):
    f = 0.15
    s = np.asarray([OB.scale_factors(3, step, g, f) for step in (0, 7) for g in range(500)], np.float64)
    assert s.min() >= 1 - f and s.max() <= 1 + f and s.std() > 0.05
    assert OB.scale_factors(3, 0, 4, 0.0) == (np.float32(1.0), np.float32(1.0))
    c = dev_ds.corpus
    pts, offs = c.points.numpy(), c.offsets.numpy()
    for p in (0.1, 0.5):
        E = D = 0
        for i in range(c.S):
            el = OB.eligible(pts[offs[i]:offs[i + 1], 2] == 1)
            u = OB.drop_uniforms(9, 2, i, NMAX, len(el)).astype(np.float64)
            E += int(el.sum())
            D += int((el & (u < p)).sum())
        bound = 5 * math.sqrt(p * (1 - p) / E)
        assert bound < 0.02, (E, bound)
        assert abs(D / E - p) <= bound, (D, E, p)


# -- errors and CLI -----------------------------------------------------------------------
def test_errors(dev_ds):
    c = dev_ds.corpus
    ok = dict(seed=0, step=0)
    for nmax in (0, OB.MAX_N + 1):
        with pytest.raises(ValueError):
            OB.assemble(c, nmax, 2, **ok)
    with pytest.raises(ValueError):
        OB.assemble(c, NMAX - 1, 2, **ok)                       # a sketch longer than Nmax
    with pytest.raises(ValueError):
        OB.make_corpus([np.zeros((5, 3), np.float32)], Nmax=4)
    for bad in ([0, len(dev_ds)], [-1, 0], [0], [[0, 1]], torch.tensor([0, 1], dtype=torch.int32), [0.0, 1.0]):
        with pytest.raises(ValueError):
            OB.assemble(c, NMAX, 2, indices=bad, **ok)
    for prob in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            OB.assemble(c, NMAX, 2, augment_stroke_prob=prob, **ok)
    for f in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            OB.assemble(c, NMAX, 2, random_scale_factor=f, **ok)
    with pytest.raises(ValueError):
        OB.assemble(c, NMAX, 2, row0=2, world_rows=3, **ok)
    with pytest.raises(ValueError):
        OB.assemble(c, NMAX, 2, out=(torch.zeros(2, NMAX, 5), torch.zeros(2, dtype=torch.int64),
                                     torch.zeros(2, dtype=torch.int64)), **ok)
    with pytest.raises(ValueError):
        OB.make_corpus([np.asarray([[1, 1, 0.5]], np.float32)])
    assert OB.assemble(c, NMAX, 0, **ok)[0].shape == (0, NMAX + 1, 5)
    used = {0, 1, 7, 8, 11, 12, 13, 14, 17, 18, 23, 24, 29, 30, 31, 32, 0x5A3D}
    ids = {OB.STREAM_SHUFFLE, OB.STREAM_SCALE, OB.STREAM_DROP}
    assert len(ids) == 3 and not ids & used and not {(i - 0x3C6EF372) & 0xFFFFFFFF for i in ids} & used


def test_vae_train_cli_device_data_cpu(tmp_path, capsys):
    rc = vae_train.main(["--device_data", "--synthetic", "300", "--num_steps", "3", "--device", "cpu", "--dtype", "fp32",
                         "--enc_rnn_size", "8", "--dec_rnn_size", "16", "--z_size", "4", "--num_mixture", "2",
                         "--max_seq_len", "32", "--batch_size", "8", "--save_every", "0", "--log_every", "1",
                         "--random_scale_factor", "0.15", "--augment_stroke_prob", "0.1",
                         "--save_dir", str(tmp_path / "save")])
    out = capsys.readouterr().out
    assert rc == 0 and "step: 3," in out and "test: cost" in out
