"""The batch-assembly kernel (csrc/batch.hip) on the GPU against the NumPy
reference of sketch_rnn_amd/ops/batch.py, bit for bit on strokes, lengths and
labels: every operation of the definition is a single correctly rounded fp32
or fp64 operation or an integer one, so there is no margin. Shapes on both
sides of the 64-point pass, the longest drop runs, the largest Nmax, a global
row offset, a position past 2^32; poisoned outputs, repeats, explicit indices,
the device dataset, and a captured training step fed through the aliased
static buffers."""
import numpy as np
import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.data.dataset import StrokeDataset
from sketch_rnn_amd.data.device_dataset import DeviceStrokeDataset
from sketch_rnn_amd.data.synthetic import synthetic_corpus, synthetic_raw_corpus
from sketch_rnn_amd.ops import batch as OB

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_backend("auto")


def _same(a, b):
    a, b = [t.cpu() for t in a], [t.cpu() for t in b]
    return (torch.equal(a[0].contiguous().view(torch.int32), b[0].contiguous().view(torch.int32))
            and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))


def _bitwise(corpus, Nmax, B, **kw):
    """Kernel and reference agree bit for bit; returns the kernel's results."""
    ref = OB.assemble_reference(corpus, Nmax, B, **kw)
    got = OB.assemble_hip(corpus.to(DEV), Nmax, B, **kw)
    assert all(t.is_cuda for t in got)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.int64
    assert got[0].shape == (B, Nmax + 1, 5)
    assert torch.equal(got[1].cpu(), ref[1]), (got[1], ref[1])
    assert torch.equal(got[2].cpu(), ref[2]), (got[2], ref[2])
    assert _same(got, ref)
    return got


def _walk(n, lifts, seed):
    """A sketch of ``n`` points with non-integer offsets, lifted at ``lifts`` and at its end."""
    rng = np.random.RandomState(seed)
    s = np.zeros((n, 3), np.float32)
    s[:, 0:2] = rng.normal(0.0, 3.0, size=(n, 2))
    s[[t for t in lifts if t < n], 2] = 1
    if n:
        s[-1, 2] = 1
    return s


@pytest.fixture(scope="module")
def host_ds():
    strokes, labels = synthetic_corpus(600, seed=4, max_len=250, n_classes=7)
    ds = StrokeDataset(strokes, 100, 250, random_scale_factor=0.15, augment_stroke_prob=0.1, labels=labels)
    ds.normalize()
    return ds


@pytest.fixture(scope="module")
def corpus(host_ds):
    return OB.make_corpus(host_ds.strokes, host_ds.labels, 250)


def test_one_row(corpus):
    _bitwise(corpus, 250, 1, seed=3, step=5, random_scale_factor=0.15, augment_stroke_prob=0.3)


def test_lengths_0_1_5():
    c = OB.make_corpus([np.zeros((0, 3), np.float32), _walk(1, [], 1), _walk(5, [], 2)], labels=[3, 1, 2], Nmax=5)
    for prob in (0.0, 1.0):
        got = _bitwise(c, 5, 3, seed=1, step=0, indices=[0, 1, 2], random_scale_factor=0.3, augment_stroke_prob=prob)
        assert got[1].tolist() == [0, 1, 5 if prob == 0 else 4] and got[2].tolist() == [3, 1, 2]


@pytest.mark.parametrize("Nmax", [64, 65, 129])
def test_strokes_and_drop_runs_across_the_pass_boundaries(Nmax):
    sk = [_walk(Nmax, [], 1),                       # one stroke over every pass
          _walk(Nmax, [62], 2), _walk(Nmax, [63], 3), _walk(Nmax, [64 % Nmax], 4),      # lifts around row 64
          _walk(Nmax, [60, 61, 66], 5), _walk(Nmax - 1, [127 % (Nmax - 1)], 6), _walk(3, [], 7)]
    c = OB.make_corpus(sk, labels=range(len(sk)), Nmax=Nmax)
    for prob in (1.0, 0.5):
        got = _bitwise(c, Nmax, len(sk), seed=9, step=2, indices=list(range(len(sk))), random_scale_factor=0.15,
                       augment_stroke_prob=prob)
    assert got[1][0] < Nmax
    got = _bitwise(c, Nmax, len(sk), seed=9, step=2, indices=list(range(len(sk))), augment_stroke_prob=1.0)
    assert got[1].tolist()[0] == 4                  # points 0, 1, 2 and the lifted end


def test_prob_1_on_the_synthetic_corpus(corpus):
    got = _bitwise(corpus, 250, 32, seed=2, step=1, augment_stroke_prob=1.0)
    assert int(got[1].max()) < 250


def test_flagship_shape(corpus, host_ds):
    got = _bitwise(corpus, 250, 100, seed=7, step=3, random_scale_factor=0.15, augment_stroke_prob=0.1)
    assert len(set(got[2].tolist())) > 1 and int(got[1].max()) > 64


def test_2048_points():
    rows = synthetic_raw_corpus(1, seed=2)[0]
    assert len(rows) == 2048
    c = OB.make_corpus([rows], Nmax=2048)
    for prob in (0.5, 1.0):
        got = _bitwise(c, 2048, 1, seed=5, step=8, random_scale_factor=0.15, augment_stroke_prob=prob)
        assert 0 < int(got[1][0]) < 2048
    assert int(_bitwise(c, 2048, 1, seed=5, step=8)[1][0]) == 2048


def test_row_offset_and_world_rows(corpus):
    kw = dict(seed=4, step=6, random_scale_factor=0.15, augment_stroke_prob=0.1)
    part = _bitwise(corpus, 250, 8, row0=16, world_rows=32, **kw)
    whole = OB.assemble_hip(corpus.to(DEV), 250, 32, **kw)
    assert _same(part, tuple(t[16:24] for t in whole))


def test_position_past_2_pow_32(corpus):
    step = (1 << 31) + 12345
    assert step * 8 + 3 > 1 << 32
    _bitwise(corpus, 250, 4, seed=1, step=step, row0=4, world_rows=8, random_scale_factor=0.15,
             augment_stroke_prob=0.1)


def test_no_augmentation_equals_host_get_batch(host_ds, corpus):
    dd = DeviceStrokeDataset.from_dataset(host_ds, DEV)
    for b in (0, host_ds.num_batches - 1):
        want = tuple(torch.from_numpy(np.ascontiguousarray(w)) for w in host_ds.get_batch(b))
        assert _same(dd.get_batch(b), want)
    idx = list(range(100, 200))
    want = tuple(torch.from_numpy(np.ascontiguousarray(w)) for w in host_ds._from_indices(idx, augment=False))
    assert _same(_bitwise(corpus, 250, 100, seed=0, step=0, indices=idx), want)


def test_out_is_overwritten_and_runs_repeat(corpus):
    cd = corpus.to(DEV)
    kw = dict(seed=11, step=2, random_scale_factor=0.15, augment_stroke_prob=0.2)
    first = OB.assemble(cd, 250, 24, **kw)
    out = (torch.full((24, 251, 5), float("nan"), device=DEV),
           torch.full((24,), -7, dtype=torch.int64, device=DEV), torch.full((24,), -7, dtype=torch.int64, device=DEV))
    got = OB.assemble(cd, 250, 24, out=out, **kw)
    assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2]
    assert not torch.isnan(out[0]).any() and int(out[1].min()) >= 0 and int(out[2].min()) >= 0
    assert _same(out, first) and _same(OB.assemble(cd, 250, 24, **kw), first)
    assert _same(first, OB.assemble_reference(corpus, 250, 24, **kw))


def test_indices_given(corpus):
    idx = [599, 0, 17, 17, 300, 1]
    kw = dict(seed=3, step=4, random_scale_factor=0.15, augment_stroke_prob=0.3)
    got = _bitwise(corpus, 250, 6, indices=idx, **kw)
    assert got[2].tolist() == corpus.labels[idx].tolist()
    assert not torch.equal(got[0][2], got[0][3])          # the same sketch in two rows draws its own augmentation
    on_dev = OB.assemble_hip(corpus.to(DEV), 250, 6, indices=torch.tensor(idx, device=DEV), **kw)
    assert _same(on_dev, got)
    with pytest.raises(ValueError):
        OB.assemble_hip(corpus.to(DEV), 250, 6, indices=torch.tensor([0, 1, 2, 3, 4, 600], device=DEV), **kw)
    with pytest.raises(ValueError):
        OB.assemble_hip(corpus, 250, 6, **kw)              # the kernel path takes a corpus on the GPU


def test_device_dataset_equals_cpu_dataset(host_ds):
    on_gpu = DeviceStrokeDataset.from_dataset(host_ds, DEV, seed=5)
    on_cpu = DeviceStrokeDataset.from_dataset(host_ds, "cpu", seed=5)
    for step, rank, world in ((0, 0, 1), (7, 1, 2), (7, 3, 4)):
        got = on_gpu.random_batch(step, rank, world)
        assert got[0].is_cuda and _same(got, on_cpu.random_batch(step, rank, world))
    assert _same(on_gpu.get_batch(2), on_cpu.get_batch(2))
    assert len(on_gpu) == len(host_ds) and on_gpu.num_batches == host_ds.num_batches and on_gpu.state_dict() == {}
    ops.set_backend("torch")                               # the reference serves a GPU corpus when the backend is off
    assert _same(on_gpu.random_batch(7, 1, 2), on_cpu.random_batch(7, 1, 2))


def test_training_step_from_aliased_static_buffers(tmp_path):
    """Three bf16 steps of a captured vae_small-sized trainer fed by the device
    dataset (from the second step on the batch is assembled straight into the
    graph's static inputs) equal the same steps fed the identical tensors
    through ``batch_to_device``."""
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.config import VAEConfig
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = VAEConfig(enc_rnn_size=256, dec_rnn_size=512, z_size=32, num_mixture=5, max_seq_len=60, batch_size=16,
                    dec_model="lstm", save_every=0, random_scale_factor=0.15, augment_stroke_prob=0.1, seed=3)
    (train, valid, test), _ = make_datasets(cfg, None, 64)
    on_cpu = DeviceStrokeDataset.from_dataset(train, "cpu", seed=cfg.seed)

    def trainer(ds):
        return VAETrainer(cfg, ds, None, None, device=DEV, save_dir=str(tmp_path), use_graph=True,
                          log=lambda s: None, compute_dtype="bf16")

    a = trainer(DeviceStrokeDataset.from_dataset(train, DEV, seed=cfg.seed))
    costs_a, aliased = [], []
    step = a.train_step

    def recording(*batch):
        st = a._graph.static if a._graph is not None else None
        aliased.append(st is not None and all(t.data_ptr() == st[k].data_ptr()
                                              for t, k in zip(batch, ("strokes", "lengths", "labels"))))
        assert _same(batch, on_cpu.random_batch(a.step))
        out = step(*batch)
        costs_a.append(out["cost"].detach().clone())
        return out
    a.train_step = recording
    a.train(num_steps=3, log_every=100)
    assert a._prefetch is None and aliased == [False, True, True]

    b = trainer(train)
    costs_b = []
    for s in range(3):
        out = b.train_step(*b.batch_to_device(on_cpu.random_batch(s)))
        costs_b.append(out["cost"].detach().clone())
    torch.cuda.synchronize()
    assert torch.isfinite(torch.stack(costs_a)).all()
    assert torch.equal(torch.stack(costs_a), torch.stack(costs_b))
    assert torch.equal(a.opt.flat, b.opt.flat)
