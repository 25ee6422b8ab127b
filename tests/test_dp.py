"""Data parallelism (P1/P2) on CPU with the gloo backend, world_size 2 and 4.

* gradient averaging through the bucketed flat-arena reducer equals the
  single-process gradient of the concatenated batch;
* the VAE trainer keeps parameters bitwise identical across ranks (rank 0's
  initial weights are broadcast, every rank applies the same averaged
  update) and reports rank-averaged evaluation scalars.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from sketch_rnn_amd.parallel import dp
    assert dp.init_from_env(backend="gloo")
    return dp


def _grad_worker(rank, world, port, out_dir):
    dp = _init(rank, world, port)
    from sketch_rnn_amd.config import RefConfig
    from sketch_rnn_amd.models.reference import SketchRNN
    from sketch_rnn_amd.train.optim import FlatAdam
    torch.manual_seed(0)
    m = SketchRNN(RefConfig(rnn_size=16, num_mixture=3, keep_prob=1.0), seed=rank + 10)  # different init per rank
    opt = FlatAdam(m.parameters(), lr=0.01)
    dp.broadcast_params(opt.flat)                       # rank 0 wins
    x = torch.randn(8, 6, 5, generator=torch.Generator().manual_seed(3))
    y = torch.randn(8, 6, 5, generator=torch.Generator().manual_seed(4))
    x[..., 2:], y[..., 2:] = 0, 0
    x[..., 4], y[..., 4] = 1, 1
    sl = slice(rank * 4, rank * 4 + 4)
    opt.zero_grad()
    cost = m.loss(x[sl], y[sl], None, train=False)[0]
    cost.backward()
    red = dp.GradReducer(opt.grad, bucket_mb=0.01)      # many small buckets
    assert len(red.buckets) > 1
    red.wait(red.all_reduce(async_op=True))
    avg = dp.average_scalars({"cost": float(cost)})
    torch.save({"grad": opt.grad.clone(), "flat": opt.flat.clone(), "cost": avg["cost"]},
               os.path.join(out_dir, "r%d.pt" % rank))
    dp.barrier()
    torch.distributed.destroy_process_group()


def _vae_worker(rank, world, port, out_dir):
    dp = _init(rank, world, port)
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.config import VAEConfig
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = VAEConfig(enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2, max_seq_len=24, batch_size=4,
                    save_every=0, seed=rank)  # different seeds: broadcast must still align the weights
    (tr_set, va, te), _ = make_datasets(cfg, None, 40, rank=rank)
    tr = VAETrainer(cfg, tr_set, va, te, save_dir=os.path.join(out_dir, "v"), log=lambda s: None)
    tr.train(num_steps=3, log_every=1)
    ev = tr.evaluate(te, max_batches=1)
    torch.save({"flat": tr.opt.flat.clone(), "ev": ev}, os.path.join(out_dir, "v%d.pt" % rank))
    dp.barrier()
    torch.distributed.destroy_process_group()


def _spawn(fn, tmp_path, world=2):
    port = _free_port()
    mp.start_processes(fn, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="spawn")


def test_dp_gradient_average_equals_full_batch(tmp_path):
    _spawn(_grad_worker, tmp_path)
    r = [torch.load(tmp_path / ("r%d.pt" % k), weights_only=True) for k in range(2)]
    assert torch.equal(r[0]["flat"], r[1]["flat"]) and torch.equal(r[0]["grad"], r[1]["grad"])
    from sketch_rnn_amd.config import RefConfig
    from sketch_rnn_amd.models.reference import SketchRNN
    from sketch_rnn_amd.train.optim import FlatAdam
    m = SketchRNN(RefConfig(rnn_size=16, num_mixture=3, keep_prob=1.0), seed=10)
    opt = FlatAdam(m.parameters(), lr=0.01)
    assert torch.equal(opt.flat, r[0]["flat"])
    x = torch.randn(8, 6, 5, generator=torch.Generator().manual_seed(3))
    y = torch.randn(8, 6, 5, generator=torch.Generator().manual_seed(4))
    x[..., 2:], y[..., 2:] = 0, 0
    x[..., 4], y[..., 4] = 1, 1
    cost = m.loss(x, y, None, train=False)[0]
    cost.backward()
    assert torch.allclose(opt.grad, r[0]["grad"], atol=1e-6, rtol=1e-5)
    assert abs(float(cost) - r[0]["cost"]) < 1e-5


def test_dp_vae_trainer_ranks_stay_in_sync(tmp_path):
    _spawn(_vae_worker, tmp_path)
    v = [torch.load(tmp_path / ("v%d.pt" % k), weights_only=True) for k in range(2)]
    assert torch.equal(v[0]["flat"], v[1]["flat"])
    assert v[0]["ev"] == v[1]["ev"]


def _vae_overlap_worker(rank, world, port, out_dir):
    """Same training run with the two-phase overlapped step (decoder/head
    all-reduce in flight during the encoder backward) and with the plain
    step: the updates must agree bit for bit."""
    dp = _init(rank, world, port)
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.config import VAEConfig
    from sketch_rnn_amd.train.trainer import VAETrainer
    res = {}
    for mode in ("1", "0"):
        os.environ["SKR_DP_OVERLAP"] = mode
        cfg = VAEConfig(enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2, max_seq_len=24, batch_size=4,
                        save_every=0, seed=rank, num_classes=3)
        (tr_set, va, te), _ = make_datasets(cfg, None, 40, rank=rank)
        tr = VAETrainer(cfg, tr_set, va, te, save_dir=os.path.join(out_dir, "o" + mode), log=lambda s: None)
        assert tr.overlap == (mode == "1")
        if tr.overlap:
            assert len(tr.reducer.parts) == 2
        tr.train(num_steps=3, log_every=1)
        res[mode] = tr.opt.flat.clone()
    os.environ.pop("SKR_DP_OVERLAP")
    torch.save(res, os.path.join(out_dir, "o%d.pt" % rank))
    dp.barrier()
    torch.distributed.destroy_process_group()


def test_dp_overlapped_step_matches_plain_step(tmp_path):
    _spawn(_vae_overlap_worker, tmp_path)
    o = [torch.load(tmp_path / ("o%d.pt" % k), weights_only=True) for k in range(2)]
    assert torch.equal(o[0]["1"], o[0]["0"])
    assert torch.equal(o[0]["1"], o[1]["1"])


def _wire_worker(rank, world, port, out_dir):
    """bf16-on-the-wire gradient averaging vs the fp32 reduction of the same
    per-rank gradients."""
    dp = _init(rank, world, port)
    g = torch.Generator().manual_seed(100 + rank)
    base = torch.randn(10000, generator=g) * (1.0 + rank)
    res = {}
    for wire in ("fp32", "bf16"):
        grad = base.clone()
        red = dp.GradReducer(grad, bucket_mb=0.01, split=3000, wire_dtype=wire)
        assert len(red.parts) == 2 and len(red.buckets) > 2
        w0 = red.start(0)
        red.wait(w0 + red.start(1))
        res[wire] = grad
    torch.save(res, os.path.join(out_dir, "w%d.pt" % rank))
    dp.barrier()
    torch.distributed.destroy_process_group()


def test_dp_bf16_wire_matches_fp32(tmp_path):
    _spawn(_wire_worker, tmp_path)
    w = [torch.load(tmp_path / ("w%d.pt" % k), weights_only=True) for k in range(2)]
    ref = sum(torch.randn(10000, generator=torch.Generator().manual_seed(100 + r)) * (1.0 + r) for r in range(2)) / 2
    assert torch.allclose(w[0]["fp32"], ref, atol=1e-6)
    assert torch.equal(w[0]["bf16"], w[1]["bf16"])                       # every rank holds the same average
    err = (w[0]["bf16"] - ref).abs() / ref.abs().clamp_min(1e-3)
    assert float(err.median()) < 4e-3 and float((w[0]["bf16"] - ref).abs().max()) < 0.05


def test_bench_multi_rank_cpu(tmp_path):
    """bench.py's multi-rank path (torch.distributed.run, gloo on CPU): one
    JSON line from rank 0 with n_gpus = world and the whole-job valid-stroke
    count."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "plumbing", "--batch", "4",
           "--seq-len", "24", "--sketches", "60", "--dtype", "fp32", "--backend", "torch", "--no-eval"]
    env = dict(os.environ, OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 8 and rec["config"]["parallelism"] == "dp2"
    assert 0 < rec["value"] <= rec["positions_per_s"] and 0 < rec["valid_fraction"] <= 1


def test_bench_plain_full_and_dump_cpu(tmp_path):
    """bench.py on the CPU: a plain run times ``--steps`` steps and skips the
    held-out evaluation, ``--full`` runs it, and ``--dump-outputs`` writes the
    last timed step's losses / parameters / gradients as float32 ``.npy``
    files that a second run with the same inputs (here the ``--full`` one)
    reproduces."""
    import json
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--config", "plumbing", "--batch", "4", "--seq-len", "24", "--sketches", "60", "--dtype", "fp32",
            "--backend", "torch"]
    env = dict(os.environ, OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="")

    def run(extra):
        p = subprocess.run(base + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    rec = run(["--dump-outputs", str(tmp_path / "a")])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["test_recon_nll"] is None
    assert rec["unit"] == "strokes/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    full = run(["--full", "--dump-outputs", str(tmp_path / "b")])
    assert full["test_recon_nll"] is not None and np.isfinite(full["test_recon_nll"])
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"cost.npy", "r_cost.npy", "kl_cost.npy", "params.npy", "grads.npy"} <= set(names)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "params.npy").size > 1000 and np.abs(np.load(tmp_path / "a" / "grads.npy")).max() > 0


def _scalars_worker(rank, world, port, out_dir, wire="fp32"):
    """The loss scalars packed into the arena tail come out of the last
    bucket as the sum over ranks: the trainer's logged cost is the mean of
    the per-rank costs, and the valid-point count is the global one -- also
    with the bf16 gradient wire (the tail travels in fp32)."""
    dp = _init(rank, world, port)
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.config import VAEConfig
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = VAEConfig(enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2, max_seq_len=24, batch_size=4,
                    save_every=0, seed=0)
    (tr_set, va, te), _ = make_datasets(cfg, None, 40, rank=rank)
    logs = []
    tr = VAETrainer(cfg, tr_set, va, te, save_dir=os.path.join(out_dir, "s"), log=logs.append, dp_wire_dtype=wire)
    assert tr.reducer.wire_dtype == wire
    assert tr.reducer is not None and tr.reducer.fold_scale and float(tr.opt.scalars[6]) == 0.5
    batch = tr.batch_to_device(tr_set.random_batch(rank, world))
    out = tr.train_step(*batch)
    red = tr.reduced_scalars()
    tr.train(num_steps=2, log_every=1)          # one more step through the logging loop
    glob2 = tr.reduced_scalars()
    torch.save({"local": {k: float(v) for k, v in out.items()}, "red": red, "n": float(batch[1].sum()),
                "log": logs, "glob2": glob2}, os.path.join(out_dir, "s%d.pt" % rank))
    dp.barrier()
    torch.distributed.destroy_process_group()


def _scalars_worker_bf16(rank, world, port, out_dir):
    _scalars_worker(rank, world, port, out_dir, wire="bf16")


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_dp_loss_scalars_reduced_in_last_bucket(tmp_path, wire):
    _spawn(_scalars_worker if wire == "fp32" else _scalars_worker_bf16, tmp_path)
    s = [torch.load(tmp_path / ("s%d.pt" % k), weights_only=True) for k in range(2)]
    for k in ("cost", "r_cost", "kl_cost"):
        mean = (s[0]["local"][k] + s[1]["local"][k]) / 2
        assert abs(s[0]["red"][k] - mean) < 1e-5 * max(1.0, abs(mean)), (k, s[0]["red"][k], mean)
        assert s[0]["red"][k] == s[1]["red"][k]
    assert s[0]["red"]["valid_points"] == s[0]["n"] + s[1]["n"]
    # rank 0 logged the global mean of the step it reported
    line = [ln for ln in s[0]["log"] if ln.startswith("step: 2,")][0]
    assert ("cost: %.4f" % s[0]["glob2"]["cost"]) in line
    assert s[1]["log"] == [] or all(not ln.startswith("step:") for ln in s[1]["log"])


def test_grad_scale_fold_is_bitwise_equal_to_prescaled_arena():
    """1/world folded into the clip + Adam step (FlatAdam.set_grad_scale)
    equals scaling the summed arena first, bit for bit (both clip modes)."""
    from sketch_rnn_amd.train.optim import FlatAdam
    for mode, clip in (("global_norm", 0.5), ("value", 0.01)):
        ps = [torch.nn.Parameter(torch.randn(37, 5, generator=torch.Generator().manual_seed(1))),
              torch.nn.Parameter(torch.randn(300, generator=torch.Generator().manual_seed(2)))]
        a = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.01, clip_mode=mode, clip=clip)
        b = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.01, clip_mode=mode, clip=clip)
        for it in range(3):
            g = torch.randn(a.numel, generator=torch.Generator().manual_seed(10 + it)) * 3.0
            a.grad.copy_(g * (1.0 / 3.0))          # the separate pass
            b.grad.copy_(g)
            b.set_grad_scale(1.0 / 3.0)            # folded
            a.step()
            b.step()
            assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
            assert torch.equal(a.scalars[2], b.scalars[2])


# ---- world size 4: uneven per-rank lengths, >= 3 buckets
# per arena part, overlapped vs plain step, bf16 wire, loss-tail scalars, bench

def _w4_cfg():
    from sketch_rnn_amd.config import VAEConfig
    return VAEConfig(enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2, max_seq_len=60, batch_size=3,
                     save_every=0, seed=0, num_classes=3, random_scale_factor=0.0, augment_stroke_prob=0.0)


def _w4_dataset(cfg):
    """The same synthetic corpus on every rank (and in the reference process):
    random_batch(rank, 4) then hands rank r rows [3r, 3r + 3) of one global
    permutation -- sketches of different lengths on every rank."""
    from sketch_rnn_amd.data.dataset import StrokeDataset
    from sketch_rnn_amd.data.synthetic import synthetic_corpus
    s, lab = synthetic_corpus(60, seed=11, max_len=cfg.max_seq_len, n_classes=3)
    ds = StrokeDataset(s, cfg.batch_size, cfg.max_seq_len, labels=lab, seed=5)
    ds.normalize()
    return ds


# bucket of 0.001 MB = 256 fp32 / 512 bf16 elements: several buckets in both
# parts of the ~3.4K-parameter arena (decoder/head part, encoder part)
_W4_BUCKET_MB = 0.001


def _w4_grad_worker(rank, world, port, out_dir):
    """One training step per mode (overlapped two-phase step / plain step,
    fp32 / bf16 wire) from the same broadcast weights; saved: the reduced
    gradient arena (the SUM over ranks: 1/world is folded into Adam), the
    reduced loss tail and the updated weights."""
    dp = _init(rank, world, port)
    torch.set_num_threads(1)
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = _w4_cfg()
    res = {}
    for mode, wire in (("1", "fp32"), ("0", "fp32"), ("1", "bf16")):
        os.environ["SKR_DP_OVERLAP"] = mode
        ds = _w4_dataset(cfg)
        tr = VAETrainer(cfg, ds, None, None, save_dir=os.path.join(out_dir, "w4" + mode + wire), log=lambda s: None,
                        dp_wire_dtype=wire, dp_bucket_mb=_W4_BUCKET_MB)
        assert tr.overlap == (mode == "1")
        parts = tr.reducer.parts if tr.overlap else [tr.reducer.buckets]
        assert all(len(p) >= 3 for p in parts), [len(p) for p in parts]
        batch = tr.batch_to_device(ds.random_batch(rank, world))
        tr.train_step(*batch)
        key = "ov%s_%s" % (mode, wire)
        res[key] = {"grad": tr.opt.grad.clone(), "flat": tr.opt.flat.clone(), "red": tr.reduced_scalars(),
                    "len": batch[1].clone()}
    os.environ.pop("SKR_DP_OVERLAP")
    torch.save(res, os.path.join(out_dir, "g4_%d.pt" % rank))
    dp.barrier()
    torch.distributed.destroy_process_group()


def test_dp_world4_reduced_gradient_equals_mean_of_rank_gradients(tmp_path):
    """Four gloo ranks, uneven per-rank sketch lengths, >= 3 buckets per part:
    the reduced gradient equals the mean of the four per-rank gradients
    recomputed in one process (same weights, same rank batches, same noise
    seeds), for the overlapped and the plain step; the overlapped step equals
    the plain one bit for bit; every rank ends with the same weights; the
    loss tail carries the mean cost and the global valid-point count; the
    bf16 wire stays within bf16 rounding of the fp32 wire."""
    world = 4
    _spawn(_w4_grad_worker, tmp_path, world=world)
    g = [torch.load(tmp_path / ("g4_%d.pt" % k), weights_only=True) for k in range(world)]
    lens = [int(r["ov1_fp32"]["len"].sum()) for r in g]
    assert len(set(lens)) > 1, lens                                   # uneven per-rank lengths
    for key in ("ov1_fp32", "ov0_fp32", "ov1_bf16"):
        for r in range(1, world):
            assert torch.equal(g[0][key]["flat"], g[r][key]["flat"]), (key, r)
            assert torch.equal(g[0][key]["grad"], g[r][key]["grad"]), (key, r)
    assert torch.equal(g[0]["ov1_fp32"]["grad"], g[0]["ov0_fp32"]["grad"])
    assert torch.equal(g[0]["ov1_fp32"]["flat"], g[0]["ov0_fp32"]["flat"])
    # reference: the same four rank batches in one process
    from sketch_rnn_amd.train import schedules
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = _w4_cfg()
    ds = _w4_dataset(cfg)
    tr = VAETrainer(cfg, ds, None, None, save_dir=str(tmp_path / "ref"), log=lambda s: None)
    full = ds.random_batch(0, 1, batch_size=cfg.batch_size * world)
    tr.kl_w.fill_(schedules.kl_weight(cfg, 0))
    acc = torch.zeros_like(tr.opt.grad)
    costs = []
    for r in range(world):
        sl = slice(r * cfg.batch_size, (r + 1) * cfg.batch_size)
        s, l, c = tr.batch_to_device((full[0][sl], full[1][sl], full[2][sl]))
        assert torch.equal(l, g[r]["ov1_fp32"]["len"])
        tr.seed.fill_(r)                                              # rank r's noise stream
        out = tr._fwd_bwd(s, l, c)
        costs.append(float(out["cost"]))
        acc += tr.opt.grad
    dp_grad = g[0]["ov1_fp32"]["grad"]        # (same init: cfg.seed 0 = rank 0's broadcast weights)
    assert torch.allclose(dp_grad, acc, atol=1e-6, rtol=1e-4), float((dp_grad - acc).abs().max())
    red = g[0]["ov1_fp32"]["red"]
    assert abs(red["cost"] - sum(costs) / world) < 1e-5 * max(1.0, abs(red["cost"]))
    assert red["valid_points"] == sum(lens)
    b16 = g[0]["ov1_bf16"]["grad"]
    assert float(((b16 - dp_grad).abs() / dp_grad.abs().clamp_min(1e-3)).median()) < 4e-3
    assert g[0]["ov1_bf16"]["red"]["valid_points"] == sum(lens)      # the tail travels in fp32


def test_bench_world4_cpu(tmp_path):
    """bench.py under torch.distributed.run with 4 gloo ranks."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"),
           "--gpus", "4", "--steps", "2", "--warmup", "1", "--config", "plumbing", "--batch", "4",
           "--seq-len", "24", "--sketches", "80", "--dtype", "fp32", "--backend", "torch", "--no-eval"]
    env = dict(os.environ, OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 4 and rec["config"]["global_batch"] == 16 and rec["config"]["parallelism"] == "dp4"
    assert rec["config"]["world_size_observed"] == 4
