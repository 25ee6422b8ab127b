"""Per-row sampling temperature on the CPU: the sampler's PyTorch
transcription, ``GraphDecoder.run(temperature=)``, the validation shared with
the whole-sketch decoders, and ``vae_sample --temperatures``."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from sketch_rnn_amd.config import RefConfig, VAEConfig
from sketch_rnn_amd.models.reference import SketchRNN
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import sampler as SM

N = 48
# powers of two: the scalar form takes its reciprocal in double and the per-row form in fp32; both are exact here
TEMPS = (0.25, 0.5, 1.0, 2.0)


@pytest.mark.parametrize("forced_rows", [False, True])
@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("mode", [0, 1])
def test_mdn_sample_torch_per_row(mode, step, greedy, forced_rows):
    Bn, M = 64, 5
    g = torch.Generator().manual_seed(100 * mode + 10 * step + greedy)
    z = torch.randn(Bn, 3 + 6 * M, generator=g) * 2
    done0 = (torch.rand(Bn, generator=g) < 0.3).to(torch.int32)
    pick = torch.randint(0, len(TEMPS), (Bn,), generator=g)
    temps = torch.tensor(TEMPS)[pick]
    kw = {}
    if forced_rows:
        forced = torch.randn(Bn, 5, generator=g)
        forced[:, 2:] = 0.0
        forced[torch.arange(Bn), 2 + torch.randint(0, 3, (Bn,), generator=g)] = 1.0
        kw = dict(forced=forced, nforced=torch.tensor([0, step, step + 1, 10 ** 6], dtype=torch.int32).repeat(Bn // 4))
    seed = torch.tensor([7], dtype=torch.int64)

    def call(temp, fn=SM.mdn_sample_torch):
        out, nx, pr, done = torch.zeros(Bn, 5), torch.zeros(Bn, 5), torch.zeros(Bn, 4), done0.clone()
        fn(z, M, mode, temp, greedy, True, seed, step, out, nx, done, pr, **kw)
        return out, nx, done, pr

    res = call(temps)
    scalar = {T: call(T) for T in TEMPS}
    for i, T in enumerate(TEMPS):
        rows = pick == i
        assert bool(rows.any())
        for a, b in zip(res, scalar[T]):
            assert torch.equal(a[rows], b[rows]), (T, mode, step)
    if (mode == 1 or step > 1) and not greedy and not forced_rows:     # where the temperature acts, it matters
        assert not torch.equal(res[3][pick == 0], scalar[TEMPS[3]][3][pick == 0])
    for a, b in zip(res, call(temps, SM.mdn_sample_device)):      # off the GPU the same function
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        call(temps[:-1], SM.mdn_sample_device)
    with pytest.raises(ValueError):
        call(temps.double(), SM.mdn_sample_device)


# the small models of tests/test_complete_gpu.py::_path_model (the two hyper ones differ in the hyper cell's size)
MODELS = {
    "fused4": dict(dec_model="hyper", dec_rnn_size=512, hyper_num_units=256, hyper_embedding_size=16),
    "seven": dict(dec_model="hyper", dec_rnn_size=512, hyper_num_units=128, hyper_embedding_size=16),
    "lstm": dict(dec_model="lstm", dec_rnn_size=256),
    "layer_norm": dict(dec_model="layer_norm", dec_rnn_size=256),
}


def _model(name, seed=3):
    """Pen bias -1.0: p3 ~ 6 % per stroke at temperature 0.5."""
    kw = MODELS[name]
    cfg = VAEConfig(enc_rnn_size=64, z_size=32, num_classes=0, max_seq_len=N, **kw)
    m = SketchVAE(cfg, seed=seed).eval()
    with torch.no_grad():
        m.output_b[2] += -1.0
    return cfg, m


def _not_vacuous(lengths, n=N):
    assert (lengths >= 8).float().mean().item() >= 0.25, lengths
    assert (lengths < n).float().mean().item() >= 0.25, lengths


GROUP_T = (0.25, 0.5, 1.0)


@pytest.mark.parametrize("name", list(MODELS))
def test_graph_decoder_temperature_cpu(name):
    B = 24
    cfg, m = _model(name)
    z = torch.randn(B, cfg.z_size, generator=torch.Generator().manual_seed(1))
    temps = torch.tensor(GROUP_T)[torch.arange(B) % 3]
    dec = SM.GraphDecoder(m, batch=B, steps=N, temperature=0.5)
    s0, l0 = dec.run(seed=3, z=z)
    _not_vacuous(l0)
    sv, lv = dec.run(seed=3, z=z, temperature=temps)
    _not_vacuous(lv)
    scalar = {T: dec.run(seed=3, z=z, temperature=T) for T in GROUP_T}
    for i, T in enumerate(GROUP_T):
        rows = torch.arange(B) % 3 == i
        assert torch.equal(sv[rows], scalar[T][0][rows]) and torch.equal(lv[rows], scalar[T][1][rows]), T
        for U in GROUP_T:          # no row of a group equals its decode at another temperature
            if U != T:
                assert not bool((sv[rows] == scalar[U][0][rows]).flatten(1).all(1).any()), (T, U)
    assert torch.equal(scalar[0.5][0], s0) and torch.equal(scalar[0.5][1], l0)
    sp, lp = dec.run(seed=3, z=z)                        # a temperature does not stick
    assert torch.equal(sp, s0) and torch.equal(lp, l0)
    sl, ll = dec.run(seed=3, z=z, temperature=temps.tolist())     # a list is a vector too
    assert torch.equal(sl, sv) and torch.equal(ll, lv)
    fresh = SM.GraphDecoder(m, batch=B, steps=N, temperature=0.25).run(seed=3, z=z)
    assert torch.equal(fresh[0], scalar[0.25][0]) and torch.equal(fresh[1], scalar[0.25][1])


def test_reference_decoder_temperature_cpu():
    """Mode 0 through ``GraphDecoder``: the temperature acts from step 2 on."""
    B, n = 12, 16
    m = SketchRNN(RefConfig(rnn_size=32, num_mixture=4), seed=0)
    dec = SM.GraphDecoder(m, batch=B, steps=n, temperature=1.0, fix_pen_temperature=True)
    temps = torch.tensor([0.25, 2.0])[torch.arange(B) % 2]
    sv, lv = dec.run(seed=1, temperature=temps)
    for i, T in enumerate((0.25, 2.0)):
        s, l = dec.run(seed=1, temperature=T)
        rows = torch.arange(B) % 2 == i
        assert torch.equal(sv[rows], s[rows]) and torch.equal(lv[rows], l[rows])
    s1, _ = dec.run(seed=1)
    assert torch.equal(sv[:, :2], s1[:, :2]) and not torch.equal(sv, s1)


BAD = [
    lambda B: torch.ones(B - 1), lambda B: torch.ones(B + 1), lambda B: torch.ones(B, 1), lambda B: [0.5] * (B - 1),
    lambda B: 0.0, lambda B: -0.5, lambda B: float("nan"), lambda B: float("inf"),
    lambda B: torch.tensor([0.5] * (B - 1) + [0.0]), lambda B: torch.tensor([-1.0] + [0.5] * (B - 1)),
    lambda B: torch.tensor([0.5] * (B - 1) + [float("nan")]), lambda B: torch.tensor([float("inf")] + [0.5] * (B - 1)),
]


def test_check_temperature():
    B = 6
    for bad in BAD:
        with pytest.raises(ValueError, match="name"):
            SM.check_temperature("name", bad(B), B, "cpu")
    t = SM.check_temperature("name", 0.7, B, "cpu")
    assert t.shape == (B,) and t.dtype == torch.float32 and t.is_contiguous() and bool((t == np.float32(0.7)).all())
    t = SM.check_temperature("name", np.linspace(0.1, 1.0, B), B, "cpu")
    assert t.shape == (B,) and t.dtype == torch.float32
    t = SM.check_temperature("name", torch.linspace(0.1, 1.0, 2 * B, dtype=torch.float64)[::2], B, "cpu")
    assert t.shape == (B,) and t.dtype == torch.float32 and t.is_contiguous()


def test_temperature_validation_through_graph_decoder_run():
    B = 6
    cfg, m = _model("lstm")
    dec = SM.GraphDecoder(m, batch=B, steps=4, temperature=0.5)
    s0, l0 = dec.run(seed=0)
    for bad in BAD:
        with pytest.raises(ValueError, match="GraphDecoder.run"):
            dec.run(seed=0, temperature=bad(B))
    s1, l1 = dec.run(seed=0)          # a rejected temperature leaves nothing behind
    assert torch.equal(s1, s0) and torch.equal(l1, l0)
    ref = SM.GraphDecoder(SketchRNN(RefConfig(rnn_size=32, num_mixture=4), seed=0), batch=B, steps=4)
    for bad in BAD:
        with pytest.raises(ValueError):
            ref.run(seed=0, temperature=bad(B))


def test_sample_args_takes_temps_keyword():
    import inspect
    from sketch_rnn_amd.sample.hyper_step import HyperStepDecoder
    ps = list(inspect.signature(HyperStepDecoder.sample_args).parameters)
    assert ps[-3:] == ["forced", "nforced", "temps"] and ps.index("temp") == 8


def _saved(tmp_path):
    from sketch_rnn_amd.cli.vae_train import make_datasets
    from sketch_rnn_amd.train.trainer import VAETrainer
    cfg = VAEConfig(enc_rnn_size=16, dec_rnn_size=24, z_size=8, num_mixture=3, dec_model="layer_norm",
                    enc_model="layer_norm", max_seq_len=20, batch_size=4, conditional=True, num_classes=3)
    cfg = dataclasses.replace(cfg, is_training=True)
    (train, valid, test), _ = make_datasets(cfg, None, 60)
    d = str(tmp_path / "save_c")
    tr = VAETrainer(cfg, train, valid, test, device="cpu", save_dir=d, use_graph=False, log=lambda s: None)
    tr.train(num_steps=2, prefetch=False)
    if tr.step == 2:
        tr.save()
    return d


CLI_T = [0.1, 0.4, 0.7, 1.0]


@pytest.mark.parametrize("device_sampler", [False, True])
@pytest.mark.parametrize("mode", ["random", "reconstruct"])
def test_vae_sample_cli_temperatures(tmp_path, monkeypatch, capsys, mode, device_sampler):
    """The grid of ``--temperatures``: one line per latent, column j decoded at
    temperature j (after the original in ``reconstruct``), each the decoder's
    own row for that latent and temperature."""
    from sketch_rnn_amd.cli import vae_eval, vae_sample
    from sketch_rnn_amd.config import load_json
    from sketch_rnn_amd.data.strokes import to_normal_strokes
    from sketch_rnn_amd.render import svg
    d = _saved(tmp_path)
    cfg = load_json(os.path.join(d, "config.json"))
    n, K = 3, len(CLI_T)
    got, calls = {}, []
    monkeypatch.setattr(svg, "grid_strokes3", lambda sk, path, **kw: got.update(sk=[np.asarray(x) for x in sk], kw=kw))
    if device_sampler:       # record what the batched decoder returns, and with which rows
        real_run = SM.GraphDecoder.run

        def run(self, **kw):
            s, l = real_run(self, **kw)
            calls.append((kw, s.clone()))
            return s, l
        monkeypatch.setattr(SM.GraphDecoder, "run", run)
    else:                    # record the host sampler's sketches in call order
        real = SM.sample_vae

        def sample_vae(model, seq_len, temperature, greedy, **kw):
            s5, p = real(model, seq_len, temperature, greedy, **kw)
            calls.append((temperature, kw["z"].clone(), s5.copy()))
            return s5, p
        monkeypatch.setattr(SM, "sample_vae", sample_vae)
    args = ["--save_dir", d, "--device", "cpu", "--n", str(n), "--mode", mode, "--seed", "4",
            "--temperatures", ",".join(str(t) for t in CLI_T)]
    args += ["--synthetic", "60", "--offset", "2"] if mode == "reconstruct" else []
    args += ["--device_sampler"] if device_sampler else []
    assert vae_sample.main(args) == 0
    lead = 1 if mode == "reconstruct" else 0
    assert "(%d sketches)" % (n * (lead + K)) in capsys.readouterr().out
    assert len(got["sk"]) == n * (lead + K) and got["kw"] == dict(maxcol=lead + K)
    cells = [got["sk"][i * (lead + K) + lead + j] for i in range(n) for j in range(K)]
    if mode == "reconstruct":
        ds, _ = vae_eval.load_split(cfg, None, 60, "test", d)
        for i in range(n):
            assert np.array_equal(got["sk"][i * (1 + K)], ds.strokes[2 + i])
    if device_sampler:
        (kw, s), = calls
        assert torch.equal(kw["temperature"], torch.tensor(CLI_T, dtype=torch.float64).repeat(n))
        z = kw["z"].reshape(n, K, -1)
        assert bool((z == z[:, :1]).all()) and not torch.equal(z[0], z[1])     # a line shares its latent
        for c, row in zip(cells, s.numpy()):
            assert np.array_equal(c, to_normal_strokes(row))
    else:
        assert [c[0] for c in calls] == CLI_T * n
        for i in range(n):
            for j in range(K):
                assert torch.equal(calls[i * K + j][1], calls[i * K][1])
        assert not torch.equal(calls[0][1], calls[K][1])
        for c, (_, _, s5) in zip(cells, calls):
            assert np.array_equal(c, to_normal_strokes(s5))


def test_vae_sample_cli_temperatures_rejected(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample
    base = ["--save_dir", str(tmp_path), "--device", "cpu", "--n", "2"]
    for extra in (["--mode", "interpolate", "--temperatures", "0.5,1.0"],
                  ["--mode", "complete", "--temperatures", "0.5,1.0"],
                  ["--mode", "random", "--temperatures", "0.5,0"],
                  ["--mode", "random", "--temperatures", "0.5,x"]):
        with pytest.raises(SystemExit) as e:
            vae_sample.main(base + extra)
        assert e.value.code == 2
        assert "--temperatures" in capsys.readouterr().err
