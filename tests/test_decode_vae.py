"""Fused whole-sketch VAE decoder (sketch_rnn_amd/sample/fused.py,
csrc/decode_vae.hip), the parts that need no GPU: which models are eligible,
how many rows one launch takes, and the ``--fused`` flag of ``vae_sample``
without a device."""
import os

import pytest

from sketch_rnn_amd.config import RefConfig, VAEConfig, save_json
from sketch_rnn_amd.models.reference import SketchRNN
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample.fused import _chunk_rows, fused_vae_ok


def _vae(**kw):
    kw.setdefault("enc_rnn_size", 8)
    kw.setdefault("z_size", 4)
    return SketchVAE(VAEConfig(**kw), seed=0)


@pytest.mark.parametrize("kw", [
    dict(dec_rnn_size=512, num_mixture=20),                                        # conditional (vae_small)
    dict(dec_rnn_size=256, num_mixture=20, conditional=False),                     # unconditional (plumbing)
    dict(dec_rnn_size=512, num_mixture=20, num_classes=3, class_embed="add"),
    dict(dec_rnn_size=512, num_mixture=20, num_classes=3, class_embed="concat"),
    dict(dec_rnn_size=256, num_mixture=32),
    dict(dec_rnn_size=256, num_mixture=1, conditional=False, num_classes=2),
])
def test_fused_vae_ok_accepts(kw):
    assert fused_vae_ok(_vae(dec_model="lstm", **kw))


@pytest.mark.parametrize("kw", [
    dict(dec_model="layer_norm", dec_rnn_size=512, num_mixture=20),
    dict(dec_model="hyper", dec_rnn_size=512, num_mixture=20, hyper_num_units=16, hyper_embedding_size=4),
    dict(dec_model="lstm", dec_rnn_size=1024, num_mixture=20),
    dict(dec_model="lstm", dec_rnn_size=512, num_mixture=24),
    dict(dec_model="lstm", dec_rnn_size=256, num_mixture=33),
    dict(dec_model="lstm", dec_rnn_size=128, num_mixture=20),
])
def test_fused_vae_ok_rejects(kw):
    assert not fused_vae_ok(_vae(**kw))


def test_fused_vae_ok_rejects_reference_model():
    assert not fused_vae_ok(SketchRNN(RefConfig(rnn_size=256, num_layers=1, num_mixture=20), seed=0))


def test_chunk_rows_generalised():
    assert _chunk_rows(1, 2, 256, 512) == 224      # 7 row blocks of 33 workgroups
    assert _chunk_rows(1, 2, 256, 256) == 480      # 15 row blocks of 17 workgroups
    assert _chunk_rows(1, 1, 256, 512) == 112
    assert _chunk_rows(1, 2, 32, 512) == 0         # a row block cannot fit -> NotCoResident
    assert _chunk_rows(1, 1, 16, 256) == 0
    assert _chunk_rows(2, 2) == (256 // 33) * 32   # the reference decoder's default is unchanged


def test_vae_sample_fused_without_gpu_falls_back(tmp_path, capsys):
    from sketch_rnn_amd.cli import vae_sample as cvs
    save_json(VAEConfig(enc_rnn_size=8, dec_rnn_size=16, z_size=4, num_mixture=2, max_seq_len=12), str(tmp_path / "config.json"))
    out = str(tmp_path / "g.svg")
    assert cvs.main(["--save_dir", str(tmp_path), "--out", out, "--n", "2", "--device", "cpu",
                     "--device_sampler", "--fused"]) == 0
    assert "--fused" in capsys.readouterr().out          # says why it did not use the fused decoder
    assert os.path.getsize(out) > 100
    with pytest.raises(SystemExit):                       # --fused needs --device_sampler
        cvs.main(["--save_dir", str(tmp_path), "--out", out, "--n", "2", "--device", "cpu", "--fused"])
