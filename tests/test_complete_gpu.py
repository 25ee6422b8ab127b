"""Sketch completion on the GPU: forced strokes in the two sampler kernels
(csrc/sampler.hip) and in the sampler folded into the decode-step hyper cell
(csrc/decode_step.hip), and stroke prefixes through every step path of
``GraphDecoder`` (four-launch stroke, wide decoder, seven-launch step, generic
``decode_step``)."""
import ctypes

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import VAEConfig
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.utils import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, TEMP = 48, 0.5


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _forced_rows(B, step, stop_col, g):
    """Forced rows (a third of them stop) and nforced drawn from
    {0, step, step + 1, 10^6}: the rows with step < nforced are forced."""
    forced = torch.randn(B, 5, device=DEV, generator=g)
    forced[:, 2:] = 0.0
    forced[torch.arange(B, device=DEV), 2 + torch.randint(0, 3, (B,), device=DEV, generator=g)] = 1.0
    pick = torch.randint(0, 4, (B,), device=DEV, generator=g)
    nforced = torch.tensor([0, step, step + 1, 10 ** 6], dtype=torch.int32, device=DEV)[pick]
    on = step < nforced
    assert bool(on.any()) and bool((~on).any())
    assert bool((forced[on][:, stop_col] > 0).any()) and bool((forced[on][:, stop_col] == 0).any())
    return forced, nforced, on


def _check_forced(res, plain, forced, on, done0, stop_col):
    (o, nx, d), (o0, n0, d0) = res, plain
    assert torch.equal(o[~on], o0[~on]) and torch.equal(nx[~on], n0[~on]) and torch.equal(d[~on], d0[~on])
    assert torch.equal(o[on], forced[on]) and torch.equal(nx[on], forced[on])
    assert torch.equal(d[on], ((done0[on] != 0) | (forced[on][:, stop_col] > 0)).to(torch.int32))


@pytest.mark.parametrize("mode,step", [(0, 5), (1, 0), (1, 7)])
def test_sampler_kernel_forced(mode, step):
    lib = native.require_hip().lib
    B, M = 512, 20
    stop_col = 4 if mode == 1 else 3
    g = torch.Generator(device=DEV).manual_seed(10 * mode + step)
    z = torch.randn(B, 3 + 6 * M, device=DEV, generator=g) * 2
    done0 = (torch.rand(B, device=DEV, generator=g) < 0.3).to(torch.int32)
    forced, nforced, on = _forced_rows(B, step, stop_col, g)
    assert bool((on & (done0 != 0)).any())
    seed = torch.tensor([77], dtype=torch.int64, device=DEV)

    def run(zz, f, nf):
        out, nx, pr, done = (torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV),
                             torch.zeros(B, 4, device=DEV), done0.clone())
        SM.mdn_sample_device(zz, M, mode, TEMP, False, False, seed, step, out, nx, done, pr, f, nf)
        return (out, nx, done), pr

    plain, p0 = run(z, None, None)
    res, p1 = run(z, forced, nforced)
    # forced rows in a strided view (the decoder passes prefix[:, t] of a [B, N, 5] buffer)
    wide = torch.zeros(B, 3, 5, device=DEV)
    wide[:, 1] = forced
    res_w, _ = run(z, wide[:, 1], nforced)
    zn = z.clone()
    zn[on] = float("nan")
    res_n, _ = run(zn, forced, nforced)
    # the exported entry point with no forced rows is the old kernel
    out, nx, done = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV), done0.clone()
    rc = lib.skr_mdn_sample_forced(z.data_ptr(), z.stride(0), B, M, mode, TEMP, 0, 0, seed.data_ptr(), step,
                                   out.data_ptr(), 5, nx.data_ptr(), 5, done.data_ptr(), None, None, 0, None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _check_forced(res, plain, forced, on, done0, stop_col)
    assert torch.equal(p1, p0)                        # params keep describing the draw
    for a, b in zip(res, res_w):
        assert torch.equal(a, b)
    for a, b in zip(res, res_n):                      # NaN in a forced row's head output does not leak
        assert torch.equal(a, b)
    for a, b in zip(plain, (out, nx, done)):
        assert torch.equal(a, b)
    # CPU transcription: the same select on the same draws (ties at float rounding may flip a few rows)
    oc, nc, dc = torch.zeros(B, 5), torch.zeros(B, 5), done0.cpu()
    SM.mdn_sample_torch(z.cpu(), M, mode, TEMP, False, False, seed.cpu(), step, oc, nc, dc, None, forced.cpu(),
                        nforced.cpu())
    assert torch.equal(oc[on.cpu()], res[0][on].cpu()) and torch.equal(dc[on.cpu()], res[2][on].cpu())
    assert (dc == res[2].cpu()).float().mean().item() > 0.998


@pytest.mark.parametrize("mode,step,nslab", [(0, 5, 1), (1, 0, 3), (1, 7, 3), (1, 7, 1)])
def test_sampler_slabs_kernel_forced(mode, step, nslab):
    lib = native.require_hip().lib
    B, M, row0 = 512, 20, 37
    stop_col = 4 if mode == 1 else 3
    g = torch.Generator(device=DEV).manual_seed(100 + 10 * mode + step + nslab)
    zs = torch.randn(nslab, B, 128, device=DEV, generator=g)
    bias = torch.randn(128, device=DEV, generator=g) * 0.3
    done0 = (torch.rand(B, device=DEV, generator=g) < 0.3).to(torch.int32)
    forced, nforced, on = _forced_rows(B, step, stop_col, g)
    seed = torch.tensor([78], dtype=torch.int64, device=DEV)

    def run(zz, f, nf):
        out, nx, done = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV), done0.clone()
        head = (zz.data_ptr(), 128, nslab, B * 128, bias.data_ptr(), B, M, mode, TEMP, 0, 0, seed.data_ptr(), step,
                row0, out.data_ptr(), 5, nx.data_ptr(), 5, done.data_ptr())
        if f is None:
            rc = lib.skr_mdn_sample_slabs(*head, _stream())
        else:
            rc = lib.skr_mdn_sample_slabs_forced(*head, f.data_ptr(), f.stride(0), nf.data_ptr(), _stream())
        assert rc == 0
        return out, nx, done

    plain = run(zs, None, None)
    res = run(zs, forced, nforced)
    zn = zs.clone()
    zn[:, on] = float("nan")
    res_n = run(zn, forced, nforced)
    none = run(zs, forced, torch.zeros_like(nforced))
    torch.cuda.synchronize()
    _check_forced(res, plain, forced, on, done0, stop_col)
    for a, b in zip(res, res_n):
        assert torch.equal(a, b)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)


def _hyper256(seed=1, H=512, E=16, Hh=256):
    cfg = VAEConfig(enc_rnn_size=64, dec_rnn_size=H, z_size=32, dec_model="hyper", hyper_num_units=Hh,
                    hyper_embedding_size=E, num_classes=0, max_seq_len=N)
    return cfg, SketchVAE(cfg, seed=seed).to(DEV).eval()


class _bf16_hip:
    def __enter__(self):
        native.require_hip()
        ops.set_backend("hip")
        ops.set_compute_dtype("bf16")

    def __exit__(self, *exc):
        ops.set_backend("auto")
        ops.set_compute_dtype("fp32")


def test_hyper_cell_folded_sampler_forced():
    """The sampler folded into the decode hyper cell with forced rows: the
    stroke, the next input and the eos flags are those of
    skr_mdn_sample_slabs_forced from the same head slabs; with every row
    forced the cell computes what a teacher-forced step computes from the
    same rows."""
    from sketch_rnn_amd.sample.hyper_step import HyperStepDecoder
    lib = native.require_hip().lib
    with _bf16_hip():
        cfg, m = _hyper256(seed=5)
        B, M = 100, cfg.num_mixture
        g = torch.Generator(device=DEV).manual_seed(4)
        zc = m.condition(torch.randn(B, cfg.z_size, device=DEV, generator=g), None, B, DEV)
        x0 = torch.zeros(B, 5, device=DEV)
        x0[:, 2] = 1
        seed = torch.tensor([11], dtype=torch.int64, device=DEV)
        forced, nforced, on = _forced_rows(B, 0, 4, g)
        done0 = torch.zeros(B, dtype=torch.int32, device=DEV)
        done0[::7] = 1

        def cell(nf):
            """Two strokes; the second samples stroke 0 with ``nf`` (None: takes
            ``forced`` as a given input instead)."""
            st = HyperStepDecoder(m, B, torch.device(DEV))
            st.begin(zc, m.initial_state(zc, B, DEV), x0=x0)
            out, done = torch.zeros(B, 4, 5, device=DEV), done0.clone()
            st.step_fused(0, None)
            if nf is None:
                st.X.copy_(forced)
                st.step_fused(1, None)
            else:
                st.step_fused(1, st.sample_args(0, 3, out[:, 0], done, seed, M, 1, 0.6, False, False,
                                                forced=forced, nforced=nf))
            torch.cuda.synchronize()
            return st, out[:, 0], done

        st, out, done = cell(nforced)
        out_ref, nx_ref, done_ref = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV), done0.clone()
        rc = lib.skr_mdn_sample_slabs_forced(
            st.ZS.data_ptr(), 128, st.S_o, B * 128, st._w["bo"].data_ptr(), B, M, 1, 0.6, 0, 0, seed.data_ptr(), 0, 3,
            out_ref.data_ptr(), 5, nx_ref.data_ptr(), 5, done_ref.data_ptr(), forced.data_ptr(), 5,
            nforced.data_ptr(), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out, out_ref) and torch.equal(st.X, nx_ref) and torch.equal(done, done_ref)
        assert torch.equal(out[on], forced[on]) and not torch.equal(out[~on], forced[~on])
        # every row forced == teacher-forced with the same rows
        sa, out_a, _ = cell(torch.full((B,), 1, dtype=torch.int32, device=DEV))
        sb, _, _ = cell(None)
        assert torch.equal(out_a, forced) and torch.equal(sa.X, forced)
        H = sa.H
        assert torch.equal(sa.HH, sb.HH) and torch.equal(sa.HCC, sb.HCC)
        assert torch.equal(sa.A[:, H:], sb.A[:, H:])


def _not_vacuous(lengths, n=N):
    assert (lengths >= 8).float().mean().item() >= 0.25, lengths
    assert (lengths < n).float().mean().item() >= 0.25, lengths


def _random_prefix(B, P, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pre = torch.zeros(B, P, 5, device=DEV)
    pre[..., :2] = torch.randn(B, P, 2, device=DEV, generator=g) * 0.5
    pen = torch.randint(0, 2, (B * P,), device=DEV, generator=g)
    pre.view(-1, 5)[torch.arange(B * P, device=DEV), 2 + pen] = 1.0
    return pre


# name -> (model kwargs, batch, what _steppers() must be)
PATHS = {
    "fused4": (dict(dec_model="hyper", dec_rnn_size=512, hyper_num_units=256, hyper_embedding_size=16), 100),
    "wide": (dict(dec_model="hyper", dec_rnn_size=512, hyper_num_units=256, hyper_embedding_size=16), 256),
    "seven": (dict(dec_model="hyper", dec_rnn_size=512, hyper_num_units=128, hyper_embedding_size=16), 16),
    "lstm": (dict(dec_model="lstm", dec_rnn_size=256), 16),
    "layer_norm": (dict(dec_model="layer_norm", dec_rnn_size=256), 16),
}


def _path_model(path, bias):
    kw, B = PATHS[path]
    cfg = VAEConfig(enc_rnn_size=64, z_size=32, num_classes=0, max_seq_len=N, **kw)
    m = SketchVAE(cfg, seed=3).to(DEV).eval()
    with torch.no_grad():
        m.output_b[2] += bias
    return cfg, m, B


def _check_path(dec, path):
    stp = dec._steppers()
    if path in ("lstm", "layer_norm"):
        assert stp is None
    else:
        assert stp is not None and len(stp) == 1 and stp[0][2].fused == (path != "seven")
        assert stp[0][1] == dec.B


@pytest.mark.parametrize("path", list(PATHS))
def test_graph_decoder_prefix(path):
    with _bf16_hip():
        cfg, m, B = _path_model(path, -1.0)    # p3 ~ 6 % per stroke: sketches long enough to complete
        z = torch.randn(B, cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        P = 9
        pre = _random_prefix(B, P, 2)
        plen = torch.tensor([0, P, 1, 4, P - 1, 6], device=DEV)[torch.arange(B, device=DEV) % 6]
        a = SM.GraphDecoder(m, batch=B, steps=N, temperature=TEMP, use_graph=True)
        e = SM.GraphDecoder(m, batch=B, steps=N, temperature=TEMP, use_graph=False)
        _check_path(a, path)
        s1, l1 = a.run(seed=3, z=z, prefix=pre, prefix_len=plen)
        graphs = a.graphs
        assert graphs is not None
        s0, l0 = a.run(seed=3, z=z)
        s3, l3 = a.run(seed=3, z=z, prefix=pre, prefix_len=plen)
        sz, lz = a.run(seed=3, z=z, prefix=pre, prefix_len=torch.zeros_like(plen))
        assert a.graphs is graphs                         # a prefix never recaptures
        se, le = e.run(seed=3, z=z, prefix=pre, prefix_len=plen)
        se0, le0 = e.run(seed=3, z=z)
        torch.cuda.synchronize()
        _not_vacuous(l0)
        _not_vacuous(l1)
        inside = torch.arange(N, device=DEV)[None, :] < plen[:, None]
        assert torch.equal(s1[:, :P][inside[:, :P]], pre[inside[:, :P]])          # prefix rows bit for bit
        assert bool((l1 > plen).all())
        assert torch.equal(s1, s3) and torch.equal(l1, l3)                        # with / without / with
        assert not torch.equal(s1, s0)
        assert torch.equal(sz, s0) and torch.equal(lz, l0)                        # all-zero lengths == no prefix
        assert torch.equal(le, l1) and torch.allclose(se, s1, atol=1e-4)          # graph replay vs eager
        assert torch.equal(le0, l0) and torch.allclose(se0, s0, atol=1e-4)
        for r in range(B):
            assert torch.all(s1[r, l1[r]:, 4] == 1)
        # self-prefix: a row's own leading strokes as its prefix leave every later bit unchanged
        # (the noise is keyed by (seed, step, row))
        idx = torch.arange(B, device=DEV)
        k = torch.stack([torch.zeros_like(l0), torch.ones_like(l0), l0 // 2, l0 - 1])[idx % 4, idx]
        k = torch.minimum(k, l0 - 1)
        assert bool((k > 1).any()) and bool((k == 0).any())
        for dec in (a, e):
            base = s0 if dec is a else se0
            ss, ls = dec.run(seed=3, z=z, prefix=base[:, :int(k.max())].clone(), prefix_len=k)
            torch.cuda.synchronize()
            assert torch.equal(ss, base) and torch.equal(ls, l0)
        assert a.graphs is graphs


@pytest.mark.parametrize("path", list(PATHS))
def test_graph_decoder_prefix_early_exit(path):
    """Prefix lengths that straddle the chunk borders (chunk = 5), a model whose
    rows end soon after: the chunked decode with the all-done exit equals the
    full-length decode and stops early."""
    with _bf16_hip():
        cfg, m, B = _path_model(path, 2.5)
        z = torch.randn(B, cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        pre = _random_prefix(B, 11, 5)
        plen = torch.tensor([0, 4, 5, 6, 11], device=DEV)[torch.arange(B, device=DEV) % 5]
        full = SM.GraphDecoder(m, batch=B, steps=N, temperature=TEMP, chunk=5, early_exit=False)
        early = SM.GraphDecoder(m, batch=B, steps=N, temperature=TEMP, chunk=5, early_exit=True)
        _check_path(early, path)
        for seed in (1, 2):
            sf, lf = full.run(seed=seed, z=z, prefix=pre, prefix_len=plen)
            early.out.fill_(7.0)
            se, le = early.run(seed=seed, z=z, prefix=pre, prefix_len=plen)
            torch.cuda.synchronize()
            assert full.steps_run == N and 11 < early.steps_run < N, early.steps_run
            assert torch.equal(lf, le) and torch.equal(sf, se), seed
            inside = torch.arange(11, device=DEV)[None, :] < plen[:, None]
            assert torch.equal(se[:, :11][inside], pre[inside]) and bool((le > plen).all())


def test_state_after_prefix_is_teacher_forced_state():
    """Four-launch stepper: after P forced strokes the resident state (A =
    [h | hh] bf16, CC, HCC) is bit for bit that of P + 1 hand-driven
    teacher-forced steps fed S0, prefix[:, 0], ... -- the same kernels on the
    same inputs; the head product that rides in the sampling arm's grouped
    GEMM launch has its own split-K slabs and changes no bit of the others."""
    from sketch_rnn_amd.sample.hyper_step import HyperStepDecoder
    with _bf16_hip():
        cfg, m = _hyper256(seed=2)
        B, P = 100, 6
        z = torch.randn(B, cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        pre = _random_prefix(B, P, 8)
        dec = SM.GraphDecoder(m, batch=B, steps=P + 1, temperature=TEMP, use_graph=False)
        s, _ = dec.run(seed=5, z=z, prefix=pre)
        stp = dec._steppers()
        assert stp is not None and len(stp) == 1 and stp[0][2].fused
        got = stp[0][2]
        with torch.no_grad():
            zc = m.condition(z, None, B, DEV)
            st = HyperStepDecoder(m, B, torch.device(DEV))
            x0 = torch.zeros(B, 5, device=DEV)
            x0[:, 2] = 1
            st.begin(zc, m.initial_state(zc, B, DEV), x0=x0)
            st.step_fused(0, None)
            for t in range(1, P + 1):
                st.X.copy_(pre[:, t - 1])
                st.step_fused(t, None)
        torch.cuda.synchronize()
        assert torch.equal(s[:, :P], pre)
        assert torch.equal(got.A, st.A) and torch.equal(got.CC, st.CC) and torch.equal(got.HCC, st.HCC)
