"""Per-row sampling temperature on the GPU: the two sampler kernels
(csrc/sampler.hip), the sampler folded into the decode-step hyper cell
(csrc/decode_step.hip), ``GraphDecoder.run(temperature=)`` on every step path,
and the three whole-sketch decoders (csrc/decode_vae.hip,
csrc/decode_vae_ln.hip, csrc/decode_ref.hip)."""
import ctypes
import functools

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.config import RefConfig, VAEConfig
from sketch_rnn_amd.models.reference import SketchRNN
from sketch_rnn_amd.models.vae import SketchVAE
from sketch_rnn_amd.sample import fused as F
from sketch_rnn_amd.sample import sampler as SM
from sketch_rnn_amd.utils import native
from test_decode_vae_ln import make_model as make_ln_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 48
KERNEL_T = (0.2, 0.37, 1.0, 1.7)      # by row in the kernel tests
GROUP_T = (0.25, 0.5, 1.0)            # [b % 3] in the decoder tests: does not line up with the 128-row blocks


@pytest.fixture(autouse=True)
def _restore():
    yield
    F.LN_DECODE_POISON = False
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    from sketch_rnn_amd.ops.recurrent import check_cluster_errors
    torch.cuda.synchronize()
    check_cluster_errors(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _forced_rows(B, step, g):
    forced = torch.randn(B, 5, device=DEV, generator=g)
    forced[:, 2:] = 0.0
    forced[torch.arange(B, device=DEV), 2 + torch.randint(0, 3, (B,), device=DEV, generator=g)] = 1.0
    pick = torch.randint(0, 4, (B,), device=DEV, generator=g)
    nforced = torch.tensor([0, step, step + 1, 10 ** 6], dtype=torch.int32, device=DEV)[pick]
    assert bool((step < nforced).any()) and bool((step >= nforced).any())
    return forced, nforced


def _row_temps(B, g):
    pick = torch.randint(0, len(KERNEL_T), (B,), device=DEV, generator=g)
    assert all(bool((pick == i).any()) for i in range(len(KERNEL_T)))
    return torch.tensor(KERNEL_T, device=DEV)[pick], pick


def _groups_equal(res, scalar, pick):
    """Each temperature group's rows of ``res`` equal, bit for bit, the same
    rows of the scalar call at that value."""
    for i, T in enumerate(KERNEL_T):
        rows = pick == i
        for a, b in zip(res, scalar[T]):
            assert torch.equal(a[rows], b[rows]), T


@pytest.mark.parametrize("mode,step,greedy,fix_pen", [(1, 0, False, False), (1, 7, False, False), (0, 5, False, True),
                                                      (0, 1, False, True), (1, 3, True, False)])
def test_sampler_kernel_per_row(mode, step, greedy, fix_pen):
    native.require_hip()
    B, M = 257, 20
    g = torch.Generator(device=DEV).manual_seed(10 * mode + step)
    z = torch.randn(B, 3 + 6 * M, device=DEV, generator=g) * 2
    done0 = (torch.rand(B, device=DEV, generator=g) < 0.3).to(torch.int32)
    forced, nforced = _forced_rows(B, step, g)
    temps, pick = _row_temps(B, g)
    seed = torch.tensor([77], dtype=torch.int64, device=DEV)

    def run(temp, f=None, nf=None, fn=SM.mdn_sample_device):
        out, nx, pr, done = (torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV),
                             torch.zeros(B, 4, device=DEV), done0.clone())
        fn(z, M, mode, temp, greedy, fix_pen, seed, step, out, nx, done, pr, f, nf)
        return out, nx, done, pr

    uni = run(torch.full((B,), 0.37, device=DEV))
    mixed = run(temps)
    mixed_f = run(temps, forced, nforced)
    wide = torch.zeros(B, 3, device=DEV)
    wide[:, 1] = temps
    strided = run(wide[:, 1])
    strided_f = run(wide[:, 1], forced, nforced)
    scalar = {T: run(T) for T in KERNEL_T}
    scalar_f = {T: run(T, forced, nforced) for T in KERNEL_T}
    torch_mixed = run(temps, fn=SM.mdn_sample_torch)
    torch.cuda.synchronize()
    for a, b in zip(uni, scalar[0.37]):
        assert torch.equal(a, b)
    _groups_equal(mixed, scalar, pick)
    _groups_equal(mixed_f, scalar_f, pick)
    for a, b in zip(mixed + mixed_f, strided + strided_f):
        assert torch.equal(a, b)
    if mode == 0 and step <= 1:                     # the reference applies its temperature from step 2 on
        assert torch.equal(mixed[0], scalar[1.0][0])
    elif not greedy:                                # where it acts, it matters
        assert not torch.equal(mixed[0], scalar[1.0][0])
    # against the transcription with the same vector (inverse-CDF ties at float rounding may flip a row)
    (o1, n1, d1, p1), (o2, n2, d2, p2) = mixed, torch_mixed
    same = (p1[:, 0] == p2[:, 0]) & (p1[:, 1] == p2[:, 1])
    print("rows with the same (idx, pidx): %.4f" % same.float().mean().item())
    assert same.float().mean().item() > 0.998
    assert torch.allclose(n1[same], n2[same], rtol=1e-4, atol=1e-4)
    assert torch.allclose(o1[same], o2[same], rtol=1e-4, atol=1e-4)
    assert torch.allclose(p1[same], p2[same], rtol=1e-4, atol=1e-4)
    assert torch.equal(d1[same], d2[same])


@pytest.mark.parametrize("mode,step,nslab", [(1, 0, 1), (1, 7, 3), (0, 5, 3), (0, 5, 1)])
def test_sampler_slabs_kernel_per_row(mode, step, nslab):
    lib = native.require_hip().lib
    B, M, row0 = 257, 20, 37
    g = torch.Generator(device=DEV).manual_seed(100 + 10 * mode + step + nslab)
    zs = torch.randn(nslab, B, 128, device=DEV, generator=g)
    bias = torch.randn(128, device=DEV, generator=g) * 0.3
    done0 = (torch.rand(B, device=DEV, generator=g) < 0.3).to(torch.int32)
    forced, nforced = _forced_rows(B, step, g)
    temps, pick = _row_temps(B, g)
    seed = torch.tensor([78], dtype=torch.int64, device=DEV)

    def run(temp, f=None, nf=None):
        out, nx, done = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV), done0.clone()
        vec = torch.is_tensor(temp)
        head = (zs.data_ptr(), 128, nslab, B * 128, bias.data_ptr(), B, M, mode, 1.0 if vec else temp, 0, 1,
                seed.data_ptr(), step, row0, out.data_ptr(), 5, nx.data_ptr(), 5, done.data_ptr())
        fa = (None, 0, None) if f is None else (f.data_ptr(), f.stride(0), nf.data_ptr())
        if vec:
            rc = lib.skr_mdn_sample_slabs_temps(*head, *fa, temp.data_ptr(), _stream())
        elif f is None:
            rc = lib.skr_mdn_sample_slabs(*head, _stream())
        else:
            rc = lib.skr_mdn_sample_slabs_forced(*head, *fa, _stream())
        assert rc == 0
        return out, nx, done

    uni = run(torch.full((B,), 0.37, device=DEV))
    mixed = run(temps)
    mixed_f = run(temps, forced, nforced)
    # a view into a larger buffer: temps is indexed by the launch's local row, row0 is a hash key only
    big = torch.full((B + 50,), 9.0, device=DEV)
    big[50:] = temps
    offset = run(big[50:])
    scalar = {T: run(T) for T in KERNEL_T}
    scalar_f = {T: run(T, forced, nforced) for T in KERNEL_T}
    none = out, nx, done = torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV), done0.clone()
    rc = lib.skr_mdn_sample_slabs_temps(zs.data_ptr(), 128, nslab, B * 128, bias.data_ptr(), B, M, mode, 0.37, 0, 1,
                                        seed.data_ptr(), step, row0, out.data_ptr(), 5, nx.data_ptr(), 5,
                                        done.data_ptr(), None, 0, None, None, _stream())     # null temps: the scalar
    assert rc == 0
    torch.cuda.synchronize()
    for a, b, c in zip(uni, scalar[0.37], none):
        assert torch.equal(a, b) and torch.equal(a, c)
    _groups_equal(mixed, scalar, pick)
    _groups_equal(mixed_f, scalar_f, pick)
    for a, b in zip(mixed, offset):
        assert torch.equal(a, b)
    assert not torch.equal(mixed[0], scalar[1.0][0])
    # against the transcription with the same vector, on the head output folded in the kernel's order
    # (fold_head_slabs: bias + ((s0 + s1) + (s2 + 0)): the same fp32 sums, so the same bits). The slab kernel
    # returns no (idx, pidx): a row that agrees to the tolerance drew the same pair.
    z = bias + (zs[0] if nslab == 1 else (zs[0] + zs[1]) + zs[2])
    R = row0 + B                                    # rows of the hash: row0 + b
    u = torch.zeros(R, 3 + 6 * M, device=DEV)
    u[row0:] = z[:, :3 + 6 * M]
    tt = torch.ones(R, device=DEV)
    tt[row0:] = temps
    d2 = torch.zeros(R, dtype=torch.int32, device=DEV)
    d2[row0:] = done0
    o2, n2 = torch.zeros(R, 5, device=DEV), torch.zeros(R, 5, device=DEV)
    SM.mdn_sample_torch(u, M, mode, tt, False, True, seed, step, o2, n2, d2)
    o2, n2, d2 = o2[row0:], n2[row0:], d2[row0:]
    same = torch.isclose(mixed[1], n2, rtol=1e-4, atol=1e-4).all(1)
    print("rows agreeing with the transcription: %.4f" % same.float().mean().item())
    assert same.float().mean().item() > 0.998
    assert torch.allclose(mixed[0][same], o2[same], rtol=1e-4, atol=1e-4)
    assert torch.equal(mixed[2][same], d2[same])


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


def test_hyper_cell_folded_sampler_per_row():
    """The sampler folded into the decode hyper cell with per-row temperatures:
    the stroke, the next input and the eos flags are those of
    skr_mdn_sample_slabs_temps from the same head slabs, each temperature
    group's rows are the scalar launch's, and so is the cell state the launch
    leaves for those rows."""
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
        forced, nforced = _forced_rows(B, 0, g)
        temps, pick = _row_temps(B, g)
        done0 = torch.zeros(B, dtype=torch.int32, device=DEV)
        done0[::7] = 1

        def cell(temp, nf=None):
            """Two strokes; the second samples stroke 0 at ``temp`` (a float or a vector)."""
            st = HyperStepDecoder(m, B, torch.device(DEV))
            st.begin(zc, m.initial_state(zc, B, DEV), x0=x0)
            out, done = torch.zeros(B, 4, 5, device=DEV), done0.clone()
            st.step_fused(0, None)
            vec = torch.is_tensor(temp)
            kw = dict(forced=forced, nforced=nf) if nf is not None else {}
            st.step_fused(1, st.sample_args(0, 3, out[:, 0], done, seed, M, 1, 1.0 if vec else temp, False, False,
                                            temps=temp if vec else None, **kw))
            torch.cuda.synchronize()
            return st, (out[:, 0].clone(), st.X.clone(), done)

        def state(st):
            H = st.H
            return st.HH.clone(), st.HCC.clone(), st.A[:, H:].clone()

        st, mixed = cell(temps)
        ref = out_ref, nx_ref, done_ref = (torch.zeros(B, 5, device=DEV), torch.zeros(B, 5, device=DEV),
                                           done0.clone())
        rc = lib.skr_mdn_sample_slabs_temps(
            st.ZS.data_ptr(), 128, st.S_o, B * 128, st._w["bo"].data_ptr(), B, M, 1, 1.0, 0, 0, seed.data_ptr(), 0, 3,
            out_ref.data_ptr(), 5, nx_ref.data_ptr(), 5, done_ref.data_ptr(), None, 0, None, temps.data_ptr(),
            _stream())
        assert rc == 0
        torch.cuda.synchronize()
        for a, b in zip(mixed, ref):
            assert torch.equal(a, b)
        s_mixed = state(st)
        st_u, uni = cell(torch.full((B,), 0.37, device=DEV))
        st_s, sca = cell(0.37)
        for a, b in zip(uni + state(st_u), sca + state(st_s)):
            assert torch.equal(a, b)
        _, mixed_f = cell(temps, nforced)
        for i, T in enumerate(KERNEL_T):
            rows = pick == i
            st_t, res_t = cell(T)
            for a, b in zip(mixed + s_mixed, res_t + state(st_t)):
                assert torch.equal(a[rows], b[rows]), T
            _, res_tf = cell(T, nforced)
            for a, b in zip(mixed_f, res_tf):
                assert torch.equal(a[rows], b[rows]), T
        assert not torch.equal(mixed[0], sca[0])


def _not_vacuous(lengths, n=N):
    assert (lengths >= 8).float().mean().item() >= 0.25, lengths
    assert (lengths < n).float().mean().item() >= 0.25, lengths


# the step paths of tests/test_complete_gpu.py: name -> (model kwargs, batch)
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


def _random_prefix(B, P, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pre = torch.zeros(B, P, 5, device=DEV)
    pre[..., :2] = torch.randn(B, P, 2, device=DEV, generator=g) * 0.5
    pen = torch.randint(0, 2, (B * P,), device=DEV, generator=g)
    pre.view(-1, 5)[torch.arange(B * P, device=DEV), 2 + pen] = 1.0
    return pre


@pytest.mark.parametrize("path", list(PATHS))
def test_graph_decoder_temperature(path):
    with _bf16_hip():
        cfg, m, B = _path_model(path, -1.0)
        z = torch.randn(B, cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        group = torch.arange(B, device=DEV) % 3
        temps = torch.tensor(GROUP_T, device=DEV)[group]
        a = SM.GraphDecoder(m, batch=B, steps=N, temperature=0.5, use_graph=True)
        e = SM.GraphDecoder(m, batch=B, steps=N, temperature=0.5, use_graph=False)
        _check_path(a, path)
        s0, l0 = a.run(seed=3, z=z)
        graphs = a.graphs
        assert graphs is not None
        sv, lv = a.run(seed=3, z=z, temperature=temps)
        scalar = {T: a.run(seed=3, z=z, temperature=T) for T in GROUP_T}
        sp, lp = a.run(seed=3, z=z)                       # back to the constructor's value
        assert a.graphs is graphs                         # a temperature never recaptures
        se, le = e.run(seed=3, z=z, temperature=temps)
        torch.cuda.synchronize()
        _not_vacuous(l0)
        _not_vacuous(lv)
        assert torch.equal(sp, s0) and torch.equal(lp, l0)
        assert torch.equal(scalar[0.5][0], s0) and torch.equal(scalar[0.5][1], l0)
        for i, T in enumerate(GROUP_T):
            rows = group == i
            assert torch.equal(sv[rows], scalar[T][0][rows]) and torch.equal(lv[rows], scalar[T][1][rows]), T
            # a decoder freshly built at T (at 0.5 that is `a`'s own first run)
            fs, fl = (s0, l0) if T == 0.5 else SM.GraphDecoder(m, batch=B, steps=N, temperature=T).run(seed=3, z=z)
            assert torch.equal(sv[rows], fs[rows]) and torch.equal(lv[rows], fl[rows]), T
        assert not torch.equal(sv[group == 0], s0[group == 0])
        assert torch.equal(le, lv) and torch.allclose(se, sv, atol=1e-4)          # graph replay vs eager
        if path == "fused4":      # together with a prefix
            P = 9
            pre = _random_prefix(B, P, 2)
            plen = torch.tensor([0, P, 1, 4, P - 1, 6, 2], device=DEV)[torch.arange(B, device=DEV) % 7]
            s1, l1 = a.run(seed=3, z=z, prefix=pre, prefix_len=plen, temperature=temps)
            inside = torch.arange(P, device=DEV)[None, :] < plen[:, None]
            assert torch.equal(s1[:, :P][inside], pre[inside])
            for i, T in enumerate(GROUP_T):
                rows = group == i
                st, lt = a.run(seed=3, z=z, prefix=pre, prefix_len=plen, temperature=T)
                assert torch.equal(s1[rows], st[rows]) and torch.equal(l1[rows], lt[rows]), T
            assert torch.equal(s1[plen == 0], sv[plen == 0])
        assert a.graphs is graphs


def test_graph_decoder_temperature_early_exit():
    """Chunks of 5 steps with the all-done exit: the mixed vector equals each
    group's scalar run there too."""
    with _bf16_hip():
        cfg, m, B = _path_model("fused4", 2.5)
        z = torch.randn(B, cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        group = torch.arange(B, device=DEV) % 3
        temps = torch.tensor(GROUP_T, device=DEV)[group]
        dec = SM.GraphDecoder(m, batch=B, steps=N, temperature=0.5, chunk=5)
        sv, lv = dec.run(seed=2, z=z, temperature=temps)
        assert dec.steps_run < N, dec.steps_run
        for i, T in enumerate(GROUP_T):
            st, lt = dec.run(seed=2, z=z, temperature=T)
            assert torch.equal(sv[group == i], st[group == i]) and torch.equal(lv[group == i], lt[group == i]), T


def test_graph_decoder_temperature_fp8():
    """The MX-fp8 step decoder (the model of tests/test_mx8_gpu.py) reads the
    same buffer."""
    with _bf16_hip():
        B = 64
        cfg = VAEConfig(enc_rnn_size=64, dec_rnn_size=512, z_size=32, dec_model="hyper", hyper_num_units=256,
                        hyper_embedding_size=32, num_classes=0, max_seq_len=24)
        m = SketchVAE(cfg, seed=2).to(DEV).eval()
        group = torch.arange(B, device=DEV) % 3
        temps = torch.tensor(GROUP_T, device=DEV)[group]
        dec = SM.GraphDecoder(m, batch=B, steps=24, temperature=0.5, fp8=True)
        sv, lv = dec.run(seed=1, temperature=temps)
        assert dec._steppers()[0][2].fp8
        for i, T in enumerate(GROUP_T):
            st, lt = dec.run(seed=1, temperature=T)
            assert torch.equal(sv[group == i], st[group == i]) and torch.equal(lv[group == i], lt[group == i]), T
        assert not torch.equal(sv[group == 0], dec.run(seed=1)[0][group == 0])


def test_graph_decoder_reference_temperature():
    native.require_hip()
    ops.set_backend("hip")
    B = 64
    m = SketchRNN(RefConfig(rnn_size=256, num_mixture=24), seed=0).to(DEV)
    dec = SM.GraphDecoder(m, batch=B, steps=40, temperature=0.3)
    temps = torch.tensor([0.25, 1.0], device=DEV)[torch.arange(B, device=DEV) % 2]
    s0, l0 = dec.run(seed=5)
    graphs = dec.graphs
    sv, lv = dec.run(seed=5, temperature=temps)
    for i, T in enumerate((0.25, 1.0)):
        rows = torch.arange(B, device=DEV) % 2 == i
        st, lt = dec.run(seed=5, temperature=T)
        assert torch.equal(sv[rows], st[rows]) and torch.equal(lv[rows], lt[rows])
    s1, l1 = dec.run(seed=5)
    assert dec.graphs is graphs and torch.equal(s1, s0) and torch.equal(l1, l0) and not torch.equal(sv, s0)


@functools.lru_cache(maxsize=None)
def _fused_model(kind):
    if kind == "layer_norm":
        return make_ln_model(256, 20).to(DEV).eval()
    m = SketchVAE(VAEConfig(dec_model="lstm", enc_rnn_size=64, dec_rnn_size=256, num_mixture=20), seed=3)
    g = torch.Generator().manual_seed(103)
    with torch.no_grad():
        m.init_w *= 30
        m.dec.bias.copy_(torch.randn(m.dec.bias.shape, generator=g) * 0.1)
        m.output_b.copy_(torch.randn(m.output_b.shape, generator=g) * 0.1)
    return m.to(DEV).eval()


BAD = [lambda B: torch.ones(B - 1), lambda B: 0.0, lambda B: -1.0, lambda B: float("nan"), lambda B: float("inf"),
       lambda B: torch.tensor([0.5] * (B - 1) + [0.0])]


@pytest.mark.parametrize("kind,poison", [("lstm", False), ("layer_norm", False), ("layer_norm", True)])
def test_fused_vae_temperature(kind, poison):
    m = _fused_model(kind)
    cls = F.FusedVAEDecoder if kind == "lstm" else F.FusedLNVAEDecoder
    assert F.fused_vae_kind(m) == kind
    Nf = 20
    B = cls(m, 64, Nf).rows + 6          # two launches: the second with r0 != 0 and a partial row block
    F.LN_DECODE_POISON = poison
    dec = cls(m, B, Nf, temperature=0.5, early_exit=False)
    assert len(range(0, B, dec.rows)) == 2
    z = torch.randn(B, m.cfg.z_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    group = torch.arange(B, device=DEV) % 3
    temps = torch.tensor(GROUP_T, device=DEV)[group]
    s0, l0 = dec.run(seed=4, z=z)
    sv, lv = dec.run(seed=4, z=z, temperature=temps)
    s8, l8 = cls(m, B, Nf, temperature=0.5, chunk=8, early_exit=False).run(seed=4, z=z, temperature=temps)
    pre = _random_prefix(B, 7, 5)
    plen = torch.tensor([0, 3, 7, 1], device=DEV)[torch.arange(B, device=DEV) % 4]
    s1, l1 = dec.run(seed=4, z=z, prefix=pre, prefix_len=plen, temperature=temps)
    torch.cuda.synchronize()
    assert not torch.isnan(sv).any() and not torch.isnan(s1).any()
    assert torch.equal(s8, sv) and torch.equal(l8, lv)
    for i, T in enumerate(GROUP_T):
        rows = group == i
        st, lt = dec.run(seed=4, z=z, temperature=T)
        assert torch.equal(sv[rows], st[rows]) and torch.equal(lv[rows], lt[rows]), T
        sp, lp = dec.run(seed=4, z=z, prefix=pre, prefix_len=plen, temperature=T)
        assert torch.equal(s1[rows], sp[rows]) and torch.equal(l1[rows], lp[rows]), T
        if T == 0.5:
            assert torch.equal(st, s0) and torch.equal(lt, l0)
        else:
            assert not torch.equal(sv[rows], s0[rows])
    inside = torch.arange(7, device=DEV)[None, :] < plen[:, None]
    assert torch.equal(s1[:, :7][inside], pre[inside])
    sb, lb = dec.run(seed=4, z=z)
    assert torch.equal(sb, s0) and torch.equal(lb, l0)
    if not poison:
        for bad in BAD:
            with pytest.raises(ValueError, match=cls.__name__ + ".run"):
                dec.run(seed=4, z=z, temperature=bad(B))


def test_fused_ref_temperature():
    native.require_hip()
    B, Nf = 16, 24
    m = SketchRNN(RefConfig(rnn_size=256, num_layers=2, num_mixture=24), seed=4).to(DEV)
    dec = F.FusedRefDecoder(m, B, Nf, temperature=0.3, fix_pen_temperature=True)
    group = torch.arange(B, device=DEV) % 2
    temps = torch.tensor([0.25, 1.0], device=DEV)[group]
    s0, l0 = dec.run(seed=2)
    sv, lv = dec.run(seed=2, temperature=temps)
    for i, T in enumerate((0.25, 1.0)):
        st, lt = dec.run(seed=2, temperature=T)
        fs, fl = F.FusedRefDecoder(m, B, Nf, temperature=T, fix_pen_temperature=True).run(seed=2)
        assert torch.equal(sv[group == i], st[group == i]) and torch.equal(lv[group == i], lt[group == i]), T
        assert torch.equal(st, fs) and torch.equal(lt, fl)
    s1, l1 = dec.run(seed=2)
    assert torch.equal(s1, s0) and torch.equal(l1, l0) and not torch.equal(sv, s0)
    for bad in BAD:
        with pytest.raises(ValueError, match="FusedRefDecoder.run"):
            dec.run(seed=2, temperature=bad(B))
