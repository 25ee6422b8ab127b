"""Store paths and store policies of the skinny GEMM tiles (csrc/skinny_tile.h).

The tile epilogue has two paths -- 16 bytes per lane after an in-quad
transpose (16-byte aligned destination, row stride a multiple of 16 bytes)
and one element per lane in MFMA layout (anything else) -- and a store policy
(csrc/store_policy.h: plain or write-through). Every combination must store
the same bits, inside the [M, N] window only, and the chained launches, whose
producer tiles hand their slabs to cell rows of the same launch through the
write-through form, must keep their gradients bit for bit.
"""
import itertools
import math

import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.ops import gemm

from test_kernels_gpu import _hyper_run, _hyper_setup, _names, _run

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.0
GUARD_ROWS = 3
POLICIES = ("plain", "wt")
MS = (1, 5, 33, 100, 128)


@pytest.fixture(autouse=True)
def _restore():
    names = ("STORE_SLABS", "STORE_STEP", "STORE_SAVES", "GROUP_BN")
    saved = [getattr(gemm, n) for n in names]
    yield
    for n, v in zip(names, saved):
        setattr(gemm, n, v)
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    from sketch_rnn_amd.ops.recurrent import check_cluster_errors
    torch.cuda.synchronize()
    check_cluster_errors(DEV)


def _shapes(ms, ns):
    """(M, N, K-slice, splits, ldc): every combination the tile can take
    another path at -- one row, a partial 16-row MFMA block, rows in a second
    wave, the headline batch, a full tile (and row blocks with a partial
    last one); one and three N tiles; a K-slice of one K tile (shorter than
    the ring's prologue) and of three; one and two slabs; rows packed and
    rows 64 columns apart."""
    return [(M, N, ks, S, N + pad) for M, N, ks, S, pad in itertools.product(ms, ns, (64, 192), (1, 2), (0, 64))]


_OPERANDS = {}


def _operands(M, N, K):
    """bf16 operands and the fp64 product of them, computed once per shape."""
    key = (M, N, K)
    if key not in _OPERANDS:
        g = torch.Generator(device=DEV).manual_seed(1000 * M + 10 * N + K)
        a = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
        bt = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
        _OPERANDS[key] = (a, bt, a.double() @ bt.double().t())
    return _OPERANDS[key]


class _Guarded:
    """An [S, M, N] output window (row stride ld, slabs M + GUARD_ROWS rows
    apart) inside a sentinel-filled buffer, `shift` elements off the
    buffer's 16-byte aligned start."""

    def __init__(self, S, M, N, ld, shift, dtype=torch.float32):
        n = S * (M + GUARD_ROWS) * ld
        self.flat = torch.full((n + 2 * shift + 64,), SENTINEL, device=DEV, dtype=dtype)
        assert self.flat.data_ptr() % 16 == 0
        self.full = self.flat[shift:shift + n].view(S, M + GUARD_ROWS, ld)
        self.out = self.full[:, :M, :N]

    def check_band(self, what):
        band = torch.ones_like(self.flat, dtype=torch.bool)
        inside = torch.zeros_like(self.full, dtype=torch.bool)
        inside[:, :self.out.shape[1], :self.out.shape[2]] = True
        band[self.full.storage_offset():self.full.storage_offset() + self.full.numel()] = ~inside.reshape(-1)
        assert bool((self.flat[band] == SENTINEL).all()), "%s: wrote outside the [M, N] window" % (what,)


def _cell_args(keep):
    """A small LayerNorm cell backward step (2 rows, 64 units, no dh sources)
    for the cell rows of skr_skinny_gemm_group_cellbwd; `keep` holds its buffers."""
    from sketch_rnn_amd.ops._hipapi import LstmBwdArgs
    B, H = 2, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    t = {n: torch.randn(s, device=DEV, generator=g) * 0.5 for n, s in dict(
        dc_rec=(B, H), c_prev=(B, H), xhat=(B, 4 * H), chat=(B, H), ln_g=(4 * H,), ln_b=(4 * H,), lnc_g=(H,),
        lnc_b=(H,), dG=(B, 4 * H), dlny=(B, 4 * H), dlncy=(B, H)).items()}
    t["rstd"] = torch.rand(B, 5, device=DEV, generator=g) + 0.5
    keep.append(t)
    a = LstmBwdArgs()
    a.B, a.H, a.grp_rows = B, H, 0
    a.dho_nslab = a.dhr_nslab = a.dhr2_nslab = 1
    for n in ("dc_rec", "c_prev", "xhat", "rstd", "chat", "ln_g", "ln_b", "lnc_g", "lnc_b", "dG", "dlny", "dlncy"):
        setattr(a, n, t[n].data_ptr())
    a.ld_dG, a.keep, a.forget_bias = 4 * H, 1.0, 1.0
    return a, t


def _launch(kind, a, bt, out, S, keep):
    if kind == "gemm":
        gemm.rec_gemm(a, bt, out, S)
    elif kind == "bf16out":
        gemm.rec_gemm_bf16out(a, bt, out[0])
    elif kind in ("group4", "group8"):
        gemm.GROUP_BN = 128 if kind == "group8" else 0
        gemm.rec_gemm_group([(a, bt, out, S)])
    else:
        args, t = _cell_args(keep)
        gemm.rec_gemm_group_cellbwd([(a, bt, out, S)], args)
        return t["dG"]
    return None


# group8: the grouped launch runs 8 waves per tile only at 128-wide N tiles, which
# take N % 128 == 0: one and three tiles of that width. bf16out: one slab by contract.
@pytest.mark.parametrize("kind,ms,ns", [("gemm", MS, (64, 192)), ("bf16out", MS, (64, 192)),
                                        ("group4", MS + (300,), (64, 192)), ("group8", MS + (300,), (128, 384)),
                                        ("cellbwd", MS + (300,), (64, 192))])
def test_tile_store_paths_and_policies(kind, ms, ns):
    """Every (policy, path) of the tile epilogue: the vector path (aligned
    window) and the scalar fallback (the window one float further), plain and
    write-through, bit for bit; the sum of the slabs against the fp64 product
    of the bf16 operands at test_kernels_gpu.py's skinny-GEMM bound (1e-3 of
    the largest element + 1e-3); nothing stored outside the [M, N] window.
    bf16 output: the element's own rounding (half a bf16 ulp, at most 2^-8 of
    the largest element) is added to the bound, and the stored bits must equal
    the fp32 launch's slab rounded to bf16."""
    ops.set_backend("hip")
    bf = kind == "bf16out"
    keep = []
    for M, N, ks, S, ld in _shapes(ms, ns):
        if bf and S != 1:
            continue
        K = ks * S
        a, bt, ref = _operands(M, N, K)
        got, cell = {}, {}
        for pol, shift in itertools.product(POLICIES, (0, 2 if bf else 1)):
            gemm.STORE_SLABS = gemm.STORE_SAVES = pol   # (the bf16 output is a save, the fp32 ones are slabs)
            buf = _Guarded(S, M, N, ld, shift, torch.bfloat16 if bf else torch.float32)
            cell[pol, shift] = _launch(kind, a, bt, buf.out, S, keep)
            what = (kind, M, N, ks, S, ld, pol, shift)
            buf.check_band(what)
            got[pol, shift] = buf.out.clone()
        first = next(iter(got))
        for k, v in got.items():
            assert torch.equal(v, got[first]), (kind, M, N, ks, S, ld, k, "differs from", first)
            if cell[k] is not None:
                assert torch.equal(cell[k], cell[first]), (kind, "cell rows", k)
        tot = got[first].double().sum(0)
        err = (tot - ref).abs().max().item()
        top = ref.abs().max().item()
        bound = 1e-3 * top + 1e-3 + (2.0 ** -8 * top if bf else 0.0)
        print("%s M=%d N=%d ks=%d S=%d ld=%d err %.3e bound %.3e" % (kind, M, N, ks, S, ld, err, bound))
        assert err <= bound, (kind, M, N, ks, S, ld, err, bound)
        if bf:
            f32 = torch.empty(1, M, N, device=DEV)
            gemm.rec_gemm(a, bt, f32, 1)
            assert torch.equal(f32[0].to(torch.bfloat16), got[first][0]), (kind, M, N, ks, ld)


_RUNS = {}


def _ln_runs():
    """The bf16 LayerNorm-LSTM sequence at T = 3, B = 5, H = 512 (outputs,
    final states and every gradient, dropout on), run once per (policy,
    chained, poisoned) and shared by the tests below. The unchained steps run
    the row kernels (ops.recurrent.ROW_CELLS = "all"), the source the chained
    rows are compiled from: the default unchained path, the clustered cell
    kernels, sums the LayerNorm statistics in another order (measured at
    this shape against the chained run: 2.9e-07 of 0.93 on the outputs, up to
    7.8e-03 of 12.3 on the gradients)."""
    if "ln" in _RUNS:
        return _RUNS["ln"]
    from sketch_rnn_amd.ops import recurrent
    T, B, H = 3, 5, 512
    torch.manual_seed(17)
    xp = torch.randn(T, B, 4 * H, device=DEV, requires_grad=True)
    W = (torch.randn(H, 4 * H, device=DEV) / math.sqrt(H)).requires_grad_()
    h0 = (torch.randn(B, H, device=DEV) * 0.5).requires_grad_()
    c0 = (torch.randn(B, H, device=DEV) * 0.5).requires_grad_()
    lnp = [torch.randn(4 * H, device=DEV).mul(0.1).add(1).requires_grad_(),
           torch.randn(4 * H, device=DEV).mul(0.1).requires_grad_(),
           torch.randn(H, device=DEV).mul(0.1).add(1).requires_grad_(),
           torch.randn(H, device=DEV).mul(0.1).requires_grad_()]
    seed = torch.tensor([23], device=DEV)

    def fn(xp, W, h0, c0, *lnp):
        out, (hT, cT) = ops.lstm_sequence(xp, W, h0, c0, drop_keep=0.9, drop_seed=seed, drop_stream=5, ln=tuple(lnp))
        return [out, hT, cT]

    saved = recurrent.LN_CHAIN, recurrent.LN_CHAIN_POISON, gemm.STORE_SLABS, recurrent.ROW_CELLS
    ops.set_compute_dtype("bf16")
    res = {}
    try:
        recurrent.ROW_CELLS = "all"
        for pol, chain, pois in _CASES:
            gemm.STORE_SLABS = pol
            recurrent.LN_CHAIN, recurrent.LN_CHAIN_POISON = chain, pois
            n0, r0 = dict(recurrent.LN_CHAIN_STATS), recurrent.ROW_STATS["row"]
            o, g = _run("hip", fn, [xp, W, h0, c0] + lnp)
            if not chain:   # every unchained step, forward and backward, on the row kernels
                assert recurrent.ROW_STATS["row"] - r0 == 2 * T, (pol, recurrent.ROW_STATS["row"] - r0)
            res[pol, chain, pois] = o + g
            ran = (recurrent.LN_CHAIN_STATS["fwd"] - n0["fwd"], recurrent.LN_CHAIN_STATS["bwd"] - n0["bwd"])
            assert ran == ((T, T - 1) if chain else (0, 0)), (pol, chain, ran)
    finally:
        recurrent.LN_CHAIN, recurrent.LN_CHAIN_POISON, gemm.STORE_SLABS, recurrent.ROW_CELLS = saved
        ops.set_compute_dtype("fp32")
    names = ["out", "hT", "cT", "dxp", "dW", "dh0", "dc0", "dln_g", "dln_b", "dlnc_g", "dlnc_b"]
    _RUNS["ln"] = (names, res)
    return _RUNS["ln"]


def _hyper_runs():
    """The bf16 HyperLSTM sequence at T = 3, B = 5, H = 2048, Hh = 256
    (outputs, final states, dz and every weight gradient, dropout on), run
    once per (policy, chained, poisoned) and shared by the tests below."""
    if "hyper" in _RUNS:
        return _RUNS["hyper"]
    from sketch_rnn_amd.ops import hyper
    from sketch_rnn_amd.ops.recurrent import ROW_STATS
    T, B = 3, 5
    p, x, z, st, w = _hyper_setup(4, T, B, 5, 16, 2048, 256, 32, jitter=0.02, state=0.1)
    saved = hyper.CHAIN, hyper.CHAIN_POISON, gemm.STORE_SLABS
    res = {}
    try:
        ops.set_backend("hip")
        ops.set_compute_dtype("bf16")
        for pol, chain, pois in _CASES:
            gemm.STORE_SLABS = pol
            hyper.CHAIN, hyper.CHAIN_POISON = chain, pois
            n0 = ROW_STATS["chain"]
            res[pol, chain, pois] = _hyper_run(p, x, z, st, w, keep=0.9, hkeep=0.9)
            assert ROW_STATS["chain"] - n0 == (T - 1 if chain else 0), (pol, chain)
    finally:
        hyper.CHAIN, hyper.CHAIN_POISON, gemm.STORE_SLABS = saved
        ops.set_compute_dtype("fp32")
    _RUNS["hyper"] = (_names(p), res)
    return _RUNS["hyper"]


# (policy, chained, NaN-poisoned slabs)
_CASES = [("plain", False, False), ("wt", False, False), ("plain", True, False), ("plain", True, True),
          ("wt", True, False), ("wt", True, True)]


@pytest.mark.parametrize("runs", [_ln_runs, _hyper_runs], ids=["ln", "hyper"])
def test_chain_store_policies_bitwise(runs):
    """The chained launches (csrc/chain_step.hip: producer tiles hand their
    slabs to the cell rows of the same launch through write-through stores,
    16 bytes per lane in the HyperLSTM chain, dwords in the LayerNorm-LSTM
    chains) and their unchained twins: every store policy equals plain bit
    for bit, chained and unchained, and a run with NaN-poisoned slabs (a row
    reading ahead of its producers would carry NaN) equals the unpoisoned one."""
    names, res = runs()
    for i, n in enumerate(names):
        assert torch.equal(res["wt", False, False][i], res["plain", False, False][i]), n
        for k in _CASES[3:]:
            assert torch.isfinite(res[k][i]).all(), (n, k)
            assert torch.equal(res[k][i], res["plain", True, False][i]), (n, k)


@pytest.mark.parametrize("runs", [_ln_runs, _hyper_runs], ids=["ln", "hyper"])
def test_chained_equals_unchained_bitwise(runs):
    """Chained against unchained, every output and gradient bit for bit.

    ln: the unchained steps run the row kernels, the body the chained rows
    are compiled from (see _ln_runs). The forward body fuses its multiply-adds
    per expression (csrc/row_cell.h): with the compiler free to pick the
    pairs, the two kernels differed in the last bit (out 2.4e-07 of 0.93,
    dxp 7.2e-07 of 7.7, dc0 4.8e-07 of 7.1)."""
    names, res = runs()
    worst = []
    for i, n in enumerate(names):
        c, u = res["plain", True, True][i].float(), res["plain", False, False][i].float()
        d = (c - u).abs().max().item()
        print("%s: chained - unchained max %.3e (largest element %.3e)" % (n, d, u.abs().max().item()))
        if not torch.equal(c, u):
            worst.append((n, d))
    assert not worst, worst


def test_hyper_mod_store_policies_bitwise():
    """One modulation step (csrc/hyper_mod.hip) at B = 3: the gate
    pre-activations, their LayerNorm partial sums, the saved modulation
    vectors and the saved bf16 R, bit for bit under every combination of the
    step-output and save store policies, with sentinel-filled rows past B
    untouched."""
    import ctypes
    from sketch_rnn_amd.utils import native
    lib = native.require_hip()
    B, H, Hh, GR = 3, 64, 256, 2
    g = torch.Generator(device=DEV).manual_seed(11)
    hh = torch.randn(B, Hh, device=DEV, generator=g).to(torch.bfloat16)
    PlT = (torch.randn(12 * H, Hh, device=DEV, generator=g) / 16).to(torch.bfloat16)
    qb = torch.randn(12 * H, device=DEV, generator=g)
    xh = torch.randn(B, 4 * H, device=DEV, generator=g)
    R = torch.randn(2, B, 4 * H, device=DEV, generator=g)
    res = {}
    try:
        for step, saves in itertools.product(POLICIES, POLICIES):
            gemm.STORE_STEP, gemm.STORE_SAVES = step, saves
            gemm.apply_store_policy(lib)
            vec = torch.full((B + GR, 12 * H), SENTINEL, device=DEV, dtype=torch.bfloat16)
            gp = torch.full((B + GR, 4 * H), SENTINEL, device=DEV)
            rlp = torch.full((B + GR, 4 * H), SENTINEL, device=DEV, dtype=torch.bfloat16)
            stats = torch.full((B + GR, 4, H // 32, 2), SENTINEL, device=DEV)
            rc = lib.lib.skr_hyper_mod_fwd(hh.data_ptr(), Hh, PlT.data_ptr(), qb.data_ptr(), xh.data_ptr(), R.data_ptr(),
                                           B * 4 * H, 2, vec.data_ptr(), gp.data_ptr(), rlp.data_ptr(), stats.data_ptr(),
                                           B, H, Hh, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            torch.cuda.synchronize()
            res[step, saves] = (vec, gp, rlp, stats)
    finally:
        pass
    base = res["plain", "plain"]
    assert torch.isfinite(base[1][:B]).all() and not bool((base[1][:B] == SENTINEL).any())
    for k, r in res.items():
        for n, x, y in zip(("vec", "g", "rlp", "stats"), r, base):
            assert torch.equal(x, y), (k, n)
            assert bool((x[B:] == SENTINEL).all()), (k, n, "rows past B written")
    assert bool((base[0][:B, 8 * H:] == SENTINEL).all())   # (the shift block is not stored)

