"""The RDP kernel (csrc/simplify.hip) on the GPU: bit for bit against the host
references on integer-valued input, where every step is exact or correctly
rounded on both sides (integer sums and cross products below 2^53 are exact
in any order, sqrt and division are correctly rounded, contraction is off);
within a margin computed from the reference alone on general floats; poisoned
padding, repeats, per-row epsilon, the fit, a captured graph and the CLI."""
import math
import os

import numpy as np
import pytest
import torch

from sketch_rnn_amd import ops
from sketch_rnn_amd.cli import preprocess
from sketch_rnn_amd.data.strokes import to_big_strokes
from sketch_rnn_amd.ops import simplify as S

import simplify_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quickdraw_tiny.ndjson")


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_backend("auto")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _bitwise(x, L, eps=2.0, max_len=None, host=False):
    """Kernel and references agree bit for bit; returns the kernel's results on the host."""
    tol_ref = S.rdp_tolerance_reference(x, L)
    ref = S.simplify_reference(x, L, epsilon=eps, max_len=max_len)
    xd, Ld = x.to(DEV), (None if L is None else L.to(DEV))
    if host:                                    # past MAX_N the dispatcher takes the host path
        tol, got = S.rdp_tolerance(xd, Ld), S.simplify(xd, Ld, epsilon=eps, max_len=max_len)
    else:
        tol, got = S.rdp_tolerance_hip(xd, Ld), S.simplify_hip(xd, Ld, epsilon=eps, max_len=max_len)
    assert tol.is_cuda and tol.dtype == torch.float64 and all(t.is_cuda for t in got)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.float64
    tol, got = tol.cpu(), tuple(t.cpu() for t in got)
    assert torch.equal(_bits(tol), _bits(tol_ref))
    assert torch.equal(got[1], ref[1]), (got[1], ref[1])
    assert torch.equal(_bits(got[2]), _bits(ref[2]))
    assert torch.equal(got[0], ref[0])
    return tol, got


def test_hand_cases_bitwise():
    x, L, want = SC.hand_batch(fill=float("nan"))
    for eps in (0.0, 2.4, 4.0):
        tol, _ = _bitwise(x, L, eps)
        assert torch.equal(tol, want)
    clean, _, _ = SC.hand_batch()
    x5 = torch.tensor(np.stack([to_big_strokes(clean[b, :int(L[b])].numpy(), SC.HAND_N) for b in range(len(L))]))
    tol, got = _bitwise(x5, None, 1.0)
    assert torch.equal(tol, want) and got[0][0].tolist() == [[0, 0, 0, 0, 1]] * SC.HAND_N


@pytest.mark.parametrize("n", [65, 257, 300, 512, 513])
def test_one_stroke_bitwise(n):
    """Past one wave, past one pass of the 256-thread workgroup, and both sides of the tier boundary."""
    x, L = SC.walk_stroke(n, seed=n)
    _, got = _bitwise(x, L, 2.0)
    assert 2 <= int(got[1][0]) < n
    _bitwise(x, L, 2.0, max_len=17)


def test_corpus_bitwise():
    x, L = SC.corpus(8, 250)
    _, got = _bitwise(x, L, 2.0)
    assert int(got[1].sum()) < int(L.sum())
    # multiples of 2^-10: the sums are exact too
    y = x.clone()
    y[..., 0:2] = torch.round(x[..., 0:2] / 11.37 * 1024.0) / 1024.0
    _bitwise(y, L, 0.25)


def test_deep_recursion_bitwise():
    """298 levels: every level splits off one point."""
    x, L = SC.deep_stroke(300)
    rounds = torch.zeros(1, dtype=torch.int32, device=DEV)
    S.rdp_tolerance_hip(x.to(DEV), L.to(DEV), rounds=rounds)
    assert int(rounds[0]) == 298
    _bitwise(x, L, 2.0)


def test_raw_trace_bitwise_and_host_path_past_max_n():
    s = SC.raw_sketch()
    assert len(s) == S.MAX_N == 2048
    x, L = SC.pad([s], S.MAX_N)
    _, a = _bitwise(x, L, 2.0, max_len=250)
    assert int(a[1][0]) <= 250 and float(a[2][0]) > 2.0
    x1, _ = SC.pad([s], S.MAX_N + 1)
    _, b = _bitwise(x1, L, 2.0, max_len=250, host=True)
    assert torch.equal(a[0][0], b[0][0, :S.MAX_N]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        S.simplify_hip(x1.to(DEV), L.to(DEV))


def _margin(P, runs, eps_list):
    """The smallest relative gap, over every split of the full recursion, between
    the winning key and the runner-up and between the split's distance and each
    tested epsilon. The split term is (k_1st - k_2nd) / bound, skipped for an exact
    tie or a single candidate; the threshold term |d - eps| |u| / bound; bound =
    (|u_x| + |u_y|) max_t (|v_tx| + |v_ty|) bounds the key's magnitude, so both are
    relative to what a perturbation of the points can move. In the degenerate
    branch bound = max k and the threshold term is |d - eps| / max(d, eps). A
    margin of 1e-9 is four orders above the reordering noise N 2^-53 ~ 3e-14 of the
    kernel's scan against cumsum; below it a near tie may fall the other way."""
    best = INF
    for s, e in runs:
        stack = [(s, e)]
        while stack:
            l, r = stack.pop()
            if r - l < 2:
                continue
            ux, uy = P[r] - P[l]
            v = P[l + 1:r] - P[l]
            uu = ux * ux + uy * uy
            if uu > 0:
                k = np.abs(ux * v[:, 1] - uy * v[:, 0])
                bound = (abs(ux) + abs(uy)) * float((np.abs(v[:, 0]) + np.abs(v[:, 1])).max())
                d = float(k.max()) / math.sqrt(uu)
                thr = [abs(d - eps) * math.sqrt(uu) / bound for eps in eps_list]
            else:
                k = (v * v).sum(axis=1)
                bound = float(k.max())
                d = math.sqrt(bound)
                thr = [abs(d - eps) / max(d, eps) for eps in eps_list]
            srt = np.sort(k)
            if len(k) > 1 and srt[-1] != srt[-2]:
                best = min(best, float(srt[-1] - srt[-2]) / bound)
            best = min([best] + thr)
            m = l + 1 + int(np.argmax(k))
            stack += [(l, m), (m, r)]
    return best


def test_general_floats_within_margin():
    g = torch.Generator().manual_seed(7)
    B, N, eps_list = 16, 300, (0.5, 2.0)
    x = torch.randn(B, N, 3, generator=g)
    x[..., 2] = (torch.rand(B, N, generator=g) < 0.03).float()
    L = torch.full((B,), N, dtype=torch.int64)
    xn = x.double().numpy()
    margins, extent = [], []
    for b in range(B):
        P, runs = S._points_and_runs(xn[b], N, 3)
        margins.append(_margin(P, runs, eps_list))
        extent.append(float(np.abs(P).max()))
    print("margins: min %.3g, all %s" % (min(margins), ["%.2g" % m for m in margins]))
    assert min(margins) >= 1e-9                  # all 16 sketches qualify
    tol_ref = S.rdp_tolerance_reference(x, L)
    tol = S.rdp_tolerance_hip(x.to(DEV), L.to(DEV)).cpu()
    extent = torch.tensor(extent, dtype=torch.float64).unsqueeze(1)
    finite = torch.isfinite(tol_ref)
    assert torch.equal(torch.isfinite(tol), finite) and torch.equal(tol[~finite], tol_ref[~finite])
    err = ((tol - tol_ref).abs() / extent)[finite]
    print("largest |tol_k - tol_ref| / extent: %.3g" % float(err.max()))
    assert float(err.max()) <= 1e-9
    for eps in eps_list:
        ref = S.simplify_reference(x, L, epsilon=eps)
        got = tuple(t.cpu() for t in S.simplify_hip(x.to(DEV), L.to(DEV), epsilon=eps))
        assert torch.equal(got[1], ref[1])
        assert torch.equal((tol > eps) | (tol == INF), (tol_ref > eps) | (tol_ref == INF))     # kept sets
        assert torch.equal(got[0][..., 2], ref[0][..., 2])
        d = float((got[0] - ref[0]).abs().max())
        print("eps %.1f: largest |out_k - out_ref| %.3g of %.3g" % (eps, d, float(ref[0].abs().max())))
        assert d <= 2.0 ** -23 * float(ref[0].abs().max())


def test_poison_and_repeat():
    x, L = SC.corpus(8, 250)
    clean = [S.rdp_tolerance(x.to(DEV), L.to(DEV))] + list(S.simplify(x.to(DEV), L.to(DEV), 2.0, 40))
    poisoned = x.clone()
    for b, n in enumerate(L.tolist()):
        poisoned[b, n:] = float("nan")
    for y in (poisoned, x):                     # rows past the lengths change nothing; two calls agree
        again = [S.rdp_tolerance(y.to(DEV), L.to(DEV))] + list(S.simplify(y.to(DEV), L.to(DEV), 2.0, 40))
        for a, b in zip(clean, again):
            assert torch.equal(_bits(a) if a.dtype == torch.float64 else a, _bits(b) if b.dtype == torch.float64 else b)


def test_epsilon_tensor_equals_scalar_calls():
    x, L = (t.to(DEV) for t in SC.corpus(8, 250))
    eps = torch.tensor([0.0, 0.5, 1.0, 2.0, 3.5, 5.0, 20.0, 1e6], device=DEV)
    out, n, used = S.simplify(x, L, eps)
    assert torch.equal(used, eps.double())
    for b in range(8):
        o, k, u = S.simplify(x[b:b + 1], L[b:b + 1], float(eps[b]))
        assert torch.equal(out[b:b + 1], o) and torch.equal(n[b:b + 1], k) and torch.equal(used[b:b + 1], u)
    with pytest.raises(ValueError):
        S.simplify(x, L, -eps - 1.0)


@pytest.mark.parametrize("max_len", [1, 10, 40])
def test_fit_bitwise(max_len):
    x, L = SC.corpus(8, 250)
    _, got = _bitwise(x, L, 0.5, max_len=max_len)
    cannot = got[2] == INF
    assert bool(((got[1] <= max_len) | cannot).all())
    if max_len == 1:                            # the ends of several strokes: epsilon +inf, the length reported
        assert bool(cannot.all()) and bool((got[1] > 1).all())
    else:
        assert bool((got[2][~cannot] > 0.5).any())


def test_graph_capture_replays_the_eager_call():
    x, L = (t.to(DEV) for t in SC.corpus(8, 250))
    eps = torch.full((8,), 2.0, device=DEV)
    bx, bL = torch.flip(x, dims=[0]).clone(), torch.flip(L, dims=[0]).clone()       # warm-up and capture on these
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.simplify(bx, bL, eps, 40)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, n, used = S.simplify(bx, bL, eps, 40)
    bx.copy_(x)                                                                     # new contents, same buffers
    bL.copy_(L)
    eps.fill_(1.0)
    g.replay()
    torch.cuda.synchronize()
    eo, en, eu = S.simplify(x, L, 1.0, 40)
    assert torch.equal(out, eo) and torch.equal(n, en) and torch.equal(used, eu)
    assert not torch.equal(n, torch.flip(n, dims=[0]))


def test_cli_same_pack_on_both_backends(tmp_path):
    """Byte-identical packs: every member of the two archives holds the same bytes
    (the archives themselves carry the time of writing in their zip headers)."""
    import zipfile
    packs = []
    for backend in ("hip", "torch"):
        ops.set_backend(backend)
        path = str(tmp_path / (backend + ".skpack.npz"))
        assert preprocess.main(["ndjson", path, FIXTURE, "--all", "--fit", "--max_len", "50", "--valid", "1",
                                "--test", "1"]) == 0
        with zipfile.ZipFile(path) as z:
            packs.append([(name, z.read(name)) for name in z.namelist()])
    assert packs[0] == packs[1] and len(packs[0]) == 9 and sum(len(b) for _, b in packs[0]) > 1000


def test_empty_batches():
    for B, N in ((0, 4), (3, 0)):
        x, L = torch.zeros(B, N, 3, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
        rounds = torch.full((B,), 7, dtype=torch.int32, device=DEV)
        tol = S.rdp_tolerance_hip(x, L, rounds=rounds)
        out, n, used = S.simplify_hip(x, L, epsilon=1.5, max_len=2)
        assert tol.shape == (B, N) and tol.dtype == torch.float64 and out.shape == (B, N, 3)
        assert n.tolist() == [0] * B and used.tolist() == [1.5] * B and rounds.tolist() == [0] * B
