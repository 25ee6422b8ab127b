"""RDP simplification on the host (sketch_rnn_amd/ops/simplify.py): the
tolerance formulation against hand-worked values and against classical RDP,
the fit to a length, the round trip, the ndjson reader and the two
``preprocess`` subcommands on a hand-written fixture."""
import math
import os

import numpy as np
import pytest
import torch

from sketch_rnn_amd.cli import preprocess
from sketch_rnn_amd.data.quickdraw import load_ndjson, load_pack, normalize_drawing, simplify_corpus
from sketch_rnn_amd.data.strokes import to_big_strokes
from sketch_rnn_amd.data.synthetic import synthetic_raw_corpus
from sketch_rnn_amd.ops import simplify as S

import simplify_cases as SC

INF = math.inf
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quickdraw_tiny.ndjson")


def _kept(tol, eps):
    return (tol > eps) | (tol == INF)


def test_hand_cases_tolerance():
    x, L, want = SC.hand_batch()
    tol = S.rdp_tolerance_reference(x, L)
    assert tol.dtype == torch.float64 and tol.shape == (len(SC.HAND), SC.HAND_N)
    assert torch.equal(tol, want), (tol, want)
    # every route of the dispatcher gives the same on the host
    assert torch.equal(S.rdp_tolerance(x, L), want)


def test_hand_cases_output():
    x, L, _ = SC.hand_batch()
    names = list(SC.HAND)
    out, n, eps = S.simplify_reference(x, L, epsilon=0.0)
    assert out.dtype == torch.float32 and n.dtype == torch.int64 and eps.dtype == torch.float64
    assert n.tolist() == [0, 1, 2, 3, 2, 4, 4, 6, 4] and eps.tolist() == [0.0] * 9
    assert float(out[names.index("L0")].abs().max()) == 0.0
    assert out[names.index("L1")].tolist() == [[3, 4, 0]] + [[0, 0, 0]] * 5
    # collinear: tol = 0 is not > 0, the middle point goes and the offsets add up
    assert out[names.index("collinear")].tolist() == [[1, 1, 0], [2, 2, 1]] + [[0, 0, 0]] * 4
    assert torch.equal(out[names.index("all-lifted")], x[names.index("all-lifted")])
    out, n, _ = S.simplify_reference(x, L, epsilon=2.4)
    assert n.tolist() == [0, 1, 2, 3, 2, 3, 2, 6, 4]
    # closed: (3, 0) has tol 2.4 and goes, (3, 4) stays
    assert out[names.index("closed")].tolist() == [[0, 0, 0], [3, 4, 0], [-3, -4, 1]] + [[0, 0, 0]] * 3
    out, n, _ = S.simplify_reference(x, L, epsilon=4.0)
    assert n.tolist() == [0, 1, 2, 2, 2, 3, 2, 6, 4]


def test_stroke5_and_poisoned_rows():
    x, L, want = SC.hand_batch()
    x5 = torch.tensor(np.stack([to_big_strokes(x[b, :int(L[b])].numpy(), SC.HAND_N) for b in range(len(L))]))
    assert torch.equal(S.rdp_tolerance_reference(x5), want)            # lengths=None: stroke5_lengths
    o3, n3, _ = S.simplify_reference(x, L, epsilon=1.0)
    o5, n5, _ = S.simplify_reference(x5, None, epsilon=1.0)
    assert torch.equal(n3, n5)
    for b in range(len(L)):
        k = int(n3[b])
        assert torch.equal(o5[b, :k, 0:2], o3[b, :k, 0:2]) and torch.equal(o5[b, :k, 3], o3[b, :k, 2])
        assert torch.equal(o5[b, :k, 2], 1 - o3[b, :k, 2])               # the pen columns of the kept rows
        assert o5[b, k:].tolist() == [[0, 0, 0, 0, 1]] * (SC.HAND_N - k)
    xn, _, _ = SC.hand_batch(fill=float("nan"))
    assert torch.equal(S.rdp_tolerance_reference(xn, L), want)
    on, nn, _ = S.simplify_reference(xn, L, epsilon=1.0)
    assert torch.equal(on, o3) and torch.equal(nn, n3)


@pytest.mark.parametrize("eps", [0.0, 0.5, 2.0, 5.0, 20.0])
def test_tolerance_against_classical_rdp(eps):
    x, L = SC.corpus()
    tol = S.rdp_tolerance_reference(x, L)
    out, n, used = S.simplify_reference(x, L, epsilon=eps)
    kept = _kept(tol, eps)
    assert torch.equal(kept.sum(1), n) and used.tolist() == [eps] * 64
    P = torch.cumsum(x[..., 0:2].double(), dim=1)
    for b in range(64):
        k = torch.nonzero(kept[b]).flatten()
        assert torch.equal(torch.cumsum(out[b, :len(k), 0:2].double(), dim=0), P[b, k])      # the same points
        assert torch.equal(out[b, :len(k), 2], x[b, k, 2])
        assert float(out[b, len(k):].abs().max() if len(k) < 250 else 0.0) == 0.0
    assert int(n.sum()) < int(L.sum()) or eps == 0.0


def test_corpus_has_exact_ties():
    """The tie rule is exercised: some top-level segment of the corpus has two equal largest keys."""
    x, L = SC.corpus()
    ties = 0
    for b in range(64):
        P, runs = S._points_and_runs(x[b].double().numpy(), int(L[b]), 3)
        for s, e in runs:
            if e - s >= 3:
                ux, uy = P[e] - P[s]
                v = P[s + 1:e] - P[s]
                k = np.abs(ux * v[:, 1] - uy * v[:, 0]) if ux * ux + uy * uy > 0 else (v * v).sum(1)
                ties += int((k == k.max()).sum() > 1)
    assert ties >= 1, ties


@pytest.mark.parametrize("max_len", [1, 10, 40])
def test_fit(max_len):
    x, L = SC.corpus()
    tol = S.rdp_tolerance_reference(x, L)
    out, n, used = S.simplify_reference(x, L, epsilon=0.5, max_len=max_len)
    fits = n <= max_len
    assert bool((fits | (used == INF)).all())
    assert bool((used >= 0.5).all())
    # every corpus sketch has several strokes: none fits one point, some fit ten
    assert int(fits.sum()) == 0 if max_len == 1 else int(fits.sum()) > 0
    for b in range(64):
        t = tol[b, :int(L[b])]
        if used[b] == INF:
            assert int((t == INF).sum()) > max_len and int(n[b]) == int((t == INF).sum())
            continue
        assert int(n[b]) == int(_kept(t, used[b]).sum())
        if used[b] > 0.5:
            # the next smaller threshold (a tolerance value, 0.5 or 0) overshoots
            lower = [v for v in t.tolist() + [0.5, 0.0] if v < float(used[b])]
            assert int((t > max(lower)).sum()) > max_len
            assert float(used[b]) in t.tolist()
    # an epsilon above the fit wins
    out2, n2, used2 = S.simplify_reference(x, L, epsilon=1e6, max_len=40)
    assert bool(((used2 == 1e6) | (used2 == INF)).all()) and int((used2 == 1e6).sum()) > 0


def test_round_trip_on_raw_traces():
    sk = synthetic_raw_corpus(3, seed=0)
    assert len(sk[0]) == 2048 and all((s == np.round(s)).all() for s in sk)
    again = synthetic_raw_corpus(3, seed=0)
    assert all((a == b).all() for a, b in zip(sk, again))
    x, L = SC.pad(sk, 2048)
    tol = S.rdp_tolerance_reference(x, L)
    out, n, used = S.simplify_reference(x, L, epsilon=2.0, max_len=250)
    assert bool((n <= 250).all()) and float(used[0]) > 2.0
    P = torch.cumsum(x[..., 0:2].double(), dim=1)
    for b in range(3):
        k = torch.nonzero(_kept(tol[b], float(used[b]))).flatten()
        assert len(k) == int(n[b])
        assert torch.equal(torch.cumsum(out[b, :len(k), 0:2].double(), dim=0), P[b, k])
        assert torch.equal(out[b, :len(k), 2], x[b, k, 2])


def test_argument_validation():
    x, L, _ = SC.hand_batch()
    for fn in (S.rdp_tolerance_reference, S.rdp_tolerance, S.simplify_reference, S.simplify):
        with pytest.raises(ValueError):
            fn(x[0], L)                              # not [B, N, D]
        with pytest.raises(ValueError):
            fn(x[..., :2], L)                        # D = 2
        with pytest.raises(ValueError):
            fn(x.long(), L)                          # integer strokes
        with pytest.raises(ValueError):
            fn(x, None)                              # stroke-3 without lengths
        with pytest.raises(ValueError):
            fn(x, L[:3])
        with pytest.raises(ValueError):
            fn(x, L.float())
    for fn in (S.simplify_reference, S.simplify):
        for eps in (-1.0, INF, float("nan"), "2", torch.full((3,), 2.0), torch.full((9,), -1.0),
                    torch.full((9,), 2, dtype=torch.int64)):
            with pytest.raises(ValueError):
                fn(x, L, epsilon=eps)
        for k in (0, -3, 2.5, True):
            with pytest.raises(ValueError):
                fn(x, L, max_len=k)
    with pytest.raises(ValueError):
        S.simplify_hip(x, L)                         # host strokes on the kernel path
    with pytest.raises(ValueError):
        S.rdp_tolerance_hip(x, L)
    out, n, used = S.simplify(x, L, epsilon=torch.linspace(0.0, 4.0, 9))
    assert used.tolist() == torch.linspace(0.0, 4.0, 9).double().tolist()


def test_load_ndjson_and_normalize():
    drawings, words = load_ndjson(FIXTURE)
    assert words == ["zigzag", "house", "eye", "circle"]
    assert [len(d) for d in drawings] == [2, 3, 2, 1] and [sum(len(l) for l in d) for d in drawings] == [9, 12, 6, 400]
    everything, words_all = load_ndjson(FIXTURE, recognized_only=False)
    assert len(everything) == 5 and words_all[2] == "scribble"
    assert len(load_ndjson(FIXTURE, limit=2)[0]) == 2
    for d in everything:
        s = normalize_drawing(d)
        assert s.dtype == np.float32 and s.shape[1] == 3 and (s == np.round(s)).all()
        P = np.cumsum(s[:, 0:2].astype(np.float64), axis=0)
        assert P.min(axis=0).tolist() == [0.0, 0.0] and float(P.max()) == 255.0
        assert int(s[:, 2].sum()) == len(d) and s[-1, 2] == 1.0
    # the drawing that already fills the canvas keeps its coordinates
    house = normalize_drawing(drawings[1])
    assert np.cumsum(house[:, 0:2], axis=0)[:5].tolist() == [[0, 100], [0, 255], [255, 255], [255, 100], [0, 100]]
    # a point-sized drawing: scale 1; equal neighbours within a stroke collapse to one point
    dot = normalize_drawing([np.array([[7.0, 9.0], [7.0, 9.0]])])
    assert dot.tolist() == [[0.0, 0.0, 1.0]]
    assert normalize_drawing([np.array([[0.0, 0.0], [0.1, 0.0], [510.0, 0.0]])]).tolist() == [[0, 0, 0], [255, 0, 1]]


def test_simplify_corpus_orders_and_drops():
    sk = [normalize_drawing(d) for d in load_ndjson(FIXTURE, recognized_only=False)[0]]
    out, eps, dropped = simplify_corpus(sk, epsilon=2.0, max_len=None, batch=2, device="cpu")
    assert [len(s) for s in out][:4] == [8, 12, 5, 6] and 50 < len(out[4]) < 400 and dropped == []
    assert eps.tolist() == [2.0] * 5
    ref, n, _ = S.simplify_reference(*SC.pad(sk, 400), epsilon=2.0)
    for s, r, k in zip(out, ref, n):
        assert np.array_equal(s, r[:int(k)].numpy())
    out, eps, dropped = simplify_corpus(sk, epsilon=2.0, max_len=50, batch=2, device="cpu")
    assert len(out[4]) <= 50 and eps[4] > 2.0 and eps[:4].tolist() == [2.0] * 4 and dropped == []
    out, eps, dropped = simplify_corpus(sk, epsilon=2.0, max_len=2, device="cpu")
    assert dropped == [0, 1, 3] and eps[0] == INF and len(out[0]) == 4       # three strokes cannot fit two points


def test_cli_ndjson_and_simplify(tmp_path, capsys):
    pack = str(tmp_path / "tiny.skpack.npz")
    assert preprocess.main(["ndjson", pack, FIXTURE, FIXTURE, "--max_len", "50", "--valid", "1", "--test", "1"]) == 0
    said = capsys.readouterr().out
    assert "read 8 sketches, kept 6, dropped 2 " in said, said        # the circle of each file
    p = load_pack(pack)
    assert [len(p[k][0]) for k in ("train", "valid", "test")] == [2, 2, 2]
    assert p["train"][1].tolist() == [0, 1] and p["test"][1].tolist() == [0, 1]
    assert max(len(s) for k in p for s in p[k][0]) <= 50
    fitted = str(tmp_path / "fit.skpack.npz")
    assert preprocess.main(["ndjson", fitted, FIXTURE, "--all", "--fit", "--max_len", "50", "--valid", "1",
                            "--test", "1"]) == 0
    said = capsys.readouterr().out
    assert "read 5 sketches, kept 5, dropped 0 " in said, said
    f = load_pack(fitted)
    assert [len(f[k][0]) for k in ("train", "valid", "test")] == [3, 1, 1]
    circle = f["test"][0][0]
    assert 40 <= len(circle) <= 50 and (circle == np.round(circle)).all()
    # simplify on the pack: harder, every split, labels carried
    again = str(tmp_path / "again.skpack.npz")
    assert preprocess.main(["simplify", fitted, again, "--epsilon", "10", "--max_len", "12"]) == 0
    said = capsys.readouterr().out
    assert "read 5 sketches, kept 4, dropped 1 " in said, said        # the circle still has more than 12 points
    g = load_pack(again)
    assert [len(g[k][0]) for k in ("train", "valid", "test")] == [3, 1, 0]
    assert all(len(a) <= len(b) for k in ("train", "valid") for a, b in zip(g[k][0], f[k][0]))
    assert preprocess.main(["simplify", fitted, again, "--epsilon", "10", "--max_len", "12", "--fit"]) == 0
    assert "kept 5, dropped 0 " in capsys.readouterr().out
    assert len(load_pack(again)["test"][0][0]) <= 12


def test_empty_batches():
    for B, N in ((0, 4), (3, 0)):
        x, L = torch.zeros(B, N, 3), torch.zeros(B, dtype=torch.int64)
        assert S.rdp_tolerance_reference(x, L).shape == (B, N)
        out, n, used = S.simplify_reference(x, L, epsilon=1.5, max_len=2)
        assert out.shape == (B, N, 3) and n.tolist() == [0] * B and used.tolist() == [1.5] * B
