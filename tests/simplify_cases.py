"""Inputs shared by tests/test_simplify.py and tests/test_simplify_gpu.py: the
hand-worked cases with their tolerances, the padded synthetic corpus and the
long single strokes."""
import functools
import math

import numpy as np
import torch

from sketch_rnn_amd.data.synthetic import synthetic_corpus, synthetic_raw_corpus

INF = math.inf
HAND_N = 6

# name: (rows within the length, tol within the length). Worked out by hand
# from the definition in sketch_rnn_amd/ops/simplify.py:
HAND = {
    "L0": ([], []),
    "L1": ([(3, 4, 0)], [INF]),
    "L2": ([(1, 1, 0), (2, 0, 1)], [INF, INF]),
    # P = (0,0) (3,4) (6,0): u = (6,0), key |6*4 - 0*3| = 24, d = 24 / 6
    "L3": ([(0, 0, 0), (3, 4, 0), (3, -4, 1)], [INF, 4.0, INF]),
    "collinear": ([(1, 1, 0), (1, 1, 0), (1, 1, 1)], [INF, 0.0, INF]),
    # P = (0,0) (3,0) (3,4) (0,0): u = 0, keys 9 and 25, d = 5; then (0,2): u = (3,4), v = (3,0), key 12, d = 12/5
    "closed": ([(0, 0, 0), (3, 0, 0), (0, 4, 0), (-3, -4, 1)], [INF, 2.4, 5.0, INF]),
    # P = (0,0) (1,2) (4,2) (6,0): keys 12 and 12, the lower index splits: d = 2; then (1,3): u = (5,-2),
    # v = (3,0), key 6, d = 6/sqrt(29). (The other order would give tol = [inf, 6/sqrt(20), 2, inf].)
    "tie": ([(0, 0, 0), (1, 2, 0), (3, 0, 0), (2, -2, 1)], [INF, 2.0, 6.0 / math.sqrt(29.0), INF]),
    # runs [0..2] [3] [4..5]: P = (1,0) (2,5) (3,0): u = (2,0), key 10, d = 5
    "one-point-runs": ([(1, 0, 0), (1, 5, 0), (1, -5, 1), (7, 7, 1), (0, 3, 0), (2, 0, 1)],
                       [INF, 5.0, INF, INF, INF, INF]),
    "all-lifted": ([(1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 4, 1)], [INF] * 4),
}


def hand_batch(fill=0.0):
    """``(x [9, 6, 3], lengths, tol [9, 6])``; rows at or past the length hold ``fill``."""
    x = torch.full((len(HAND), HAND_N, 3), float(fill))
    tol = torch.full((len(HAND), HAND_N), -INF, dtype=torch.float64)
    L = []
    for b, (rows, t) in enumerate(HAND.values()):
        L.append(len(rows))
        if rows:
            x[b, :len(rows)] = torch.tensor(rows, dtype=torch.float32)
            tol[b, :len(rows)] = torch.tensor(t, dtype=torch.float64)
    return x, torch.tensor(L, dtype=torch.int64), tol


def pad(sk, N):
    x = np.zeros((len(sk), N, 3), np.float32)
    for i, s in enumerate(sk):
        x[i, :len(s)] = s
    return torch.tensor(x), torch.tensor([len(s) for s in sk], dtype=torch.int64)


@functools.lru_cache(None)
def sketches():
    return synthetic_corpus(64, seed=0, max_len=250)[0]


def corpus(B=64, N=250):
    return pad(sketches()[:B], N)


def one_stroke(points):
    """``(x [1, n, 3], lengths)`` of one pen-down stroke through ``points [n, 2]``."""
    p = np.asarray(points, np.float64)
    rows = np.zeros((1, len(p), 3), np.float32)
    rows[0, :, 0:2] = p - np.concatenate([np.zeros((1, 2)), p[:-1]], axis=0)
    rows[0, -1, 2] = 1.0
    assert (np.cumsum(rows[0, :, 0:2].astype(np.float64), axis=0) == p).all()     # float32 holds the offsets
    return torch.tensor(rows), torch.tensor([len(p)], dtype=torch.int64)


def walk_stroke(n, seed):
    """One stroke of ``n`` integer points: a random walk with steps in -9..9."""
    rng = np.random.RandomState(seed)
    return one_stroke(np.cumsum(rng.randint(-9, 10, size=(n, 2)), axis=0))


def deep_stroke(n=300):
    """``P_t = (t, (-1)^t (t+1)^2)``: every level of the recursion splits off one point."""
    t = np.arange(n)
    return one_stroke(np.stack([t, np.where(t % 2 == 0, 1, -1) * (t + 1) ** 2], axis=1))


@functools.lru_cache(None)
def raw_sketch():
    return synthetic_raw_corpus(1, seed=0)[0]
