"""QuickDraw-style stroke-3 corpora.

Two on-disk formats are supported:

* **sketch pack** (``.skpack.npz``, this framework's own, pickle-free): per
  split ``{split}_points`` int16/float32 ``[N, 3]``, ``{split}_offsets``
  int64 ``[n + 1]`` and optional ``{split}_labels``;
* the public QuickDraw ``.npz`` whose ``train/valid/test`` entries are object
  arrays. Those need NumPy's pickle path, so reading one requires the
  caller to pass ``allow_pickle=True`` explicitly for a file they trust;
  :func:`convert_to_pack` turns it into a sketch pack once.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

SPLITS = ("train", "valid", "test")


def save_pack(path: str, splits: Dict[str, Tuple[Sequence[np.ndarray], Sequence[int]]]) -> None:
    arrays = {}
    for name, (strokes, labels) in splits.items():
        off = np.zeros(len(strokes) + 1, dtype=np.int64)
        for k, s in enumerate(strokes):
            off[k + 1] = off[k] + len(s)
        pts = np.concatenate([np.asarray(s, np.float32) for s in strokes], 0) if len(strokes) else \
            np.zeros((0, 3), np.float32)
        arrays[name + "_points"] = pts
        arrays[name + "_offsets"] = off
        arrays[name + "_labels"] = np.asarray(labels, dtype=np.int64)
    np.savez(path, **arrays)


def load_pack(path: str) -> Dict[str, Tuple[List[np.ndarray], np.ndarray]]:
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for name in SPLITS:
            if name + "_points" not in z:
                continue
            pts, off = z[name + "_points"], z[name + "_offsets"]
            labels = z[name + "_labels"] if name + "_labels" in z else np.zeros(len(off) - 1, np.int64)
            out[name] = ([np.asarray(pts[off[k]:off[k + 1]], np.float32) for k in range(len(off) - 1)], labels)
    return out


def load_quickdraw_npz(path: str, allow_pickle: bool = False, label: int = 0):
    """Read a public QuickDraw ``.npz`` (object arrays of stroke-3)."""
    with np.load(path, encoding="latin1", allow_pickle=allow_pickle) as z:
        out = {}
        for name in SPLITS:
            if name in z:
                arr = z[name]
                strokes = [np.asarray(s, dtype=np.float32) for s in arr]
                out[name] = (strokes, np.full(len(strokes), label, dtype=np.int64))
    return out


def convert_to_pack(npz_paths: Sequence[str], out_path: str, allow_pickle: bool = False) -> None:
    merged: Dict[str, Tuple[list, list]] = {s: ([], []) for s in SPLITS}
    for cls, p in enumerate(npz_paths):
        d = load_quickdraw_npz(p, allow_pickle=allow_pickle, label=cls)
        for name, (strokes, labels) in d.items():
            merged[name][0].extend(strokes)
            merged[name][1].extend(labels.tolist())
    save_pack(out_path, merged)


def load_ndjson(path: str, recognized_only: bool = True, limit: int | None = None):
    """Read a QuickDraw ``.ndjson`` file, raw or simplified: one JSON object per
    line whose ``drawing`` is a list of strokes ``[[x...], [y...]]`` or
    ``[[x...], [y...], [t...]]`` (the times are ignored). Returns ``(drawings,
    words)``: each drawing a list of ``[n, 2]`` float64 polylines. Lines with
    ``recognized: false`` are skipped when ``recognized_only``; strokes without
    points are dropped, and so is a drawing without strokes."""
    import json
    drawings, words = [], []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            if limit is not None and len(drawings) >= limit:
                break
            line = line.strip()
            if not line:
                continue
            rec = json.loads(line)
            if recognized_only and not rec.get("recognized", True):
                continue
            lines = []
            for st in rec["drawing"]:
                if len(st) < 2 or len(st[0]) != len(st[1]):
                    raise ValueError("%s: a stroke needs x and y lists of one length" % path)
                if len(st[0]):
                    lines.append(np.stack([np.asarray(st[0], np.float64), np.asarray(st[1], np.float64)], axis=1))
            if lines:
                drawings.append(lines)
                words.append(rec.get("word", ""))
    return drawings, words


def normalize_drawing(lines) -> np.ndarray:
    """Absolute polylines -> integer-valued stroke-3 on the 0..255 canvas of
    the QuickDraw datasets: the box's top-left goes to (0, 0), a uniform scale
    makes the longer side 255 (scale 1 for a point-sized drawing), the
    positions are rounded to integers, a point equal to its predecessor within
    a stroke is dropped (a stroke keeps at least one point), and the result is
    delta-encoded (``data.strokes.lines_to_strokes``)."""
    from .strokes import lines_to_strokes
    lines = [np.asarray(l, np.float64).reshape(-1, 2) for l in lines]
    lines = [l for l in lines if len(l)]
    if not lines:
        return np.zeros((0, 3), np.float32)
    pts = np.concatenate(lines, axis=0)
    lo = pts.min(axis=0)
    side = float((pts.max(axis=0) - lo).max())
    scale = 255.0 / side if side > 0 else 1.0
    out = []
    for l in lines:
        q = np.round((l - lo) * scale)
        keep = np.ones(len(q), bool)
        keep[1:] = (q[1:] != q[:-1]).any(axis=1)
        out.append(q[keep])
    return lines_to_strokes(out).astype(np.float32)


def simplify_corpus(strokes: Sequence[np.ndarray], epsilon: float = 2.0, max_len: int | None = None,
                    batch: int = 1024, device=None):
    """RDP-simplify a list of stroke-3 sketches through ``ops.simplify``:
    sorted by length, padded into batches of ``batch``, one ``.cpu()`` per
    batch. ``max_len`` raises epsilon per sketch until it fits. Sketches longer
    than ``ops.simplify.MAX_N`` go through the host reference. ``device=None``
    is the GPU when there is one. Returns ``(strokes, eps_used, dropped)`` in
    the input's order: ``dropped`` lists the sketches whose new length still
    exceeds ``max_len`` (their run ends alone do)."""
    import torch
    from ..ops import simplify as S
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    device = torch.device(device)
    n = len(strokes)
    out: List[np.ndarray] = [None] * n
    eps_used = np.zeros(n, np.float64)
    order = sorted(range(n), key=lambda i: len(strokes[i]))
    i0 = 0
    while i0 < n:
        idx = order[i0:i0 + batch]
        # a batch does not straddle MAX_N: the longer sketches take the host path
        if len(strokes[idx[0]]) <= S.MAX_N < len(strokes[idx[-1]]):
            idx = [i for i in idx if len(strokes[i]) <= S.MAX_N]
        i0 += len(idx)
        N = max(len(strokes[idx[-1]]), 1)
        x = np.zeros((len(idx), N, 3), np.float32)
        for j, i in enumerate(idx):
            x[j, :len(strokes[i])] = strokes[i]
        L = torch.as_tensor([len(strokes[i]) for i in idx], dtype=torch.int64)
        dev = device if N <= S.MAX_N else torch.device("cpu")
        o, nl, eu = S.simplify(torch.from_numpy(x).to(dev), L.to(dev), epsilon, max_len)
        # the three results as bytes in one tensor: one transfer, one synchronisation
        raw = torch.cat([t.contiguous().view(torch.uint8).reshape(len(idx), -1) for t in (o, nl, eu)], dim=1)
        raw = raw.cpu().numpy()
        o = np.ascontiguousarray(raw[:, :N * 12]).view(np.float32).reshape(len(idx), N, 3)
        nl = np.ascontiguousarray(raw[:, N * 12:N * 12 + 8]).view(np.int64).reshape(-1)
        eu = np.ascontiguousarray(raw[:, N * 12 + 8:]).view(np.float64).reshape(-1)
        for j, i in enumerate(idx):
            out[i] = o[j, :nl[j]].copy()
            eps_used[i] = eu[j]
    dropped = [i for i in range(n) if max_len is not None and len(out[i]) > max_len]
    return out, eps_used, dropped
