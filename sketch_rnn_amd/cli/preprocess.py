"""``python -m sketch_rnn_amd.cli.preprocess`` -- dataset preparation.

* ``svg DIR OUT.npz``: SVG corpus -> reference stroke-4 cache (R4; the
  reference's ``data/<name>.cpkl`` step, ``utils.py:124-217``, without pickle);
* ``quickdraw OUT.skpack.npz A.npz [B.npz ...] --allow-pickle``: public
  QuickDraw files (object arrays; only for files you trust) -> sketch pack,
  one class label per input file;
* ``synthetic OUT.skpack.npz --n N``: synthetic corpus in pack format;
* ``ndjson OUT.skpack.npz A.ndjson [B.ndjson ...]``: QuickDraw ``.ndjson`` files,
  raw or simplified -> sketch pack, one class label per input file. Every
  drawing is put on the 0..255 canvas and RDP-simplified at ``--epsilon``
  (``ops.simplify``); what is still longer than ``--max_len`` is dropped, or
  with ``--fit`` simplified further until it fits;
* ``simplify IN.skpack.npz OUT.skpack.npz``: the same on an existing pack,
  every split, labels carried.
"""
from __future__ import annotations

import argparse
import sys


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("svg")
    s.add_argument("data_dir")
    s.add_argument("out")
    s.add_argument("--verbose", action="store_true")
    q = sub.add_parser("quickdraw")
    q.add_argument("out")
    q.add_argument("inputs", nargs="+")
    q.add_argument("--allow-pickle", action="store_true")
    y = sub.add_parser("synthetic")
    y.add_argument("out")
    y.add_argument("--n", type=int, default=10000)
    y.add_argument("--classes", type=int, default=1)
    y.add_argument("--max_len", type=int, default=250)
    y.add_argument("--seed", type=int, default=0)
    n = sub.add_parser("ndjson")
    n.add_argument("out")
    n.add_argument("inputs", nargs="+")
    n.add_argument("--all", action="store_true", help="keep unrecognised drawings")
    n.add_argument("--limit", type=int, default=None, help="drawings read per file")
    n.add_argument("--valid", type=int, default=2500)
    n.add_argument("--test", type=int, default=2500)
    m = sub.add_parser("simplify")
    m.add_argument("inp")
    m.add_argument("out")
    for q in (n, m):
        q.add_argument("--epsilon", type=float, default=2.0)
        q.add_argument("--max_len", type=int, default=250 if q is n else None)
        q.add_argument("--fit", action="store_true", help="raise epsilon per sketch until it fits --max_len")
    a = p.parse_args(argv)
    if a.cmd == "svg":
        from ..data.preprocess import preprocess
        sk, _ = preprocess(a.data_dir, a.out, verbose=a.verbose)
        print("wrote %d sketches to %s" % (len(sk), a.out))
    elif a.cmd == "quickdraw":
        from ..data.quickdraw import convert_to_pack
        convert_to_pack(a.inputs, a.out, allow_pickle=a.allow_pickle)
        print("wrote %s" % a.out)
    elif a.cmd in ("ndjson", "simplify"):
        _simplify_cmd(a)
    else:
        from ..data.quickdraw import save_pack
        from ..data.synthetic import synthetic_corpus
        s, l = synthetic_corpus(a.n, seed=a.seed, max_len=a.max_len, n_classes=a.classes)
        k = max(a.n // 10, 1)
        save_pack(a.out, {"train": (s[2 * k:], l[2 * k:]), "valid": (s[:k], l[:k]), "test": (s[k:2 * k], l[k:2 * k])})
        print("wrote %s" % a.out)
    return 0


def _simplify_cmd(a) -> None:
    import numpy as np
    from ..data.quickdraw import SPLITS, load_ndjson, load_pack, normalize_drawing, save_pack, simplify_corpus

    def run(strokes, labels):
        """Simplified ``(strokes, labels)`` without the sketches that stay too long, and their count."""
        out, _, dropped = simplify_corpus(strokes, epsilon=a.epsilon, max_len=a.max_len if a.fit else None)
        if a.max_len is not None and not a.fit:
            dropped = [i for i, s in enumerate(out) if len(s) > a.max_len]
        gone = set(dropped)
        keep = [i for i in range(len(out)) if i not in gone]
        return [out[i] for i in keep], [int(labels[i]) for i in keep], len(out) - len(keep)

    merged = {s: ([], []) for s in SPLITS}
    total = dropped = 0
    if a.cmd == "ndjson":
        for cls, path in enumerate(a.inputs):
            drawings, _ = load_ndjson(path, recognized_only=not a.all, limit=a.limit)
            sk, lab, gone = run([normalize_drawing(d) for d in drawings], [cls] * len(drawings))
            total, dropped = total + len(drawings), dropped + gone
            # the last valid + test sketches of each file are held out
            k = len(sk)
            nt = min(a.test, k)
            nv = min(a.valid, k - nt)
            for name, lo, hi in (("train", 0, k - nv - nt), ("valid", k - nv - nt, k - nt), ("test", k - nt, k)):
                merged[name][0].extend(sk[lo:hi])
                merged[name][1].extend(lab[lo:hi])
    else:
        pack = load_pack(a.inp)
        merged = {}
        for name, (strokes, labels) in pack.items():
            sk, lab, gone = run(strokes, np.asarray(labels).tolist())
            total, dropped = total + len(strokes), dropped + gone
            merged[name] = (sk, lab)
    save_pack(a.out, merged)
    kept = sum(len(v[0]) for v in merged.values())
    print("read %d sketches, kept %d, dropped %d longer than max_len=%s at epsilon=%g%s; wrote %s" % (
        total, kept, dropped, a.max_len, a.epsilon, " (fitted)" if a.fit else "", a.out))


if __name__ == "__main__":
    sys.exit(main())
