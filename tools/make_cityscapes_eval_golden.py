"""Writes tests/golden/cityscapes_eval/: a few tiny synthetic Cityscapes triples (labelIds, instanceIds, prediction PNGs) and what the
REFERENCE's pixel-level evaluator (lib/metrics/cityscapes_evaluator.py, EvalPixel.evaluateImgLists, its Python path: CSUPPORT off)
makes of them -- the returned dictionary, its raw instStats, the pixel accuracy it prints, and the same for every image alone (the
per-image partials a multi-rank test splits). Runs only where the reference tree exists (oracle/ref_shim.py says where); the goldens
are committed, so the tests do not need it.

The reference is imported, not copied: `PIL.PILLOW_VERSION`, which its helper insists on and Pillow dropped, is set before the import,
and no bytecode is written into its tree. File lists are passed explicitly and sorted: the reference's own order is glob order and its
float sums depend on it.

    python tools/make_cityscapes_eval_golden.py
"""
import contextlib
import io
import json
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "cityscapes_eval")
H, W = 32, 64
STEMS = ["aachen_000000_000019", "bochum_000000_000313", "cologne_000002_000019"]
STUFF = [0, 1, 3, 4, 7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 9, 14]          # void and ignored labels among them
TRAIN_IDS = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


def _rects(rs, n, hmax, wmax):
    for _ in range(n):
        h, w = rs.randint(2, hmax + 1), rs.randint(2, wmax + 1)
        y, x = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        yield slice(y, y + h), slice(x, x + w)


def make_triple(k):
    """-> labelIds u8, instanceIds u16, prediction u8 (label ids) of image k."""
    rs = np.random.RandomState(304 + k)
    lab = np.full((H, W), 7, np.uint8)
    for ys, xs in _rects(rs, 14, 12, 24):
        lab[ys, xs] = STUFF[rs.randint(len(STUFF))]
    inst = lab.astype(np.uint16)
    # instances: (label, number); 24000 and 33999 are the ends of the number range, 26003 occurs in every image, 29 / 30 are ignored in
    # the evaluation, a crowd region keeps the bare label id
    things = [(24, 0), (33, 999), (26, 3), (25, 17), (27, 1), (28, 2), (29, 4), (30, 5), (31, 6), (32, 7), (24, 1 + k), (26, 40 + k)]
    for (l, n), (ys, xs) in zip(things, _rects(rs, len(things), 9, 14)):
        lab[ys, xs] = l
        inst[ys, xs] = l * 1000 + n
    ys, xs = next(_rects(rs, 1, 6, 10))
    lab[ys, xs] = 26                                       # a group of cars: no instance id
    inst[ys, xs] = 26
    pred = np.where(np.isin(lab, TRAIN_IDS), lab, 7).astype(np.uint8)
    for ys, xs in _rects(rs, 16, 8, 16):                  # errors in blocks
        pred[ys, xs] = TRAIN_IDS[rs.randint(len(TRAIN_IDS))]
    first = inst == 27001                                  # one instance without a single true positive
    pred[first & (pred == 27)] = 26
    return lab, inst, pred


def _import_reference():
    import PIL
    from oracle.ref_shim import REFERENCE_ROOT
    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "lib", "metrics")):
        raise SystemExit("the reference tree is not present at %s" % REFERENCE_ROOT)
    if not hasattr(PIL, "PILLOW_VERSION"):
        PIL.PILLOW_VERSION = PIL.__version__
    sys.path.insert(0, REFERENCE_ROOT)
    import lib.metrics.cityscapes_evaluator as E
    assert not E.CSUPPORT
    return E


def _plain(obj):
    if isinstance(obj, dict):
        return {str(k): _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    if isinstance(obj, (np.floating, float)):
        return float(obj)
    if isinstance(obj, (np.integer, int)):
        return int(obj)
    return obj


def evaluate(E, preds, gts):
    """-> {result, instStats, pixelAccuracy, order of the result's dictionaries} of one evaluateImgLists call."""
    args = E.CArgs(data_path=OUT, out_path=OUT, predict_path=OUT)
    args.quiet = True
    seen = []
    make = E.generateInstanceStats
    E.generateInstanceStats = lambda a: seen.append(make(a)) or seen[-1]
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            result = E.EvalPixel(args, preds, gts).evaluateImgLists(preds, gts, args)
    finally:
        E.generateInstanceStats = make
    lines = buf.getvalue().splitlines()
    acc = float(lines[lines.index("pixel accuracy") + 1])
    result.pop("perImageScores", None)
    order = {k: list(result[k]) for k in ("labels", "priors", "classScores", "classInstScores", "categoryScores", "categoryInstScores")}
    return {"result": _plain(result), "instStats": _plain(seen[0]), "pixelAccuracy": acc, "order": order}


def main():
    os.makedirs(OUT, exist_ok=True)
    gts, preds = [], []
    for k, stem in enumerate(STEMS):
        lab, inst, pred = make_triple(k)
        Image.fromarray(lab).save(os.path.join(OUT, stem + "_gtFine_labelIds.png"))
        Image.fromarray(inst).save(os.path.join(OUT, stem + "_gtFine_instanceIds.png"))
        Image.fromarray(pred).save(os.path.join(OUT, stem + "_pred.png"))
        gts.append(os.path.join(OUT, stem + "_gtFine_labelIds.png"))
        preds.append(os.path.join(OUT, stem + "_pred.png"))
    E = _import_reference()
    golden = {"stems": STEMS, "all": evaluate(E, preds, gts), "per_image": [evaluate(E, [p], [g]) for p, g in zip(preds, gts)]}
    with open(os.path.join(OUT, "golden.json"), "w") as f:
        json.dump(golden, f, indent=1)
    print("wrote %s: %d images, average IoU %.6f, average iIoU %.6f" % (OUT, len(STEMS), golden["all"]["result"]["averageScoreClasses"],
                                                                       golden["all"]["result"]["averageScoreInstClasses"]))


if __name__ == "__main__":
    main()
