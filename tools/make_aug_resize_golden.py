"""Writes tests/golden/aug_decisions_resize.json: the decisions the REFERENCE'S OWN transform classes
(lib/datasets/tools/cv2_aug_transforms.py, cv2 stubbed -- it is not installed) take on images of mixed sizes under one seed, for
sequences that hold the `resize` transform: the COCO-Stuff order with min_side_length, and one run each with target_size,
max_side_length and max_side_bound. Per sample and transform: [name, skipped, arguments, output shape, first output value] -- the
recipe of oracle/make_golden.py --only aug_decisions. Needs the reference checkout (oracle/ref_shim.py); tests read the fixture only
(tests/test_aug_ragged_host.py).

    python tools/make_aug_resize_golden.py"""
import collections
import collections.abc
import importlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "aug_decisions_resize.json")
SEED = 4321
SIZES = [(160, 96), (90, 120), (123, 81), (64, 64), (200, 75), (61, 83), (333, 217), (128, 64), (64, 128), (97, 101)] * 3


def trans(resize):
    return {"trans_seq": ["random_hflip", "resize", "random_resize", "random_crop", "random_brightness"],
            "random_brightness": {"ratio": 0.7, "shift_value": 10},
            "resize": resize,
            "random_hflip": {"ratio": 0.5, "swap_pair": []},
            "random_resize": {"ratio": 0.8, "method": "random", "scale_range": [0.5, 2.0], "aspect_range": [0.9, 1.1]},
            "random_crop": {"ratio": 1.0, "crop_size": [96, 64], "method": "random", "allow_outside_center": False}}


RUNS = [("coco_min_side_length", trans({"min_side_length": 64})),
        ("target_size", trans({"target_size": [80, 56]})),
        ("max_side_length", trans({"max_side_length": 100})),
        ("max_side_bound", trans({"min_side_length": 64, "max_side_bound": 120}))]


def config_dict(train_trans):
    return {"data": {"num_classes": 19, "input_mode": "BGR", "image_tool": "cv2"},
            "train": {"data_transformer": {"size_mode": "fix_size", "input_size": [96, 64], "align_method": "only_pad",
                                           "pad_mode": "random"}},
            "train_trans": train_trans, "val_trans": {"trans_seq": []},
            "normalize": {"div_value": 255.0, "mean_value": [0.485, 0.456, 0.406], "mean": [0.485, 0.456, 0.406],
                          "std": [0.229, 0.224, 0.225]}}


def plain(v):
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    if isinstance(v, (np.integer, np.bool_)):
        return v.item()
    return v


def main():
    from oracle import ref_shim
    if not ref_shim.available():
        raise SystemExit("the reference checkout is not available: the fixture cannot be regenerated here")
    ref_shim.install()
    cv2 = sys.modules["cv2"]
    cv2.INTER_CUBIC, cv2.INTER_NEAREST = 2, 0
    cv2.resize = lambda x, size, interpolation=None: np.full((size[1], size[0]) + x.shape[2:], 128, dtype=x.dtype)
    cv2.flip = lambda x, code: x
    if not hasattr(collections, "Iterable"):
        collections.Iterable = collections.abc.Iterable      # the reference predates Python 3.10
    aug = importlib.import_module("lib.datasets.tools.cv2_aug_transforms")
    from lib.utils.tools.configer import Configer as RefConfiger
    log = []
    orig = aug._BaseTransform._process

    def spy(self, img, data_dict, skip, *args, **kw):
        out_img, out = orig(self, img, data_dict, skip, *args, **kw)
        log[-1].append([type(self).__name__, bool(skip), plain(list(args)), list(out_img.shape), int(out_img.reshape(-1)[0])])
        return out_img, out
    aug._BaseTransform._process = spy
    runs = []
    try:
        for name, train_trans in RUNS:
            compose = aug.CV2AugCompose(RefConfiger(config_dict=config_dict(train_trans)), split="train")
            random.seed(SEED)
            del log[:]
            for (w, h) in SIZES:
                log.append([])
                compose(np.full((h, w, 3), 128, np.uint8), labelmap=np.zeros((h, w), np.float32))
            runs.append((name, train_trans, [list(s) for s in log]))
    finally:
        aug._BaseTransform._process = orig
    with open(OUT, "w") as f:
        f.write('{"seed": %d, "sizes": %s, "runs": [\n' % (SEED, json.dumps([list(s) for s in SIZES])))
        for k, (name, train_trans, entries) in enumerate(runs):
            f.write('{"name": %s, "train_trans": %s, "log": [\n' % (json.dumps(name), json.dumps(train_trans)))
            f.write(",\n".join(json.dumps(sample) for sample in entries))          # one sample per line
            f.write("\n]}%s\n" % ("," if k + 1 < len(runs) else ""))
        f.write("]}\n")
    print("aug_decisions_resize: %d runs of %d samples -> %s" % (len(runs), len(SIZES), OUT))


if __name__ == "__main__":
    main()
