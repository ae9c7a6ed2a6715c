"""The reference-pinned model fixtures with a WIDE classifier head (171 classes, COCO-Stuff): the case dictionaries, in the form
oracle.make_golden.run_model_case takes, shared by the generator (tools/make_golden_wide.py) and the tests
(tests/test_gpu_cls1x1_wide.py), and the loader of the stored arrays.
Both cases lie inside the conditioning cap of tests/test_models_golden.py::_check (the reference's own fp32 forward within 2.5e-4
of its fp64 evaluation): 4.4e-5 and 1.3e-4 when generated. (The OCR model at B=2, 64x96 does not: 3.3e-4 / 3.5e-4 for seeds 42 / 43.)
A fixture is stored as model_<name>.part<i>.npz files of at most PART_BYTES of array data each (171-class logits of three images
and the auxiliary head's do not fit one file under the repository's size limit): large arrays are cut along the batch axis into
`key@<image>` entries, and load() puts them together again."""
import glob
import os

import numpy as np

WIDE_MODEL_CASES = {
    "hrnet_w48_contrast_k171": dict(model="hrnet_w48_contrast", backbone="hrnet48", K=171, B=2, H=64, W=128, seed=45, contrast={}),
    "hrnet_w48_ocr_contrast_k171": dict(model="hrnet_w48_ocr_contrast", backbone="hrnet48", K=171, B=3, H=64, W=128, seed=44,
                                        contrast={}),
}
# how many times kernels.Cls1x1Wide runs in one forward: the classifier; the OCR model's auxiliary head and classifier
WIDE_CALLS = {"hrnet_w48_contrast_k171": 1, "hrnet_w48_ocr_contrast_k171": 2}
PART_BYTES = 720 * 1024


def split(arrays):
    """dict of arrays -> list of dicts, each at most PART_BYTES of array data (arrays above a quarter of that are cut per image)."""
    items = []
    for key, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes > PART_BYTES // 4 and a.ndim >= 1 and a.shape[0] > 1:
            items += [("%s@%d" % (key, i), a[i:i + 1]) for i in range(a.shape[0])]
        else:
            items.append((key, a))
    parts, size = [{}], 0
    for key, a in items:
        if parts[-1] and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += a.nbytes
    return parts


class Golden(dict):
    """What _check of tests/test_models_golden.py reads of an NpzFile: `files` and item access."""

    @property
    def files(self):
        return list(self.keys())


def load(golden_dir, name):
    paths = sorted(glob.glob(os.path.join(golden_dir, "model_%s.part*.npz" % name)))
    assert paths, "no fixture parts for %s under %s (tools/make_golden_wide.py writes them)" % (name, golden_dir)
    pieces, out = {}, Golden()
    for path in paths:
        with np.load(path) as z:
            for key in z.files:
                if "@" in key:
                    base, i = key.split("@")
                    pieces.setdefault(base, {})[int(i)] = z[key]
                else:
                    out[key] = z[key]
    for base, d in pieces.items():
        assert sorted(d) == list(range(len(d))), (base, sorted(d))
        out[base] = np.concatenate([d[i] for i in range(len(d))], axis=0)
    return out
