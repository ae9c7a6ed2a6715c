"""Generates the reference-pinned model fixtures with a 171-class head (tests/golden/model_*_k171.part*.npz) by handing the case
dictionaries of tests/golden_wide_cases.py to oracle.make_golden.run_model_case -- the reference itself on the CPU in fp32, with its
own fp32-vs-fp64 noise recorded -- and cutting the result into parts below the repository's file-size limit. Needs the reference
checkout the oracle is set up for; about 20 s per case.
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_wide.py [--only NAME]"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden  # noqa: E402
from tests.golden_wide_cases import WIDE_MODEL_CASES, split  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for name, c in WIDE_MODEL_CASES.items():
        if args.only and args.only != name:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            make_golden.OUT = tmp                      # run_model_case writes model_<name>.npz into make_golden.OUT
            make_golden.run_model_case(name, c)
            with np.load(os.path.join(tmp, "model_%s.npz" % name)) as z:
                arrays = {k: z[k] for k in z.files}
        for i, part in enumerate(split(arrays)):
            path = os.path.join(GOLDEN, "model_%s.part%d.npz" % (name, i))
            np.savez_compressed(path, **part)
            print(path, sorted(part), os.path.getsize(path))


if __name__ == "__main__":
    main()
