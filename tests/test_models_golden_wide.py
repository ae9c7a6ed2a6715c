"""CPU leg of the reference-pinned fixtures with a 171-class head (tests/golden_wide_cases.py, tests/golden/model_*_k171.part*.npz):
this repo's model classes on the CPU with the torch restatement (oracle/cpu_port.py) against the reference's logits, at the bound of
tests/test_models_golden.py's CPU leg. Checks the wiring of the wide head and pins the fixtures; the GPU leg, through the kernels of
csrc/cls1x1_wide.hip, is tests/test_gpu_cls1x1_wide.py::test_wide_model_forward_gpu_matches_reference."""
import pytest

from oracle import cpu_port
from tests.golden_wide_cases import WIDE_MODEL_CASES, load
from tests.test_models_golden import _build, _check, _forward


@pytest.mark.parametrize("name", list(WIDE_MODEL_CASES))
def test_wide_model_forward_cpu_matches_reference(name, golden_dir, monkeypatch):
    cpu_port.install(monkeypatch)
    c = WIDE_MODEL_CASES[name]
    out = _forward(_build(name, c), c, "cpu")
    _check(out, load(golden_dir, name), 5e-4)
