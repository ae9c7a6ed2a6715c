"""tests/test_gpu_device_sampling.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run csrc/sampling.hip (planner, mt19937, picks) and the device-N kernels of csrc/contrast.hip through the C-ABI,
kernels.sample_anchors / PixelContrastDevice and the criteria -- in ascending wave order and once more in descending order (the four
phases of a regeneration and the block prefix sums must not depend on it). Not replayed: the hipGraph capture (no graphs on the
emulated device) and the train step (a whole network)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_device_sampling"
ORDERS = ["asc", "desc"]

PLAN = _cases(MOD, "test_planner_and_generator_match_the_host_planner")
STATUS = _cases(MOD, "test_status_leaves_the_generator_untouched")
CRIT = _cases(MOD, "test_criterion_is_bit_identical_to_the_host_path")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", PLAN, ids=_ids(PLAN))
def test_planner_and_generator_match_the_host_planner(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_planner_and_generator_match_the_host_planner", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", STATUS, ids=_ids(STATUS))
def test_status_leaves_the_generator_untouched(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_status_leaves_the_generator_untouched", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_bad_labels_set_bit_one(order, monkeypatch):
    _run(monkeypatch, order, "test_bad_labels_set_bit_one", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", CRIT, ids=_ids(CRIT))
def test_criterion_is_bit_identical_to_the_host_path(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_criterion_is_bit_identical_to_the_host_path", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_a_step_with_status_gives_nan_and_zero_gradient(order, monkeypatch):
    _run(monkeypatch, order, "test_a_step_with_status_gives_nan_and_zero_gradient", {})
