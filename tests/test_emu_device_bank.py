"""tests/test_gpu_device_bank.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the device enqueue of csrc/queue.hip (planner, generator, picks, both writers with the last-writer-wins rule), the bank-mode
device-N kernels of csrc/contrast.hip and the criteria through the C-ABI -- in ascending wave order and once more in descending order
(the block prefix sums and the at-most-one-writer rule must not depend on it). This is the check of contrast.device_bank that runs
without a GPU. Not replayed: the hipGraph capture (no graphs on the emulated device) and the train step (a whole network)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_device_bank"
ORDERS = ["asc", "desc"]

ENQ = _cases(MOD, "test_enqueue_matches_the_host_enqueue")
CRIT = _cases(MOD, "test_criterion_and_enqueue_are_bit_identical_to_the_host_path")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", ENQ, ids=_ids(ENQ))
def test_enqueue_matches_the_host_enqueue(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_enqueue_matches_the_host_enqueue", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", CRIT, ids=_ids(CRIT))
def test_criterion_and_enqueue_are_bit_identical_to_the_host_path(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_criterion_and_enqueue_are_bit_identical_to_the_host_path", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_the_bank_must_not_change_between_forward_and_backward(order, monkeypatch):
    _run(monkeypatch, order, "test_the_bank_must_not_change_between_forward_and_backward", {})


@pytest.mark.parametrize("order", ORDERS)
def test_a_step_with_status_gives_nan_zero_gradient_and_an_untouched_generator(order, monkeypatch):
    _run(monkeypatch, order, "test_a_step_with_status_gives_nan_zero_gradient_and_an_untouched_generator", {})
