"""tests/test_gpu_aug_ragged.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the HIP source of csrc/augment_ragged.hip through the C-ABI, kernels.resize_ragged / kernels.augment_ragged and
GPUBatchTransform -- stage 1 bit for bit, the full chains against the literal composition of the oracle's primitives, the uniform batch
against cseg_augment_batch, the refusals of the wrapper and of the library, determinism -- in ascending wave order and once more in
descending order (the kernels share nothing between waves: the result must not depend on the order). Not replayed: the refusal of CPU
tensors (the emulated device IS the CPU) and the Trainer leg (a whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_aug_ragged"
ORDERS = ["asc", "desc"]

UNIFORM = _cases(MOD, "test_uniform_batch_equals_augment_batch", lambda kw: kw["B"] * kw["Ht"] * kw["Wt"] <= 4 * 64 * 128)


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
def test_stage1_is_the_oracles_resize_bit_for_bit(order, monkeypatch):
    _run(monkeypatch, order, "test_stage1_is_the_oracles_resize_bit_for_bit", {})


@pytest.mark.parametrize("order", ORDERS)
def test_full_chain_in_the_coco_order(order, monkeypatch):
    _run(monkeypatch, order, "test_full_chain_in_the_coco_order", {})


@pytest.mark.parametrize("order", ORDERS)
def test_flip_between_resamplings_and_ahead_of_the_crop(order, monkeypatch):
    _run(monkeypatch, order, "test_flip_between_resamplings_and_ahead_of_the_crop", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", UNIFORM, ids=_ids(UNIFORM))
def test_uniform_batch_equals_augment_batch(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_uniform_batch_equals_augment_batch", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


@pytest.mark.parametrize("order", ORDERS)
def test_the_library_refuses_what_the_wrapper_refuses(order, monkeypatch):
    _run(monkeypatch, order, "test_the_library_refuses_what_the_wrapper_refuses", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_gpu_batch_transform_end_to_end_on_mixed_sizes(order, monkeypatch):
    _run(monkeypatch, order, "test_gpu_batch_transform_end_to_end_on_mixed_sizes", {})
