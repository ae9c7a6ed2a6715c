"""tests/test_gpu_cityscapes_eval.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the HIP sources of csrc/cityscapes_eval.hip through the C-ABI, kernels.cs_eval_update / kernels.cs_eval_reduce and
CityscapesScore -- the reference's goldens bit for bit, the numpy restatement on every seeded case, the per-image table, two batches
against their concatenation, determinism, the refusals -- in ascending wave order and once more in descending order: neither the
segmented scan and the LDS bins of the update kernel nor the compaction of the reduction may depend on it. Not replayed: the Tester leg
(a whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_cityscapes_eval"
ORDERS = ["asc", "desc"]

RESTATE = _cases(MOD, "test_update_and_reduce_equal_the_restatement")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
def test_golden_triples_give_the_references_numbers(order, monkeypatch):
    _run(monkeypatch, order, "test_golden_triples_give_the_references_numbers", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", RESTATE, ids=_ids(RESTATE))
def test_update_and_reduce_equal_the_restatement(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_update_and_reduce_equal_the_restatement", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_the_table_keeps_two_images_apart_and_skips_what_the_reference_skips(order, monkeypatch):
    _run(monkeypatch, order, "test_the_table_keeps_two_images_apart_and_skips_what_the_reference_skips", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_batches_equal_one_call_on_their_concatenation(order, monkeypatch):
    _run(monkeypatch, order, "test_two_batches_equal_one_call_on_their_concatenation", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})
