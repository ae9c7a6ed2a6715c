"""tests/test_gpu_lovasz.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies
run the HIP sources of csrc/lovasz.hip through the C-ABI and kernels.lovasz_errors / lovasz_order / lovasz_grad / lovasz_softmax -- the
three stages, loss and gradient against the reference, ties and saturation, determinism, the class chunks, void images, the refusals, the
memory criteria with contrast.use_lovasz -- in ascending wave order and once more in descending order (the tile scans, the ranks and the
float64 partial sums must not depend on it). The allocator and host-synchronisation checks run their kernels here and assert on the GPU."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_lovasz"
ORDERS = ["asc", "desc"]

ERRORS = _cases(MOD, "test_errors_match_float64_and_the_counts_are_exact")
ORDER = _cases(MOD, "test_order_is_the_stable_descending_sort")
GRAD = _cases(MOD, "test_grad_matches_the_float64_jaccard_differences")
LOSS = _cases(MOD, "test_loss_and_gradient_match_the_reference")
TIES = _cases(MOD, "test_ties_and_saturation_against_float64_in_the_kernels_order")
CRIT = _cases(MOD, "test_memory_criteria_with_use_lovasz")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", ERRORS, ids=_ids(ERRORS))
def test_errors_match_float64_and_the_counts_are_exact(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_errors_match_float64_and_the_counts_are_exact", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_bad_labels_are_dropped_and_counted(order, monkeypatch):
    _run(monkeypatch, order, "test_bad_labels_are_dropped_and_counted", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", ORDER, ids=_ids(ORDER))
def test_order_is_the_stable_descending_sort(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_order_is_the_stable_descending_sort", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_order_of_equal_keys_is_the_pixel_order(order, monkeypatch):
    _run(monkeypatch, order, "test_order_of_equal_keys_is_the_pixel_order", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", GRAD, ids=_ids(GRAD))
def test_grad_matches_the_float64_jaccard_differences(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_grad_matches_the_float64_jaccard_differences", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", LOSS, ids=_ids(LOSS))
def test_loss_and_gradient_match_the_reference(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_loss_and_gradient_match_the_reference", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", TIES, ids=_ids(TIES))
def test_ties_and_saturation_against_float64_in_the_kernels_order(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_ties_and_saturation_against_float64_in_the_kernels_order", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_class_chunks_give_the_same_bits(order, monkeypatch):
    _run(monkeypatch, order, "test_class_chunks_give_the_same_bits", {})


@pytest.mark.parametrize("order", ORDERS)
def test_void_images(order, monkeypatch):
    _run(monkeypatch, order, "test_void_images", {})


def test_routes_of_the_allocator_and_synchronisation_checks(monkeypatch):
    _run(monkeypatch, "asc", "test_no_gradient_buffer_without_a_gradient_to_compute", {})
    _run(monkeypatch, "asc", "test_no_host_synchronisation", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


@pytest.mark.parametrize("kw", CRIT, ids=_ids(CRIT))
def test_memory_criteria_with_use_lovasz(kw, monkeypatch):
    _run(monkeypatch, "asc", "test_memory_criteria_with_use_lovasz", kw)


def test_without_use_lovasz_the_criteria_are_unchanged(monkeypatch):
    _run(monkeypatch, "asc", "test_without_use_lovasz_the_criteria_are_unchanged", {})
