"""tests/test_gpu_ohem.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies run the
HIP sources of csrc/ohem.hip through the C-ABI and kernels.ohem_prob / ohem_threshold / ohem_reduce / ohem_ce -- the three stages, the
kept set, loss and gradient against the reference, ties, the crafted keys, determinism, the empty selections, the refusals, the
registered criteria and the four contrast criteria with contrast.use_ohem -- in ascending wave order and once more in descending order
(the histograms, the ranks and the float64 partial sums must not depend on it). The host-synchronisation check runs its kernels here and
asserts on the GPU."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_ohem"
ORDERS = ["asc", "desc"]

PROB = _cases(MOD, "test_prob_matches_float64")
THRESHOLD = _cases(MOD, "test_threshold_is_the_order_statistic_of_the_stored_p")
REDUCE = _cases(MOD, "test_reduce_over_the_stored_p")
PARITY = _cases(MOD, "test_loss_gradient_and_kept_set_match_the_reference")
NOFIX = _cases(MOD, "test_cases_without_a_fixture_against_float64_with_the_kernels_kept_set")
WITH = _cases(MOD, "test_contrast_criteria_with_use_ohem")
WITHOUT = _cases(MOD, "test_without_use_ohem_the_criteria_are_unchanged")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", PROB, ids=_ids(PROB))
def test_prob_matches_float64(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_prob_matches_float64", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_bad_labels_are_dropped_and_counted(order, monkeypatch):
    _run(monkeypatch, order, "test_bad_labels_are_dropped_and_counted", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", THRESHOLD, ids=_ids(THRESHOLD))
def test_threshold_is_the_order_statistic_of_the_stored_p(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_threshold_is_the_order_statistic_of_the_stored_p", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_threshold_of_crafted_keys(order, monkeypatch):
    _run(monkeypatch, order, "test_threshold_of_crafted_keys", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", REDUCE, ids=_ids(REDUCE))
def test_reduce_over_the_stored_p(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_reduce_over_the_stored_p", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", PARITY, ids=_ids(PARITY))
def test_loss_gradient_and_kept_set_match_the_reference(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_loss_gradient_and_kept_set_match_the_reference", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", NOFIX, ids=_ids(NOFIX))
def test_cases_without_a_fixture_against_float64_with_the_kernels_kept_set(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_cases_without_a_fixture_against_float64_with_the_kernels_kept_set", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_void_images_and_empty_selections(order, monkeypatch):
    _run(monkeypatch, order, "test_void_images_and_empty_selections", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


def test_route_of_the_synchronisation_check(monkeypatch):
    _run(monkeypatch, "asc", "test_no_host_synchronisation", {})


@pytest.mark.parametrize("order", ORDERS)
def test_registered_criteria(order, monkeypatch):
    _run(monkeypatch, order, "test_registered_criteria", {})


@pytest.mark.parametrize("kw", WITH, ids=_ids(WITH))
def test_contrast_criteria_with_use_ohem(kw, monkeypatch):
    _run(monkeypatch, "asc", "test_contrast_criteria_with_use_ohem", kw)


@pytest.mark.parametrize("kw", WITHOUT, ids=_ids(WITHOUT))
def test_without_use_ohem_the_criteria_are_unchanged(kw, monkeypatch):
    _run(monkeypatch, "asc", "test_without_use_ohem_the_criteria_are_unchanged", kw)
