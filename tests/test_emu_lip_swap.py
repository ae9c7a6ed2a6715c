"""tests/test_gpu_lip_swap.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies
run the HIP sources of csrc/ms_eval.hip, csrc/ms_eval_ragged.hip, csrc/augment.hip and csrc/augment_ragged.hip through the C-ABI and
the wrappers of kernels.py -- the permuted scoring call against gathering first and against float64, dense and ragged, the label swap
of both augmentation kernels against numpy and the oracle's primitives, the refusals, determinism -- in ascending wave order and once
more in descending order. Not replayed: the scoring helper of the validation pass (the Trainer's module)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_lip_swap"
ORDERS = ["asc", "desc"]

DENSE = _cases(MOD, "test_dense_permutation_equals_gathering_first")
RAGGED = _cases(MOD, "test_ragged_permutation_equals_gathering_first_and_the_dense_call")
F64_DENSE = _cases(MOD, "test_dense_permuted_call_matches_the_float64_composition")
F64_RAGGED = _cases(MOD, "test_ragged_permuted_call_matches_the_float64_composition")
FLIP = _cases(MOD, "test_flip_alone_swaps_the_pairs_as_the_reference_loop_does")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", DENSE, ids=_ids(DENSE))
def test_dense_permutation_equals_gathering_first(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_dense_permutation_equals_gathering_first", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_dense_three_cycle_shows_the_direction(order, monkeypatch):
    _run(monkeypatch, order, "test_dense_three_cycle_shows_the_direction", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", RAGGED, ids=_ids(RAGGED))
def test_ragged_permutation_equals_gathering_first_and_the_dense_call(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_ragged_permutation_equals_gathering_first_and_the_dense_call", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_ragged_three_cycle(order, monkeypatch):
    _run(monkeypatch, order, "test_ragged_three_cycle", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", F64_DENSE, ids=_ids(F64_DENSE))
def test_dense_permuted_call_matches_the_float64_composition(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_dense_permuted_call_matches_the_float64_composition", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", F64_RAGGED, ids=_ids(F64_RAGGED))
def test_ragged_permuted_call_matches_the_float64_composition(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_ragged_permuted_call_matches_the_float64_composition", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", FLIP, ids=_ids(FLIP))
def test_flip_alone_swaps_the_pairs_as_the_reference_loop_does(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_flip_alone_swaps_the_pairs_as_the_reference_loop_does", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_lip_order_on_a_ragged_batch(order, monkeypatch):
    _run(monkeypatch, order, "test_lip_order_on_a_ragged_batch", {})


@pytest.mark.parametrize("order", ORDERS)
def test_canonical_order_on_a_uniform_batch(order, monkeypatch):
    _run(monkeypatch, order, "test_canonical_order_on_a_uniform_batch", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})
