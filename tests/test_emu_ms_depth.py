"""tests/test_gpu_ms_depth.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies
run the HIP sources of csrc/ms_eval.hip and csrc/cseg_ms_fuse.h through the C-ABI and kernels.lut_u16_u8 /
kernels.ms_fuse_argmax(pixel_weights=...) -- the fused map and the prediction against the float64 composition with per-pixel weight
maps on every case, bit equality with the call without pixel weights (a table constant per term, a one-bin table of ones, one scale
without flip), the tie rule, determinism, either output alone, the look-up kernel against numpy, the refusals of wrapper and library --
in ascending wave order and once more in descending order. Not replayed: the memory assertion (no allocator to ask), the Tester legs
(a whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_ms_depth"
ORDERS = ["asc", "desc"]

F64 = _cases(MOD, "test_fused_map_and_prediction_match_the_float64_composition")
CONST = _cases(MOD, "test_a_table_constant_per_term_equals_scalar_weights")
ONES = _cases(MOD, "test_a_one_bin_table_of_ones_equals_the_unweighted_call")
LUT = _cases(MOD, "test_lut_u16_u8_equals_numpy_indexing")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", F64, ids=_ids(F64))
def test_fused_map_and_prediction_match_the_float64_composition(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_fused_map_and_prediction_match_the_float64_composition", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", CONST, ids=_ids(CONST))
def test_a_table_constant_per_term_equals_scalar_weights(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_a_table_constant_per_term_equals_scalar_weights", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", ONES, ids=_ids(ONES))
def test_a_one_bin_table_of_ones_equals_the_unweighted_call(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_a_one_bin_table_of_ones_equals_the_unweighted_call", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_one_scale_without_flip_equals_ss_test(order, monkeypatch):
    _run(monkeypatch, order, "test_one_scale_without_flip_equals_ss_test", {})


@pytest.mark.parametrize("order", ORDERS)
def test_first_index_wins_among_equal_maxima(order, monkeypatch):
    _run(monkeypatch, order, "test_first_index_wins_among_equal_maxima", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_pred_alone_and_fused_alone(order, monkeypatch):
    _run(monkeypatch, order, "test_pred_alone_and_fused_alone", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", LUT, ids=_ids(LUT))
def test_lut_u16_u8_equals_numpy_indexing(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_lut_u16_u8_equals_numpy_indexing", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})
