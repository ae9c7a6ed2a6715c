"""tests/test_gpu_ms_eval_ragged.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the HIP sources of csrc/ms_eval_ragged.hip and csrc/ms_eval.hip through the C-ABI and kernels.ms_fuse_argmax_ragged -- every
image's fused map and prediction against the float64 composition at its padded size, bit equality with kernels.ms_fuse_argmax image by
image, a missing flipped map among present ones, the tie rule, determinism, either output alone, the refusals of wrapper and library --
in ascending wave order and once more in descending order. Not replayed: the memory assertion (no allocator to ask), the Tester legs
(a whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_ms_eval_ragged"
ORDERS = ["asc", "desc"]

F64 = _cases(MOD, "test_fused_map_and_prediction_match_the_float64_composition")
BITS = _cases(MOD, "test_every_image_is_bit_equal_to_ms_fuse_argmax_on_it_alone")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", F64, ids=_ids(F64))
def test_fused_map_and_prediction_match_the_float64_composition(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_fused_map_and_prediction_match_the_float64_composition", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", BITS, ids=_ids(BITS))
def test_every_image_is_bit_equal_to_ms_fuse_argmax_on_it_alone(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_every_image_is_bit_equal_to_ms_fuse_argmax_on_it_alone", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_pred_alone_and_fused_alone(order, monkeypatch):
    _run(monkeypatch, order, "test_pred_alone_and_fused_alone", {})


@pytest.mark.parametrize("order", ORDERS)
def test_one_image_without_flipped_maps_among_images_with_them(order, monkeypatch):
    _run(monkeypatch, order, "test_one_image_without_flipped_maps_among_images_with_them", {})


@pytest.mark.parametrize("order", ORDERS)
def test_first_index_wins_among_equal_maxima(order, monkeypatch):
    _run(monkeypatch, order, "test_first_index_wins_among_equal_maxima", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})
