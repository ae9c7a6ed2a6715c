"""tests/test_gpu_crop_eval.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies
run the HIP source of csrc/crop_eval.hip through the C-ABI and kernels.crop_fuse_argmax -- the fused map and the prediction against the
float64 composition on every case, the one-tile case against cseg_ms_fuse_argmax, the mirrored tiling, the tie rule, determinism, the
refusals of the wrapper and of the library -- in ascending wave order and once more in descending order (the tap tables in LDS are
written by the first two waves and read by all four: the result must not depend on the order). Not replayed: the memory assertion's
allocator half (no allocator to ask), the Tester legs (a whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_crop_eval"
ORDERS = ["asc", "desc"]

FUSED = _cases(MOD, "test_fused_map_matches_the_float64_composition")
PRED = _cases(MOD, "test_prediction_matches_the_float64_argmax")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", FUSED, ids=_ids(FUSED))
def test_fused_map_matches_the_float64_composition(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_fused_map_matches_the_float64_composition", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", PRED, ids=_ids(PRED))
def test_prediction_matches_the_float64_argmax(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_prediction_matches_the_float64_argmax", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_the_flipped_pass_tiles_the_mirrored_canvas(order, monkeypatch):
    _run(monkeypatch, order, "test_the_flipped_pass_tiles_the_mirrored_canvas", {})


@pytest.mark.parametrize("order", ORDERS)
def test_first_index_wins_among_equal_maxima(order, monkeypatch):
    _run(monkeypatch, order, "test_first_index_wins_among_equal_maxima", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


@pytest.mark.parametrize("order", ORDERS)
def test_the_library_refuses_what_the_wrapper_refuses(order, monkeypatch):
    _run(monkeypatch, order, "test_the_library_refuses_what_the_wrapper_refuses", {})


def test_nothing_of_the_size_of_a_canvas_is_allocated(monkeypatch):
    _run(monkeypatch, "asc", "test_nothing_of_the_size_of_a_canvas_is_allocated", {})
