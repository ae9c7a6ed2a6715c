"""tests/test_gpu_ms_eval.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies
run the HIP sources of csrc/ms_eval.hip through the C-ABI and kernels.ms_fuse_argmax / kernels.confusion_update -- the fused map and the
prediction against the float64 composition on every case, the tie rule, the confusion matrix on both of its paths, determinism, the
refusals -- in ascending wave order and once more in descending order (the segmented scan of the global confusion path and the LDS
histogram must not depend on it). Not replayed: the memory assertion (no allocator to ask), the Tester / Trainer legs (a whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_ms_eval"
ORDERS = ["asc", "desc"]

FUSED = _cases(MOD, "test_fused_map_matches_the_float64_composition")
PRED = _cases(MOD, "test_prediction_matches_the_float64_argmax")
CONF = _cases(MOD, "test_confusion_update_equals_bincount")


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
def test_first_index_wins_among_equal_maxima(order, monkeypatch):
    _run(monkeypatch, order, "test_first_index_wins_among_equal_maxima", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", CONF, ids=_ids(CONF))
def test_confusion_update_equals_bincount(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_confusion_update_equals_bincount", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})
