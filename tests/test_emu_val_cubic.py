"""tests/test_gpu_val_cubic.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies
run the HIP source of csrc/cubic_eval.hip through the C-ABI and kernels.cubic_argmax -- the fused map against the numpy float32
restatement of the rule bit for bit on both launch paths, map and prediction against float64, cubic against bilinear, the mirrored
operand against averaging first, the tie rule, either output alone, determinism, the refusals of wrapper and library, score_cubic
against the float64 argmax, the val loader's label files -- in ascending wave order and once more in descending order (the tiled path
hands data between waves through LDS: a result that depends on the order is a missing barrier). Not replayed: the Trainer legs (a
whole model)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_val_cubic"
ORDERS = ["asc", "desc"]

BITS = _cases(MOD, "test_fused_map_equals_the_restatement_bit_for_bit_on_every_path")
F64 = _cases(MOD, "test_fused_map_and_prediction_match_float64")
MIRROR = _cases(MOD, "test_mirrored_operand_equals_averaging_first")
SCORE = _cases(MOD, "test_score_cubic_counts_what_float64_predicts")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", BITS, ids=_ids(BITS))
def test_fused_map_equals_the_restatement_bit_for_bit_on_every_path(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_fused_map_equals_the_restatement_bit_for_bit_on_every_path", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", F64, ids=_ids(F64))
def test_fused_map_and_prediction_match_float64(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_fused_map_and_prediction_match_float64", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_cubic_differs_from_bilinear(order, monkeypatch):
    _run(monkeypatch, order, "test_cubic_differs_from_bilinear", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", MIRROR, ids=_ids(MIRROR))
def test_mirrored_operand_equals_averaging_first(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_mirrored_operand_equals_averaging_first", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_first_index_wins_among_equal_maxima(order, monkeypatch):
    _run(monkeypatch, order, "test_first_index_wins_among_equal_maxima", {})


@pytest.mark.parametrize("order", ORDERS)
def test_pred_alone_and_fused_alone(order, monkeypatch):
    _run(monkeypatch, order, "test_pred_alone_and_fused_alone", {})


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", SCORE, ids=_ids(SCORE))
def test_score_cubic_counts_what_float64_predicts(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_score_cubic_counts_what_float64_predicts", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_score_cubic_on_a_tensor_of_targets_and_a_mirrored_pair(order, monkeypatch):
    _run(monkeypatch, order, "test_score_cubic_on_a_tensor_of_targets_and_a_mirrored_pair", {})


def test_val_loader_yields_the_label_files_at_their_own_size(tmp_path, monkeypatch):
    _run(monkeypatch, "asc", "test_val_loader_yields_the_label_files_at_their_own_size", {"tmp_path": tmp_path})
