"""tests/test_gpu_ocr_fused.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the HIP sources of csrc/ocr.hip through the C-ABI and the autograd wrappers -- parity with the torch composition (the
cases of at most 300 pixels), the raw entry points with their guard regions, determinism, refusals, what autograd keeps for the
backward pass, the routing of the two modules. Not replayed: the full-size cases, the whole-model and SGD-step legs, the capture."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_ocr_fused"
_SMALL = lambda kw: kw["case"][3] * kw["case"][4] <= 300

ATTN = _cases(MOD, "test_fused_attention_matches_the_torch_composition", _SMALL)


@pytest.mark.parametrize("kw", ATTN, ids=_ids(ATTN))
def test_fused_attention_matches_the_torch_composition(kw, monkeypatch):
    _replay(monkeypatch, MOD, "test_fused_attention_matches_the_torch_composition", dict(kw, monkeypatch=monkeypatch))


GATHER = _cases(MOD, "test_fused_gather_matches_the_torch_composition", _SMALL)


@pytest.mark.parametrize("kw", GATHER, ids=_ids(GATHER))
def test_fused_gather_matches_the_torch_composition(kw, monkeypatch):
    _replay(monkeypatch, MOD, "test_fused_gather_matches_the_torch_composition", dict(kw, monkeypatch=monkeypatch))


RAW = _cases(MOD, "test_ocr_entry_points_match_fp64_einsums")


@pytest.mark.parametrize("kw", RAW, ids=_ids(RAW))
def test_ocr_entry_points_match_fp64_einsums(kw, monkeypatch):
    _replay(monkeypatch, MOD, "test_ocr_entry_points_match_fp64_einsums", kw)


def test_ocr_entry_points_are_deterministic(monkeypatch):
    _replay(monkeypatch, MOD, "test_ocr_entry_points_are_deterministic", {})


def test_ocr_entry_points_refuse_other_shapes(monkeypatch):
    _replay(monkeypatch, MOD, "test_ocr_entry_points_refuse_other_shapes", {})


def test_nothing_of_the_size_of_the_map_is_saved_for_backward(monkeypatch):
    _replay(monkeypatch, MOD, "test_nothing_of_the_size_of_the_map_is_saved_for_backward", {"monkeypatch": monkeypatch})


def test_ocr_routing(monkeypatch):
    _replay(monkeypatch, MOD, "test_ocr_routing", {"monkeypatch": monkeypatch})
