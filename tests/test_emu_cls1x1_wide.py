"""tests/test_gpu_cls1x1_wide.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the HIP sources of csrc/cls1x1_wide.hip through the C-ABI and the autograd wrappers -- module parity, the raw entry points,
determinism, the routing. Not replayed: the full-size case (16 900 pixels x 720 channels is hours on an emulator that switches fibres
at every matrix instruction) and the whole-model GPU leg."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_cls1x1_wide"

MODULE = _cases(MOD, "test_wide_classifier_with_folded_dropout_matches_the_reference_modules",
                lambda kw: kw["case"][3] * kw["case"][4] <= 1024)


@pytest.mark.parametrize("kw", MODULE, ids=_ids(MODULE))
def test_wide_classifier_with_folded_dropout_matches_the_reference_modules(kw, monkeypatch):
    _replay(monkeypatch, MOD, "test_wide_classifier_with_folded_dropout_matches_the_reference_modules", dict(kw, monkeypatch=monkeypatch))


RAW = _cases(MOD, "test_wide_entry_points_match_fp64_einsums")


@pytest.mark.parametrize("kw", RAW, ids=_ids(RAW))
def test_wide_entry_points_match_fp64_einsums(kw, monkeypatch):
    _replay(monkeypatch, MOD, "test_wide_entry_points_match_fp64_einsums", kw)


def test_wide_entry_points_are_deterministic(monkeypatch):
    _replay(monkeypatch, MOD, "test_wide_entry_points_are_deterministic", {})


def test_wide_entry_points_refuse_other_shapes(monkeypatch):
    _replay(monkeypatch, MOD, "test_wide_entry_points_refuse_other_shapes", {})


def test_wide_routing(monkeypatch):
    _replay(monkeypatch, MOD, "test_wide_routing", {"monkeypatch": monkeypatch})
