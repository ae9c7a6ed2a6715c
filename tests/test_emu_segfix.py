"""tests/test_gpu_segfix.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies run
the HIP source of csrc/segfix.hip through the C-ABI and kernels.segfix_shift -- every golden of the reference exactly, fp32 and int8
offsets with identical output, refined_ids == lut[refined], the changed-pixel counts, the padded batch, the odd alignments against
the numpy restatement, the refusals -- in ascending wave order and once more in descending order: the block reduction of the
changed-pixel count may not depend on it. The fused multiply-adds are std::fma there. Not replayed: the 1024 x 2048 image (half a
million fibers) and the Tester leg (it needs a device for the loader's transform)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_segfix"
ORDERS = ["asc", "desc"]

GOLDENS = _cases(MOD, "test_goldens_are_exact_for_both_offset_types")
PADDED = _cases(MOD, "test_padded_batch_refines_each_region_as_its_own_image")
ODD = _cases(MOD, "test_odd_alignments_equal_the_restatement")
LARGE = _cases(MOD, "test_large_images_equal_the_restatement", lambda kw: kw["H"] <= 256)


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", GOLDENS, ids=_ids(GOLDENS))
def test_goldens_are_exact_for_both_offset_types(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_goldens_are_exact_for_both_offset_types", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", PADDED, ids=_ids(PADDED))
def test_padded_batch_refines_each_region_as_its_own_image(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_padded_batch_refines_each_region_as_its_own_image", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", ODD, ids=_ids(ODD))
def test_odd_alignments_equal_the_restatement(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_odd_alignments_equal_the_restatement", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", LARGE, ids=_ids(LARGE))
def test_large_images_equal_the_restatement(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_large_images_equal_the_restatement", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_refined_ids_are_optional_and_two_calls_agree(order, monkeypatch):
    _run(monkeypatch, order, "test_refined_ids_are_optional_and_two_calls_agree", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})
