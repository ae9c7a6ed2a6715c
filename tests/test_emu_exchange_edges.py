"""tests/test_gpu_exchange_edges.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same
bodies (tests/exchange_cases.py) run the HIP sources of csrc/upcat.hip, csrc/fuse.hip and csrc/cseg_bilinear.h through
contrastiveseg_amd/kernels.py, once in ascending and once in descending wave order -- the band kernel hands its band and its
horizontal sums from wave to wave through LDS. The host build fuses nothing, so here the strict bound holds: float64 on the rounded
taps, without the term for the compiler's choice."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_exchange_edges"
ORDERS = ["asc", "desc"]

UPCAT = _cases(MOD, "test_upsample_concat_edges_match_float64_on_the_kernels_taps")
FUSE = _cases(MOD, "test_fuse_sum_relu_edges_match_float64_on_the_kernels_taps")
SUM = _cases(MOD, "test_nary_sum_is_the_left_to_right_fp32_sum")
REFUSALS = _cases(MOD, "test_exchange_refusals")


def _run(monkeypatch, order, func, kw, mp=False):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, dict(kw, monkeypatch=monkeypatch) if mp else kw)


def test_every_route_is_taken_for_its_own_reason(monkeypatch):
    _run(monkeypatch, "asc", "test_every_route_is_taken_for_its_own_reason", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", UPCAT, ids=_ids(UPCAT))
def test_upsample_concat_edges_match_float64_on_the_kernels_taps(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_upsample_concat_edges_match_float64_on_the_kernels_taps", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", FUSE, ids=_ids(FUSE))
def test_fuse_sum_relu_edges_match_float64_on_the_kernels_taps(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_fuse_sum_relu_edges_match_float64_on_the_kernels_taps", kw, mp=True)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", SUM, ids=_ids(SUM))
def test_nary_sum_is_the_left_to_right_fp32_sum(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_nary_sum_is_the_left_to_right_fp32_sum", kw)


def test_fan_out_of_five_falls_back_to_torch_adds(monkeypatch):
    _run(monkeypatch, "asc", "test_fan_out_of_five_falls_back_to_torch_adds", {})


@pytest.mark.parametrize("kw", REFUSALS, ids=_ids(REFUSALS))
def test_exchange_refusals(kw, monkeypatch):
    _run(monkeypatch, "asc", "test_exchange_refusals", kw)
