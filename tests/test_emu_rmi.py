"""tests/test_gpu_rmi.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test bodies run
the HIP sources of csrc/rmi.hip through the C-ABI and kernels.rmi_pool / rmi_cov / rmi_solve / rmi_loss -- pooled maps and route, loss
and gradient, covariances, the solve stage, determinism, the refusals, the four contrast criteria with contrast.use_rmi -- in ascending
wave order and once more in descending order (the block partials and the wave reductions must not depend on it). Not replayed: the
memory assertion (no allocator to ask)."""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_rmi"
ORDERS = ["asc", "desc"]

POOL = _cases(MOD, "test_pooled_maps_and_route_match_float64")
LOSS = _cases(MOD, "test_loss_and_gradient_match_the_reference")
COV = _cases(MOD, "test_covariances_match_the_centred_float64_product")
SOLVE = _cases(MOD, "test_solve_matches_torch_float64_autograd")
CRIT = _cases(MOD, "test_contrast_criteria_with_use_rmi")


def _run(monkeypatch, order, func, kw):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", POOL, ids=_ids(POOL))
def test_pooled_maps_and_route_match_float64(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_pooled_maps_and_route_match_float64", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", LOSS, ids=_ids(LOSS))
def test_loss_and_gradient_match_the_reference(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_loss_and_gradient_match_the_reference", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", COV, ids=_ids(COV))
def test_covariances_match_the_centred_float64_product(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_covariances_match_the_centred_float64_product", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", SOLVE, ids=_ids(SOLVE))
def test_solve_matches_torch_float64_autograd(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_solve_matches_torch_float64_autograd", kw)


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_are_bit_identical(order, monkeypatch):
    _run(monkeypatch, order, "test_two_calls_are_bit_identical", {})


@pytest.mark.parametrize("order", ORDERS)
def test_refusals(order, monkeypatch):
    _run(monkeypatch, order, "test_refusals", {})


@pytest.mark.parametrize("kw", CRIT, ids=_ids(CRIT))
def test_contrast_criteria_with_use_rmi(kw, monkeypatch):
    _run(monkeypatch, "asc", "test_contrast_criteria_with_use_rmi", kw)


def test_without_use_rmi_the_criteria_are_unchanged(monkeypatch):
    _run(monkeypatch, "asc", "test_without_use_rmi_the_criteria_are_unchanged", {})
