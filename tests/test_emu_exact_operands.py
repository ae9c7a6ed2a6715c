"""tests/exact_cases.py on the CPU emulation of the execution model (tests/emu): the kernel SOURCES, through the autograd-free entry
points of contrastiveseg_amd/kernels.py, on operands that leave nothing to round -- every result must equal the float64 convolution
bit for bit (torch.equal, no tolerance). The derivation is in the docstring of tests/exact_cases.py; the MI355X copy of the same
bodies is tests/test_gpu_exact_operands.py, which runs every configuration (this file runs the ones marked `emu`)."""
import os

import pytest
import torch

from tests import exact_cases as X
from tests.emu import build_emu

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
CPU = torch.device("cpu")


def _K(monkeypatch, arith=X.F16X3, env=None):
    from tests.emu import inject
    from contrastiveseg_amd import kernels as K
    inject.install(monkeypatch)
    X.setup(K, monkeypatch, arith, env)
    return K


@pytest.mark.parametrize("cfg", [c for c in X.CONFIGS if c["emu"]], ids=X.config_id)
def test_exact_operands(cfg, monkeypatch):
    X.run_config(_K(monkeypatch, cfg["arith"], cfg["env"]), CPU, cfg, X.EXACT_KINDS)


@pytest.mark.parametrize("i", X.EPILOGUE_EMU)
def test_epilogues_on_exact_and_degenerate_operands(i, monkeypatch):
    X.run_epilogue(_K(monkeypatch, X.EPILOGUE_CONFIGS[i][2]), CPU, X.EPILOGUE_CONFIGS[i])


@pytest.mark.parametrize("i", X.DEGENERATE_EMU)
def test_degenerate_operands(i, monkeypatch):
    X.run_degenerate(_K(monkeypatch, X.DEGENERATE_CONFIGS[i][2]), CPU, X.DEGENERATE_CONFIGS[i])


@pytest.mark.parametrize("arith", [X.F16X3, X.BF16X6])
def test_all_zero_input_and_gradient_through_autograd(arith, monkeypatch):
    X.run_autograd_zero_input(_K(monkeypatch, arith), CPU)


def test_grouped_launches(monkeypatch):
    X.run_group(_K(monkeypatch), CPU, X.GROUPS[0], X.EXACT_KINDS + ("zero_a", "zero_b"))


def test_fp32_paths(monkeypatch):
    K = _K(monkeypatch)
    X.run_conv3x3_fp32(K, CPU, (2, 48, 48, 9, 12), ("dense", "zero_a"))
    X.run_rgb_stem(K, CPU, (2, 10, 132), ("dense", "zero_b"))
    X.run_classifier(K, CPU, X.CLS_CASES[0], False, ("dense", "zero_a"))
    X.run_classifier(K, CPU, X.CLS_WIDE_CASES[0], True, ("dense", "zero_b"))
    X.run_classifier(K, CPU, X.CLS_WIDE_CASES[1], True, ("dense",))
